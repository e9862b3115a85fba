// receipts.hip.h -- a block's receipts end to end on the device (included by bulk_keccak.hip): per-receipt blooms, the EIP-2718
// receipt encodings written straight into the value array of the receipts trie, the block's bloom, the rlp(index) keys, and the
// index-keyed tries of the block (receipts, plus any lists that ride along) as ONE forest pass.
//
//   receipt i = [tx_type, when != 0] ++ rlp([status, cum_gas, bloom, [ [address, [topics...], data] ... ]])
//               src/types/receipt.zig:13-35 (which has no type prefix yet; tx_type 0 reproduces it), EIP-658, EIP-2718
//
//   rc_check_kernel      device form only: the offsets and flags a caller can lie about (a lane per entry)
//   rc_list_len_kernel   a riding list's item lengths in trie order (a lane per item)
//   rc_bloom_kernel      a lane per bloom item (a log's address or topic): hash it, OR addToBloom's three bits into its receipt's row
//   rc_size_kernel       a lane per receipt: its logs' lengths (each log's offset inside the logs list) and its own, from RLP's rules
//   (exclusive scan)     radix_sort.hip's tiled scan over the lengths of all values of the forest
//   rc_keys_kernel       a lane per value: its 64-bit offset, its key rlp(index) and that key's offset, in trie order
//   rc_encode_kernel     a WAVE per unit of work -- a receipt's head with its 256-byte bloom, or one log body -- writing into the
//                        value array; the head units OR their rows into the block's bloom on the way
//   rc_scatter_kernel    a wave per item of a riding list: index order -> trie order
//   rc_gather_kernel     a wave per receipt: its encoding back in index order for the caller who wants the bytes
//
// Trie order of n items keyed by rlp(index) (trie_build.hip: append_rlp_index_pairs): indices 1 .. 0x7f, then 0 (key 0x80), then
// 0x80 onward: seg::pos_of_index / index_of_pos / key_bytes_before of segment_lists.hip.h.  Plain C++ only: tests/emu.py compiles this file for the host.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/phant_gpu.h"
#include "absorb.hip.h"
#include "launch.h"
#include "receipts.h"
#include "rlp.h"
#include "segment_lists.hip.h"
#include "staging.h"
#include "trie_build.h"
#include "wave_util.hip.h"

namespace phant {

// the three bits src/types/receipt.zig:50-63 `addToBloom` sets for one hashed item, ORed into a 64-dword bloom
PHANT_DEV void bloom_add_digest(const Sponge& s, uint32_t* __restrict__ bloom) {
    // digest bytes 0..5 = the three big-endian 16-bit words (receipt.zig:53-55); lo[0] holds bytes 0..3
    // little-endian, hi[0] bytes 4..7
    const uint32_t w0 = ((s.lo[0] & 0xffu) << 8) | ((s.lo[0] >> 8) & 0xffu);
    const uint32_t w1 = (((s.lo[0] >> 16) & 0xffu) << 8) | (s.lo[0] >> 24);
    const uint32_t w2 = ((s.hi[0] & 0xffu) << 8) | ((s.hi[0] >> 8) & 0xffu);
    const uint32_t w[3] = {w0, w1, w2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint32_t bit_index = 0x07FFu - (w[i] & 0x07FFu);          // receipt.zig:56-57
        const uint32_t byte_index = bit_index >> 3;
        const uint32_t bit_value = 1u << (7u - (bit_index & 7u));       // receipt.zig:60
        atomicOr(&bloom[byte_index >> 2], bit_value << (8u * (byte_index & 3u)));  // byte -> its dword, little-endian
    }
}

namespace rc {

#define RC_HD __host__ __device__ inline

enum : uint32_t { F_INVALID = 1u, F_UNSUPPORTED = 2u };
// the call's control words (64-bit, device memory, zeroed): [0] low half = F_*, [1] = bytes of all receipts
constexpr size_t CTL_WORDS = 4;

struct In {  // device pointers in a kernel, host pointers in the host form's check
    const uint8_t* tx_type;
    const uint8_t* status;
    const uint64_t* cum_gas;
    const uint32_t* log_first;
    const uint8_t* address;
    const uint32_t* topic_first;
    const uint64_t* data_off;
    const uint8_t* topics;
    const uint8_t* data;
    uint32_t n, n_logs, n_topics;
    uint64_t data_bytes;
};

// ---- lengths, from rlp.h's rules
constexpr uint32_t BLOOM_FIELD = 3u + 256u;  // 0xb9 0x01 0x00 ++ bloom

struct LogLen {
    uint64_t topics_payload, data_len, payload, total;
};
RC_HD LogLen log_len(const In& in, uint32_t l) {
    LogLen r;
    const uint64_t d = in.data_off[l + 1u] - in.data_off[l];
    r.topics_payload = 33ull * (in.topic_first[l + 1u] - in.topic_first[l]);
    r.data_len = d;
    r.payload = 21u + hdr_len(r.topics_payload) + r.topics_payload + str_len(d, d == 1u ? in.data[in.data_off[l]] : 0u);
    r.total = hdr_len(r.payload) + r.payload;
    return r;
}
// receipt i's encoded length; logs_payload = the bytes of its log bodies; log_rel (may be null): each log's offset among them
RC_HD uint64_t receipt_len(const In& in, uint32_t i, uint64_t& logs_payload, uint32_t* log_rel) {
    uint64_t lp = 0;
    for (uint32_t l = in.log_first[i]; l < in.log_first[i + 1u]; ++l) {
        if (log_rel) log_rel[l] = (uint32_t)lp;  // (beyond 32 bits the receipt is refused and nobody reads this)
        lp += log_len(in, l).total;
    }
    logs_payload = lp;
    const uint64_t payload = 1u + uint_len(in.cum_gas[i]) + BLOOM_FIELD + hdr_len(lp) + lp;
    return (in.tx_type[i] ? 1u : 0u) + hdr_len(payload) + payload;
}
// most bytes the receipts of a block of this shape can take
inline uint64_t encoded_bound(uint32_t n, uint32_t n_logs, uint32_t n_topics, uint64_t data_bytes) {
    return (uint64_t)n * (1u + 9u + 1u + 9u + BLOOM_FIELD + 9u) + (uint64_t)n_logs * (9u + 21u + 9u + 9u) + 33ull * n_topics + data_bytes;
}

__global__ void __launch_bounds__(256) rc_check_kernel(In in, uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (i == 0u) {
        if (in.n) bad = in.log_first[0] != 0u || in.log_first[in.n] != in.n_logs;
        if (in.n_logs) bad = bad || in.topic_first[0] != 0u || in.topic_first[in.n_logs] != in.n_topics || in.data_off[0] != 0ull ||
                             in.data_off[in.n_logs] != in.data_bytes;
    }
    if (i < in.n) bad = bad || in.log_first[i + 1u] < in.log_first[i] || in.status[i] > 1u || in.tx_type[i] > 0x7fu;
    if (i < in.n_logs) bad = bad || in.topic_first[i + 1u] < in.topic_first[i] || in.data_off[i + 1u] < in.data_off[i];
    if (bad) atomicOr(ctl, (uint32_t)F_INVALID);
}

// len[p] = the length of the item at trie position p; ends != 0: the offsets run from 0 to `bytes` (device form)
__global__ void __launch_bounds__(256) rc_list_len_kernel(const uint64_t* __restrict__ off, uint32_t n, uint64_t bytes, uint32_t ends,
                                                          uint32_t* __restrict__ len, uint32_t* __restrict__ ctl) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t idx = seg::index_of_pos(p, n);
    const uint64_t b = off[idx], e = off[idx + 1u];
    uint32_t flags = 0;
    if (p == 0u && ends && (off[0] != 0ull || off[n] != bytes)) flags |= F_INVALID;
    if (e < b) flags |= F_INVALID;
    else if (e - b > 0xffffffffull) flags |= F_UNSUPPORTED;
    len[p] = flags ? 0u : (uint32_t)(e - b);
    if (flags) atomicOr(ctl, flags);
}

__global__ void __launch_bounds__(256) rc_bloom_kernel(In in, uint32_t* __restrict__ rows /* n x 64 dwords, zeroed */) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= in.n_logs + in.n_topics) return;
    uint32_t l, len;
    const uint8_t* p;
    if (k < in.n_logs) {
        l = k;
        p = in.address + 20ull * l;
        len = 20u;
    } else {
        const uint32_t t = k - in.n_logs;
        l = upper_bound(in.topic_first, in.n_logs + 1u, t) - 1u;
        p = in.topics + 32ull * t;
        len = 32u;
    }
    const uint32_t r = upper_bound(in.log_first, in.n + 1u, l) - 1u;
    Sponge s;
    keccak256_global(s, p, len);
    bloom_add_digest(s, rows + 64ull * r);
}

// receipt i sized: its logs' offsets and payload noted, its bytes counted (or the call flagged) -> its length, 0 when refused
PHANT_DEV uint32_t size_receipt(const In& in, uint32_t i, uint32_t* __restrict__ log_rel, uint32_t* __restrict__ logs_payload,
                                uint32_t* __restrict__ ctl) {
    uint64_t lp;
    const uint64_t total = receipt_len(in, i, lp, log_rel);
    const bool fits = total <= 0xffffffffull;
    logs_payload[i] = (uint32_t)lp;
    if (fits) atomicAdd(reinterpret_cast<unsigned long long*>(ctl) + 1, (unsigned long long)total);
    else atomicOr(ctl, (uint32_t)F_UNSUPPORTED);
    return fits ? (uint32_t)total : 0u;
}

__global__ void __launch_bounds__(256) rc_size_kernel(In in, uint32_t* __restrict__ len /* at the receipts' first position */,
                                                      uint32_t* __restrict__ log_rel, uint32_t* __restrict__ logs_payload,
                                                      uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= in.n) return;
    len[seg::pos_of_index(i, in.n)] = size_receipt(in, i, log_rel, logs_payload, ctl);
}

// meta = seg_first[n_tries + 1] ++ key_base[n_tries] (the keys of list t start at key_base[t]): the trie of value g
PHANT_DEV uint32_t trie_of(const uint32_t* __restrict__ meta, uint32_t n_tries, uint32_t g) {
    uint32_t t = 0;
    while (t + 1u < n_tries && meta[t + 1u] <= g) ++t;
    return t;
}

// value g's key rlp(index) and that key's offset
PHANT_DEV void write_key(const uint32_t* __restrict__ meta, uint32_t n_tries, uint32_t total, uint32_t key_total, uint32_t g,
                         uint32_t* __restrict__ key_off, uint8_t* __restrict__ keys) {
    if (g == total) {
        key_off[g] = key_total;
        return;
    }
    const uint32_t t = trie_of(meta, n_tries, g);
    const uint32_t p = g - meta[t], n = meta[t + 1u] - meta[t], idx = seg::index_of_pos(p, n);
    const uint32_t ko = meta[n_tries + 1u + t] + seg::key_bytes_before(p);
    key_off[g] = ko;
    (void)put_uint(keys + ko, idx);
}

// len = the scanned lengths
__global__ void __launch_bounds__(256) rc_keys_kernel(const uint32_t* __restrict__ len, const uint32_t* __restrict__ meta, uint32_t n_tries,
                                                      uint32_t total, uint32_t key_total, uint64_t* __restrict__ val_off,
                                                      uint32_t* __restrict__ key_off, uint8_t* __restrict__ keys) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > total) return;
    val_off[g] = len[g];
    write_key(meta, n_tries, total, key_total, g, key_off, keys);
}

// A small block (total < SMALL_PLAN_MAX values, at most SMALL_PLAN_LISTS riding lists): ONE workgroup sizes every value, scans
// the lengths and writes offsets and keys -- rc_list_len_kernel, rc_size_kernel, the scan and rc_keys_kernel in one launch.
// Lane tid owns the eight values 8 tid .. 8 tid + 7.
constexpr uint32_t SMALL_PLAN_MAX = 2048, SMALL_PLAN_LISTS = 4;
struct SmallLists {
    const uint64_t* off[SMALL_PLAN_LISTS];
};
__global__ void __launch_bounds__(256) rc_plan_small_kernel(In in, SmallLists lists, const uint32_t* __restrict__ meta, uint32_t n_tries,
                                                            uint32_t receipts_at, uint32_t total, uint32_t key_total,
                                                            uint32_t* __restrict__ log_rel, uint32_t* __restrict__ logs_payload,
                                                            uint32_t* __restrict__ ctl, uint64_t* __restrict__ val_off,
                                                            uint32_t* __restrict__ key_off, uint8_t* __restrict__ keys) {
    __shared__ uint32_t s_sum[2][256];
    const uint32_t tid = threadIdx.x;
    uint32_t len[8], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t g = 8u * tid + j;
        uint32_t v = 0;
        if (g < total) {
            const uint32_t t = trie_of(meta, n_tries, g);
            const uint32_t p = g - meta[t], n = meta[t + 1u] - meta[t], idx = seg::index_of_pos(p, n);
            if (t == receipts_at) v = size_receipt(in, idx, log_rel, logs_payload, ctl);
            else {
                const uint64_t* const off = lists.off[t < receipts_at ? t : t - 1u];
                const uint64_t b = off[idx], e = off[idx + 1u];
                if (e < b) atomicOr(ctl, (uint32_t)F_INVALID);
                else if (e - b > 0xffffffffull) atomicOr(ctl, (uint32_t)F_UNSUPPORTED);
                else v = (uint32_t)(e - b);
            }
        }
        len[j] = v;
        mine += v;
    }
    s_sum[0][tid] = mine;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t o = 1; o < 256u; o <<= 1) {  // inclusive scan of the lanes' sums, two buffers
        s_sum[cur ^ 1u][tid] = s_sum[cur][tid] + (tid >= o ? s_sum[cur][tid - o] : 0u);
        cur ^= 1u;
        __syncthreads();
    }
    uint32_t run = s_sum[cur][tid] - mine;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t g = 8u * tid + j;
        if (g <= total) {
            val_off[g] = run;
            write_key(meta, n_tries, total, key_total, g, key_off, keys);
        }
        run += len[j];
    }
}

// Unit u < n: receipt u's head -- type byte, list header, status, gas, the bloom field, the logs list's header.  Unit n + l: log l's
// body.  A wave per unit, `waves` of them stride over the units; val_off = the offsets of the receipts' values (trie order).
// Lane 0 writes a unit's few header bytes; rows, topics and data go out a byte per lane and step.
__global__ void __launch_bounds__(256) rc_encode_kernel(In in, const uint32_t* __restrict__ rows, const uint64_t* __restrict__ val_off,
                                                        const uint32_t* __restrict__ log_rel, const uint32_t* __restrict__ logs_payload,
                                                        uint8_t* __restrict__ vals, uint64_t val_cap, uint32_t waves,
                                                        uint32_t* __restrict__ block_bloom) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t acc = 0;
    for (uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6); u < in.n + in.n_logs; u += waves) {
        const bool head = u < in.n;
        const uint32_t l = head ? 0u : u - in.n;
        const uint32_t i = head ? u : upper_bound(in.log_first, in.n + 1u, l) - 1u;
        const uint32_t pos = seg::pos_of_index(i, in.n);
        if (val_off[pos + 1u] > val_cap) continue;  // (cannot happen: the array is sized from the same rules)
        uint8_t* const out = vals + val_off[pos];
        const uint64_t lp = logs_payload[i];
        const uint64_t payload = 1u + uint_len(in.cum_gas[i]) + BLOOM_FIELD + hdr_len(lp) + lp;
        const uint32_t at_status = (in.tx_type[i] ? 1u : 0u) + hdr_len(payload);
        const uint32_t at_bloom = at_status + 1u + uint_len(in.cum_gas[i]) + 3u;
        if (head) {
            if (lane == 0u) {
                uint8_t* o = out;
                if (in.tx_type[i]) *o++ = in.tx_type[i];
                o += put_hdr(o, 0xc0u, payload);
                *o++ = in.status[i] ? 0x01u : 0x80u;  // EIP-658: the integer 1 or 0
                o += put_uint(o, in.cum_gas[i]);
                o[0] = 0xb9u;
                o[1] = 0x01u;
                o[2] = 0x00u;
                (void)put_hdr(out + at_bloom + 256u, 0xc0u, lp);
            }
            const uint32_t w = rows[64ull * i + lane];
            acc |= w;
            uint8_t* const b = out + at_bloom + 4u * lane;
            b[0] = (uint8_t)w;
            b[1] = (uint8_t)(w >> 8);
            b[2] = (uint8_t)(w >> 16);
            b[3] = (uint8_t)(w >> 24);
            continue;
        }
        const LogLen ll = log_len(in, l);
        uint8_t* const o = out + at_bloom + 256u + hdr_len(lp) + log_rel[l];
        const uint32_t at_addr = hdr_len(ll.payload);
        const uint32_t at_topics = at_addr + 21u + hdr_len(ll.topics_payload);
        const uint64_t at_data = at_topics + ll.topics_payload;
        const uint8_t* const d = in.data + in.data_off[l];
        const bool bare = ll.data_len == 1u && d[0] < 0x80u;  // a single byte below 0x80 is its own encoding
        if (lane == 0u) {
            (void)put_hdr(o, 0xc0u, ll.payload);
            o[at_addr] = 0x94u;
            (void)put_hdr(o + at_addr + 21u, 0xc0u, ll.topics_payload);
            if (!bare) (void)put_hdr(o + at_data, 0x80u, ll.data_len);
        }
        if (lane < 20u) o[at_addr + 1u + lane] = in.address[20ull * l + lane];
        const uint8_t* const tp = in.topics + 32ull * in.topic_first[l];
        // (32 bits: the call's values, 33 bytes a topic and at least 288 a receipt among them, were bounded by 2^32 - 1 before this launch)
        const uint32_t topics_payload = (uint32_t)ll.topics_payload;
        for (uint32_t k = lane; k < topics_payload; k += 64u) {
            const uint32_t t = k / 33u, r = k - 33u * t;
            o[at_topics + k] = r ? tp[32u * t + r - 1u] : (uint8_t)0xa0u;
        }
        wave_copy(o + at_data + (bare ? 0u : hdr_len(ll.data_len)), d, ll.data_len, lane);
    }
    if (acc) atomicOr(&block_bloom[lane], acc);
}

// a riding list: item idx (index order, src_off) to its trie position (val_off = the offsets of the list's values)
__global__ void __launch_bounds__(256) rc_scatter_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off, uint32_t n,
                                                         const uint64_t* __restrict__ val_off, uint8_t* __restrict__ vals, uint64_t val_cap) {
    const uint32_t idx = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (idx >= n) return;
    const uint32_t p = seg::pos_of_index(idx, n);
    if (val_off[p + 1u] > val_cap || val_off[p + 1u] - val_off[p] != src_off[idx + 1u] - src_off[idx]) return;  // (cannot happen)
    wave_copy(vals + val_off[p], src + src_off[idx], src_off[idx + 1u] - src_off[idx], lane);
}

// the receipts back in index order: out_off (may be null) n + 1 offsets, out (may be null) the bytes
__global__ void __launch_bounds__(256) rc_gather_kernel(const uint8_t* __restrict__ vals, const uint64_t* __restrict__ val_off, uint32_t n,
                                                        uint8_t* __restrict__ out, uint64_t* __restrict__ out_off) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    const uint32_t k = n < 128u ? n : 128u;
    const uint64_t base = val_off[0], len0 = val_off[k] - val_off[k - 1u];  // index 0 sits at position k - 1
    // in front of index i in trie order: indices 1 .. i - 1 (i < k), or every index below i (i >= k)
    const uint64_t at = i == 0u ? 0ull : i < k ? val_off[i - 1u] - base + len0 : val_off[i] - base;
    const uint32_t p = seg::pos_of_index(i, n);
    if (out_off && lane == 0u) {
        out_off[i] = at;
        if (i == 0u) out_off[n] = val_off[n] - base;
    }
    if (out) wave_copy(out + at, vals + val_off[p], val_off[p + 1u] - val_off[p], lane);
}


// what the host form refuses before anything is copied; *total = the bytes of all receipts
inline int32_t check_host(const In& in, uint64_t* total, std::string& err) {
    const uint32_t n = in.n, nl = in.n_logs;
    if (n && (in.log_first[0] != 0u || in.log_first[n] != nl)) return err = "block_receipts: log_first does not run from 0 to n_logs", PHANT_E_INVALID_ARG;
    if (nl && (in.topic_first[0] != 0u || in.topic_first[nl] != in.n_topics || in.data_off[0] != 0ull || in.data_off[nl] != in.data_bytes))
        return err = "block_receipts: topic_first / data_off do not run from 0 to n_topics / data_bytes", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (in.log_first[i + 1u] < in.log_first[i] || in.status[i] > 1u || in.tx_type[i] > 0x7fu)
            return err = "block_receipts: log_first not monotone, status > 1 or tx_type > 0x7f", PHANT_E_INVALID_ARG;
    for (uint32_t l = 0; l < nl; ++l)
        if (in.topic_first[l + 1u] < in.topic_first[l] || in.data_off[l + 1u] < in.data_off[l])
            return err = "block_receipts: topic_first / data_off not monotone", PHANT_E_INVALID_ARG;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t lp;
        const uint64_t r = receipt_len(in, i, lp, nullptr);
        if (r > 0xffffffffull) return err = "block_receipts: a receipt's encoding exceeds 2^32 - 1 bytes", PHANT_E_UNSUPPORTED;
        sum += r;
    }
    *total = sum;
    return PHANT_OK;
}

}  // namespace rc

int32_t block_receipts(Workspaces& ws, hipStream_t st, ReceiptsArgs& a, bool dev, std::string& err) {
    using namespace rc;
    const uint32_t n = a.n, nl = a.n_logs, nt = a.n_topics, n_tries = a.n_lists + 1u;
    a.encoded_len = 0;
    In hin{a.tx_type, a.status, a.cum_gas, a.log_first, a.address, a.topic_first, a.data_off, a.topics, a.data, n, nl, nt, a.data_bytes};
    // ---- the forest's shape: trie t < receipts_at = list t, trie receipts_at = the receipts, the lists behind it follow
    std::vector<uint32_t> meta(2u * n_tries + 1u, 0u);
    std::vector<uint64_t> lbytes(a.n_lists, 0), lfirst(a.n_lists, 0);
    uint64_t list_total = 0, key_total = 0, count = 0;
    for (uint32_t t = 0; t < n_tries; ++t) {
        const bool rcpt = t == a.receipts_at;
        const uint32_t l = t < a.receipts_at ? t : t - 1u, cnt = rcpt ? n : a.list_n[l];
        if (!rcpt && cnt) {
            if (dev) lbytes[l] = a.list_bytes[l];
            else {
                const uint64_t* o = a.list_off[l];
                for (uint32_t k = 0; k < cnt; ++k)
                    if (o[k + 1u] < o[k]) return err = "block_receipts: a list's item offsets are not monotone", PHANT_E_INVALID_ARG;
                lfirst[l] = o[0];
                lbytes[l] = o[cnt] - o[0];
            }
            list_total += lbytes[l];
        }
        meta[t] = (uint32_t)count;
        meta[n_tries + 1u + t] = (uint32_t)key_total;
        count += cnt;
        key_total += seg::key_bytes_before(cnt);
    }
    if (count >= 0x7fffffffull || key_total > 0xffffffffull) return err = "block_receipts: more than 2^31 - 2 items in one call", PHANT_E_UNSUPPORTED;
    const uint32_t total = (uint32_t)count, base_r = meta[a.receipts_at];
    meta[n_tries] = total;
    uint64_t rbytes = 0;  // the receipts' bytes: the host form knows them from its check, the device form reads them back
    if (!dev && n) {
        const int32_t rc = check_host(hin, &rbytes, err);
        if (rc) return rc;
    }
    const uint64_t val_cap = encoded_bound(n, nl, nt, a.data_bytes) + list_total;
    if (val_cap > 0xffffffffull) return err = "block_receipts: more than 4 GiB of trie values in one call", PHANT_E_UNSUPPORTED;

    // ---- the arena: (host form) the caller's arrays first, so that a small call crosses the bus in one copy
    In d = hin;
    std::vector<const uint8_t*> d_list(a.n_lists, nullptr);
    std::vector<const uint64_t*> d_loff(a.n_lists, nullptr);
    uint32_t *d_meta = nullptr, *d_rows = nullptr, *d_block = nullptr, *d_ctl = nullptr, *d_len = nullptr, *d_scan = nullptr, *d_log_rel = nullptr,
             *d_logs_payload = nullptr, *d_key_off = nullptr;
    uint64_t *d_val_off = nullptr, *d_enc_off = nullptr;
    uint8_t *d_zero = nullptr, *d_keys = nullptr, *d_vals = nullptr, *d_roots = nullptr, *d_enc = nullptr;
    const size_t zero_bytes = 256 * (size_t)n + 256 + 8 * CTL_WORDS + 4 * ((size_t)total + 1);
    const bool want_enc = a.encoded || a.encoded_off;
    auto carve = [&](auto& io) {
        if (!dev) {
            d.tx_type = io.template take<uint8_t>((size_t)n + 16);
            d.status = io.template take<uint8_t>((size_t)n + 16);
            d.cum_gas = io.template take<uint64_t>((size_t)n + 1);
            d.log_first = io.template take<uint32_t>((size_t)n + 1);
            d.address = io.template take<uint8_t>(20 * (size_t)nl + 16);
            d.topic_first = io.template take<uint32_t>((size_t)nl + 1);
            d.data_off = io.template take<uint64_t>((size_t)nl + 1);
            d.topics = io.template take<uint8_t>(32 * (size_t)nt + 16);
            d.data = io.template take<uint8_t>((size_t)a.data_bytes + 16);
            for (uint32_t l = 0; l < a.n_lists; ++l) {
                d_list[l] = io.template take<uint8_t>((size_t)lbytes[l] + 16);
                d_loff[l] = io.template take<uint64_t>((size_t)a.list_n[l] + 1);
            }
        }
        d_meta = io.template take<uint32_t>(meta.size());
        // what goes back to the caller, in one piece: roots, rows and the block's bloom (inside d_zero), the encodings
        d_roots = io.template take<uint8_t>(32 * (size_t)n_tries);
        d_zero = io.template take<uint8_t>(zero_bytes);
        if (!dev && want_enc) {
            d_enc_off = io.template take<uint64_t>((size_t)n + 1);
            d_enc = io.template take<uint8_t>((size_t)rbytes + 16);
        }
        d_scan = io.template take<uint32_t>(scan_scratch_entries(total + 1u) + 4);
        d_log_rel = io.template take<uint32_t>((size_t)nl + 1);
        d_logs_payload = io.template take<uint32_t>((size_t)n + 1);
        d_key_off = io.template take<uint32_t>((size_t)total + 1);
        d_val_off = io.template take<uint64_t>((size_t)total + 1);
        d_keys = io.template take<uint8_t>((size_t)key_total + 16);
        d_vals = io.template take<uint8_t>((size_t)val_cap + 16);
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_receipts", "workspace", err)) return rc;
    if (dev) {
        d_list.assign(a.lists, a.lists + a.n_lists);
        d_loff.assign(a.list_off, a.list_off + a.n_lists);
    }
    d_rows = reinterpret_cast<uint32_t*>(d_zero);
    d_block = d_rows + 64 * (size_t)n;
    d_ctl = d_block + 64;
    d_len = d_ctl + 2 * CTL_WORDS;
    CALL_TRY("block_receipts", ws.ensure_mailbox());
    static_assert(2 * CTL_WORDS <= Workspaces::MAILBOX_RECEIPTS_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_RECEIPTS;  // (behind everything the trie builder writes)

    // ---- in
    if (!dev) {
        std::vector<std::vector<uint64_t>> rel(a.n_lists);
        StagedInputs ins(ws, st, d.tx_type, d_meta + meta.size());
        ins.put(d.tx_type, a.tx_type, n);
        ins.put(d.status, a.status, n);
        ins.put(d.cum_gas, a.cum_gas, 8 * (size_t)n);
        if (n) ins.put(d.log_first, a.log_first, 4 * ((size_t)n + 1));
        ins.put(d.address, a.address, 20 * (size_t)nl);
        if (nl) ins.put(d.topic_first, a.topic_first, 4 * ((size_t)nl + 1));
        if (nl) ins.put(d.data_off, a.data_off, 8 * ((size_t)nl + 1));
        ins.put(d.topics, a.topics, 32 * (size_t)nt);
        ins.put(d.data, a.data, (size_t)a.data_bytes);
        for (uint32_t l = 0; l < a.n_lists; ++l) {
            if (!a.list_n[l]) continue;
            rel[l].resize((size_t)a.list_n[l] + 1);
            for (size_t k = 0; k < rel[l].size(); ++k) rel[l][k] = a.list_off[l][k] - lfirst[l];
            ins.put(d_list[l], a.lists[l] + lfirst[l], (size_t)lbytes[l]);
            ins.put(d_loff[l], rel[l].data(), 8 * rel[l].size());
        }
        ins.put(d_meta, meta.data(), 4 * meta.size());
        CALL_TRY("block_receipts", ins.finish());
        if (!ins.staged) CALL_TRY("block_receipts", hipStreamSynchronize(st));  // (the copies read `rel`, which goes at the end of this block)
    } else {
        CALL_TRY("block_receipts", hipMemcpyAsync(d_meta, meta.data(), 4 * meta.size(), hipMemcpyHostToDevice, st));
    }
    CALL_TRY("block_receipts", hipMemsetAsync(d_zero, 0, zero_bytes, st));

    // a small block: one workgroup sizes, scans and keys (the device form still checks its lists first, a launch each)
    const bool small = total < SMALL_PLAN_MAX && a.n_lists <= SMALL_PLAN_LISTS;
    // ---- lengths; the device form reads its verdict before any kernel indexes with the caller's offsets
    auto read_ctl = [&]() { return ws.read_words(Workspaces::MAILBOX_RECEIPTS, d_ctl, 2 * CTL_WORDS, st); };
    if (dev && (n || nl)) hipLaunchKernelGGL(rc_check_kernel, dim3(blocks_of((uint64_t)(n > nl ? n : nl) + 1, 256)), dim3(256), 0, st, d, d_ctl);
    for (uint32_t l = 0; l < a.n_lists; ++l) {
        const uint32_t t = l < a.receipts_at ? l : l + 1u;
        if (a.list_n[l] && (dev || !small))
            hipLaunchKernelGGL(rc_list_len_kernel, dim3(blocks_of(a.list_n[l], 256)), dim3(256), 0, st, d_loff[l], a.list_n[l], lbytes[l], dev ? 1u : 0u,
                               d_len + meta[t], d_ctl);
    }
    if (dev) {
        CALL_TRY("block_receipts", read_ctl());
        if (mb[0] & F_INVALID)
            return err = "block_receipts_dev: status > 1, tx_type > 0x7f, or offsets that are not monotone or do not span the stated totals", PHANT_E_INVALID_ARG;
    }
    if (n && nl + nt) hipLaunchKernelGGL(rc_bloom_kernel, dim3(blocks_of((uint64_t)nl + nt, 256)), dim3(256), 0, st, d, d_rows);
    if (small && total) {
        SmallLists sl{};
        for (uint32_t l = 0; l < a.n_lists; ++l) sl.off[l] = d_loff[l];
        hipLaunchKernelGGL(rc_plan_small_kernel, dim3(1), dim3(256), 0, st, d, sl, d_meta, n_tries, a.receipts_at, total, (uint32_t)key_total, d_log_rel,
                           d_logs_payload, d_ctl, d_val_off, d_key_off, d_keys);
    } else if (n) {
        hipLaunchKernelGGL(rc_size_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, d, d_len + base_r, d_log_rel, d_logs_payload, d_ctl);
    }
    if (dev) {
        CALL_TRY("block_receipts", read_ctl());
        if (mb[0] & F_INVALID) return err = "block_receipts_dev: a list's item offsets are not monotone", PHANT_E_INVALID_ARG;
        if (mb[0] & F_UNSUPPORTED) return err = "block_receipts_dev: a receipt or an item exceeds 2^32 - 1 bytes", PHANT_E_UNSUPPORTED;
        rbytes = (uint64_t)mb[2] | ((uint64_t)mb[3] << 32);
    }
    if (rbytes + list_total > 0xffffffffull) return err = "block_receipts: more than 4 GiB of trie values in one call", PHANT_E_UNSUPPORTED;
    a.encoded_len = rbytes;

    // ---- offsets, keys, values
    if (total && !small) {
        CALL_TRY("block_receipts", launch_exclusive_scan_u32(d_len, total + 1u, d_scan, st));
        hipLaunchKernelGGL(rc_keys_kernel, dim3(blocks_of((uint64_t)total + 1, 256)), dim3(256), 0, st, d_len, d_meta, n_tries, total, (uint32_t)key_total,
                           d_val_off, d_key_off, d_keys);
    }
    if (n) {
        const uint32_t units = n + nl, waves = 4u * std::min(blocks_of(units, 4), 2048u);
        hipLaunchKernelGGL(rc_encode_kernel, dim3(waves / 4u), dim3(256), 0, st, d, d_rows, d_val_off + base_r, d_log_rel, d_logs_payload, d_vals, val_cap,
                           waves, d_block);
    }
    for (uint32_t l = 0; l < a.n_lists; ++l) {
        const uint32_t t = l < a.receipts_at ? l : l + 1u;
        if (a.list_n[l])
            hipLaunchKernelGGL(rc_scatter_kernel, dim3(blocks_of(a.list_n[l], 4)), dim3(256), 0, st, d_list[l], d_loff[l], a.list_n[l], d_val_off + meta[t],
                               d_vals, val_cap);
    }
    CALL_TRY("block_receipts", hipGetLastError());

    // ---- the tries
    const bool want_roots = a.receipts_root || a.roots_out;
    if (want_roots) {
        const int32_t rc = trie_forest_dev(ws, st, TriePairs{d_keys, d_key_off, key_total, d_vals, d_val_off, rbytes + list_total, total, d_meta, n_tries, d_roots}, err);
        if (rc) return rc;
    }

    // ---- out
    // (a buffer nobody wants has no capacity to exceed: the other one is then written under its own bound alone)
    const bool fits = (!a.encoded || rbytes <= a.encoded_cap) && (!a.encoded_off || (uint64_t)n + 1 <= a.encoded_off_cap);
    if (want_enc && fits) {
        uint8_t* const o = dev ? a.encoded : (a.encoded ? d_enc : nullptr);
        uint64_t* const oo = dev ? a.encoded_off : (a.encoded_off ? d_enc_off : nullptr);
        if (n) hipLaunchKernelGGL(rc_gather_kernel, dim3(blocks_of(n, 4)), dim3(256), 0, st, d_vals, d_val_off + base_r, n, o, oo);
        else if (oo) CALL_TRY("block_receipts", hipMemsetAsync(oo, 0, 8, st));
        CALL_TRY("block_receipts", hipGetLastError());
    }
    // roots, rows and the block's bloom (inside d_zero) and the host form's encodings lie next to each other: one span in the host form
    // while it fits the pinned stage.  No control words go back: the device form has read them above, the host form needs none.
    CallOutputs outs(ws, st, dev, d_roots);
    outs.cover(d_enc ? d_enc + rbytes : d_zero + zero_bytes);
    outs.add(a.receipts_root, d_roots + 32 * (size_t)a.receipts_at, 32);
    outs.add(a.roots_out, d_roots, 32 * (size_t)n_tries);
    outs.add(a.logs_bloom, d_block, 256);
    outs.add(a.blooms, d_rows, 256 * (size_t)n);
    if (!dev && want_enc && fits) {
        outs.add(a.encoded, d_enc, (size_t)rbytes);
        outs.add(a.encoded_off, d_enc_off, 8 * ((size_t)n + 1));
    }
    CALL_TRY("block_receipts", outs.deliver());
    return PHANT_OK;
}

#undef RC_HD

}  // namespace phant
