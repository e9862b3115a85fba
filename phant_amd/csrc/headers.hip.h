// headers.hip.h -- block headers end to end on the device (included by bulk_keccak.hip): every header's fork-aware RLP encoding
// (src/types/block.zig:51-69), its hash, and src/blockchain/blockchain.zig:100-145 `validateBlockHeader` of every header against
// the one before it, for any number of independent chain segments in one call.
//
//   header i = rlp([parent_hash, uncle_hash, fee_recipient, state_root, transactions_root, receipts_root, logs_bloom,   (448 bytes
//                   difficulty, number, gas_limit, gas_used, timestamp, extra_data, prev_randao, nonce,                  at static
//                   base_fee, withdrawals_root, blob_gas_used, excess_blob_gas, parent_beacon_root, requests_hash])      positions)
//              cut after its first n_fields items
//
//   hdr_check_args_kernel  device form only: the arguments a caller can lie about (n_fields, extra_off, seg_first, a missing array), a
//                          lane per entry; the host reads the verdict before any other kernel indexes with them
//   hdr_size_kernel        a lane per header: its encoded length from RLP's rules
//   (exclusive scan)       radix_sort.hip's tiled scan over the lengths
//   hdr_plan_small_kernel  fewer than SMALL_MAX headers: ONE workgroup sizes and scans -- the two steps above in one launch
//   hdr_encode_kernel      a WAVE per header: lane 0 writes the few prefix and integer bytes, hashes, bloom and extra data go out
//                          a byte per lane and step (no alignment is asked of either side); notes the header's 64-bit offset
//   (keccak256_var_kernel) keccak_batch.hip's variable-length launch over the encodings: a lane per header
//   hdr_check_kernel       a lane per header: the twelve rules against the header before it (whose digest the launch above left in
//                          hashes[i - 1]) and the expected hash; the least flagged index by one atomic
//
// Plain C++ only: tests/emu.py compiles this file for the host.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/phant_gpu.h"
#include "headers.h"
#include "launch.h"
#include "rlp.h"
#include "staging.h"
#include "trie_build.h"
#include "wave_util.hip.h"

namespace phant {
namespace hd {

#define HD_HD __host__ __device__ inline

using In = phant_headers_in;  // device pointers in a kernel, host pointers in the host form's check

enum : uint32_t { F_INVALID = 1u };
// the call's control words (32-bit, device memory, zeroed): [0] = F_*, [1] = n - (the least flagged index) or 0, [2..3] = the
// bytes of all encodings (64-bit), [4] = extra_off[n] (device form)
constexpr size_t CTL_WORDS = 8;
// most bytes a header takes besides its extra data: two list and string headers of five bytes, the 445 static bytes, seven
// integers of nine, four more hashes of 33, the nonce's nine and a base fee of 33
constexpr uint64_t HEADER_BOUND = 700;
static_assert(5 + 445 + 7 * 9 + 5 + 4 * 33 + 9 + 33 <= HEADER_BOUND, "the bound covers a 21-field header");
constexpr uint32_t SMALL_MAX = 2048;
constexpr uint32_t STATIC_BYTES = 5u * 33u + 21u + 259u;  // the seven items in front of the first integer
// which optional arrays the caller left out
enum : uint32_t { NO_BASE_FEE = 1u, NO_WITHDRAWALS = 2u, NO_BLOB = 4u, NO_BEACON = 8u, NO_REQUESTS = 16u, NO_EXTRA = 32u };

HD_HD uint32_t null_mask(const In& in) {
    return (in.base_fee ? 0u : NO_BASE_FEE) | (in.withdrawals_root ? 0u : NO_WITHDRAWALS) | (in.blob_gas_used && in.excess_blob_gas ? 0u : NO_BLOB) |
           (in.parent_beacon_root ? 0u : NO_BEACON) | (in.requests_hash ? 0u : NO_REQUESTS) | (in.extra_data ? 0u : NO_EXTRA);
}
HD_HD bool fields_ok(uint32_t nf) { return nf == 15u || nf == 16u || nf == 17u || nf == 19u || nf == 20u || nf == 21u; }
// header i's n_fields and extra_off entries are what the interface says, and no array it needs is missing
HD_HD bool header_args_ok(const In& in, uint32_t i, uint32_t nulls) {
    const uint32_t nf = in.n_fields[i];
    if (!fields_ok(nf) || in.extra_off[i + 1u] < in.extra_off[i] || (i == 0u && in.extra_off[0] != 0u)) return false;
    if ((nulls & NO_EXTRA) && in.extra_off[i + 1u] != in.extra_off[i]) return false;
    return !((nf >= 16u && (nulls & NO_BASE_FEE)) || (nf >= 17u && (nulls & NO_WITHDRAWALS)) || (nf >= 19u && (nulls & NO_BLOB)) ||
             (nf >= 20u && (nulls & NO_BEACON)) || (nf == 21u && (nulls & NO_REQUESTS)));
}
// entry j of seg_first (j < n_segs) increases, and the ends are 0 and n
HD_HD bool seg_args_ok(const In& in, uint32_t j) {
    if (in.seg_first[j + 1u] <= in.seg_first[j]) return false;
    return j != 0u || (in.seg_first[0] == 0u && in.seg_first[in.n_segs] == in.n);
}

// the payload of header i's list (its arguments are sound: header_args_ok)
HD_HD uint64_t payload_len(const In& in, uint32_t i) {
    const uint32_t nf = in.n_fields[i];
    const uint64_t xl = in.extra_off[i + 1u] - in.extra_off[i];
    uint64_t p = STATIC_BYTES + uint_len(in.difficulty[i]) + uint_len(in.number[i]) + uint_len(in.gas_limit[i]) + uint_len(in.gas_used[i]) +
                 uint_len(in.timestamp[i]) + str_len(xl, xl == 1u ? in.extra_data[in.extra_off[i]] : 0u) + 33u + 9u;
    if (nf >= 16u) {
        const uint8_t* const f = in.base_fee + 32ull * i;
        p += str_len(be_bytes(f, 32u), f[31]);
    }
    if (nf >= 17u) p += 33u;
    if (nf >= 19u) p += uint_len(in.blob_gas_used[i]) + uint_len(in.excess_blob_gas[i]);
    if (nf >= 20u) p += 33u;
    if (nf >= 21u) p += 33u;
    return p;
}
HD_HD uint64_t header_len(const In& in, uint32_t i) {
    const uint64_t p = payload_len(in, i);
    return hdr_len(p) + p;
}
// ---- the expected base fee (EIP-1559, blockchain.zig:105-119) in exact arithmetic: 32-bit limbs, little-endian
struct Wide {
    uint32_t w[10];  // 320 bits: a 256-bit fee times a 64-bit gas delta
};
HD_HD void load_fee(const uint8_t* be, uint32_t w[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint8_t* p = be + 28 - 4 * k;
        w[k] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    }
}
// fee * delta / t / 8, floored at every step as the reference does (t != 0, t < 2^63 as it is half of a 64-bit limit)
HD_HD Wide fee_delta(const uint32_t fee[8], uint64_t delta, uint64_t t) {
    Wide p;
    const uint32_t d0 = (uint32_t)delta, d1 = (uint32_t)(delta >> 32);
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {  // column k of the schoolbook product: fee[k] d0 + fee[k - 1] d1
        const uint64_t a = k < 8 ? (uint64_t)fee[k] * d0 : 0ull, b = (k >= 1 && k <= 8) ? (uint64_t)fee[k - 1] * d1 : 0ull;
        const uint64_t lo = (carry & 0xffffffffull) + (a & 0xffffffffull) + (b & 0xffffffffull);
        p.w[k] = (uint32_t)lo;
        carry = (carry >> 32) + (a >> 32) + (b >> 32) + (lo >> 32);
    }
    // shift-subtract division by t: the remainder stays below t < 2^63, so doubling it never leaves 64 bits
    uint64_t rem = 0;
#pragma unroll
    for (int k = 9; k >= 0; --k) {
        const uint32_t w = p.w[k];
        uint32_t q = 0;
        for (int bit = 31; bit >= 0; --bit) {
            rem = (rem << 1) | ((w >> bit) & 1u);
            q <<= 1;
            if (rem >= t) rem -= t, q |= 1u;
        }
        p.w[k] = q;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) p.w[k] = (p.w[k] >> 3) | (k < 9 ? p.w[k + 1] << 29 : 0u);
    return p;
}
// does `have` (a header's 32-byte field) equal the fee that follows from the parent's fee, gas_used and gas_limit?
HD_HD bool base_fee_ok(const uint8_t* parent_fee, uint64_t p_gas_used, uint64_t p_gas_limit, const uint8_t* have) {
    const uint64_t t = p_gas_limit / 2u;
    uint32_t fee[8], got[8];
    load_fee(parent_fee, fee);
    load_fee(have, got);
    Wide e;
#pragma unroll
    for (int k = 0; k < 10; ++k) e.w[k] = k < 8 ? fee[k] : 0u;
    if (p_gas_used != t) {
        if (t == 0u) return false;  // (the reference divides by zero)
        const bool up = p_gas_used > t;
        Wide d = fee_delta(fee, up ? p_gas_used - t : t - p_gas_used, t);
        if (up) {
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 10; ++k) any |= d.w[k];
            if (!any) d.w[0] = 1u;  // max(delta, 1)
        }
        uint64_t c = 0;  // carry, or borrow (the delta going down is at most an eighth of the fee)
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            if (up) {
                c += (uint64_t)e.w[k] + d.w[k];
                e.w[k] = (uint32_t)c;
                c >>= 32;
            } else {
                const uint64_t s = (uint64_t)e.w[k] - d.w[k] - c;
                e.w[k] = (uint32_t)s;
                c = (s >> 32) & 1u;
            }
        }
    }
    bool same = e.w[8] == 0u && e.w[9] == 0u;  // (a value beyond 2^256 - 1 equals no field)
#pragma unroll
    for (int k = 0; k < 8; ++k) same = same && e.w[k] == got[k];
    return same;
}

// keccak256(0xc0): block.zig:13 empty_uncle_hash
HD_HD uint8_t empty_uncle_byte(uint32_t k) {
    const uint8_t h[32] = {0x1d, 0xcc, 0x4d, 0xe8, 0xde, 0xc7, 0x5d, 0x7a, 0xab, 0x85, 0xb5, 0x67, 0xb6, 0xcc, 0xd4, 0x1a,
                           0xd3, 0x12, 0x45, 0x1b, 0x94, 0x8a, 0x74, 0x13, 0xf0, 0xa1, 0x42, 0xfd, 0x40, 0xd4, 0x93, 0x47};
    return h[k];
}
HD_HD bool same32(const uint8_t* a, const uint8_t* b) {
    uint32_t diff = 0;
    for (uint32_t k = 0; k < 32u; ++k) diff |= (uint32_t)(a[k] ^ b[k]);
    return diff == 0u;
}
// bits 0 .. 11 of header i against header i - 1, whose digest is parent_digest
HD_HD uint32_t check_pair(const In& in, uint32_t i, const uint8_t* parent_digest) {
    const uint32_t p = i - 1u;
    uint32_t f = 0;
    const uint64_t gl = in.gas_limit[i], pgl = in.gas_limit[p], md = pgl / 1024u;
    if (pgl + md >= pgl && gl >= pgl + md) f |= PHANT_HDR_GAS_LIMIT_TOO_HIGH;  // (a bound beyond 2^64 - 1 is above every limit)
    if (gl <= pgl - md) f |= PHANT_HDR_GAS_LIMIT_TOO_LOW;
    if (gl < 5000u) f |= PHANT_HDR_GAS_LIMIT_MINIMUM;
    if (in.gas_used[i] > gl) f |= PHANT_HDR_GAS_LIMIT_EXCEEDED;
    const bool has = in.n_fields[i] >= 16u, phas = in.n_fields[p] >= 16u;
    if (has != phas) f |= PHANT_HDR_BASE_FEE;
    else if (has && !base_fee_ok(in.base_fee + 32ull * p, in.gas_used[p], pgl, in.base_fee + 32ull * i)) f |= PHANT_HDR_BASE_FEE;
    if (in.timestamp[i] <= in.timestamp[p]) f |= PHANT_HDR_TIMESTAMP;
    if (in.number[p] == ~0ull || in.number[i] != in.number[p] + 1u) f |= PHANT_HDR_NUMBER;
    if (in.extra_off[i + 1u] - in.extra_off[i] > 32u) f |= PHANT_HDR_EXTRA_DATA;
    if (in.difficulty[i] != 0u) f |= PHANT_HDR_DIFFICULTY;
    uint32_t nz = 0, ud = 0;
    for (uint32_t k = 0; k < 8u; ++k) nz |= in.nonce[8ull * i + k];
    if (nz) f |= PHANT_HDR_NONCE;
#pragma unroll
    for (uint32_t k = 0; k < 32u; ++k) ud |= (uint32_t)(in.uncle_hash[32ull * i + k] ^ empty_uncle_byte(k));
    if (ud) f |= PHANT_HDR_UNCLE_HASH;
    if (!same32(in.parent_hash + 32ull * i, parent_digest)) f |= PHANT_HDR_PARENT_HASH;
    return f;
}

// Device form only: what a caller can lie about, a lane per entry, before any kernel indexes with it.  ctl[4] = extra_off[n], from
// which the host bounds the encodings' bytes.
__global__ void __launch_bounds__(256) hdr_check_args_kernel(In in, uint32_t nulls, uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (in.seg_first && i < in.n_segs) bad = !seg_args_ok(in, i);
    if (i < in.n) bad = bad || !header_args_ok(in, i, nulls);
    if (bad) atomicOr(ctl, (uint32_t)F_INVALID);
    if (i == 0u) ctl[4] = in.extra_off[in.n];
}

__global__ void __launch_bounds__(256) hdr_size_kernel(In in, uint32_t* __restrict__ len) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < in.n) len[i] = (uint32_t)header_len(in, i);  // (32 bits: the call's bound on all encodings is below 2^32)
}

// n < SMALL_MAX: ONE workgroup sizes and scans; lane tid owns the eight headers 8 tid .. 8 tid + 7; enc_off = the n + 1 offsets
__global__ void __launch_bounds__(256) hdr_plan_small_kernel(In in, uint64_t* __restrict__ enc_off) {
    __shared__ uint32_t s_sum[2][256];
    const uint32_t tid = threadIdx.x;
    uint32_t len[8], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t i = 8u * tid + j;
        len[j] = i < in.n ? (uint32_t)header_len(in, i) : 0u;
        mine += len[j];
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
        const uint32_t i = 8u * tid + j;
        if (i <= in.n) enc_off[i] = run;
        run += len[j];
    }
}

// A wave per header, `waves` of them stride over the call.  off32 != null: the scanned 32-bit lengths, widened into enc_off on the
// way (the large call); null: enc_off is already there (hdr_plan_small_kernel).
__global__ void __launch_bounds__(256) hdr_encode_kernel(In in, const uint32_t* __restrict__ off32, uint64_t* __restrict__ enc_off,
                                                         uint8_t* __restrict__ enc, uint64_t enc_cap, uint32_t waves) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < in.n; i += waves) {
        const uint64_t at = off32 ? (uint64_t)off32[i] : enc_off[i], end = off32 ? (uint64_t)off32[i + 1u] : enc_off[i + 1u];
        if (off32 && lane == 0u) {
            enc_off[i] = at;
            if (i + 1u == in.n) enc_off[in.n] = end;
        }
        const uint64_t payload = payload_len(in, i);
        if (end > enc_cap || end - at != hdr_len(payload) + payload) continue;  // (cannot happen: sized from the same rules)
        const uint32_t nf = in.n_fields[i];
        uint8_t* const s = enc + at + hdr_len(payload);  // the static part: 5 hashes, the address, the bloom
        const uint8_t* const h32[5] = {in.parent_hash, in.uncle_hash, in.state_root, in.transactions_root, in.receipts_root};
        const uint32_t h_at[5] = {0u, 33u, 87u, 120u, 153u};
        if (lane == 0u) {
            (void)put_hdr(enc + at, 0xc0u, payload);
#pragma unroll
            for (int k = 0; k < 5; ++k) s[h_at[k]] = 0xa0u;
            s[66] = 0x94u;
            s[186] = 0xb9u, s[187] = 0x01u, s[188] = 0x00u;
        }
        if (lane < 32u) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s[h_at[k] + 1u + lane] = h32[k][32ull * i + lane];
        }
        if (lane < 20u) s[67u + lane] = in.fee_recipient[20ull * i + lane];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) s[189u + 64u * k + lane] = in.logs_bloom[256ull * i + 64u * k + lane];
        // the tail: every lane knows where its items sit, lane 0 writes the integers and the prefixes
        const uint64_t ints[5] = {in.difficulty[i], in.number[i], in.gas_limit[i], in.gas_used[i], in.timestamp[i]};
        uint8_t* t = s + STATIC_BYTES;
        if (lane == 0u) {
            uint8_t* o = t;
#pragma unroll
            for (int k = 0; k < 5; ++k) o += put_uint(o, ints[k]);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) t += uint_len(ints[k]);
        const uint64_t xl = in.extra_off[i + 1u] - in.extra_off[i];
        const uint8_t* const x = in.extra_data + in.extra_off[i];
        const bool bare = xl == 1u && x[0] < 0x80u;  // a single byte below 0x80 is its own encoding
        const uint32_t xh = bare ? 0u : hdr_len(xl);
        if (lane == 0u && !bare) (void)put_hdr(t, 0x80u, xl);
        wave_copy(t + xh, x, xl, lane);
        t += xh + xl;
        if (lane == 0u) t[0] = 0xa0u, t[33] = 0x88u;
        if (lane < 32u) t[1u + lane] = in.prev_randao[32ull * i + lane];
        if (lane < 8u) t[34u + lane] = in.nonce[8ull * i + lane];
        t += 42u;
        if (nf >= 16u) {
            const uint8_t* const f = in.base_fee + 32ull * i;
            const uint32_t nb = be_bytes(f, 32u), fl = (uint32_t)str_len(nb, f[31]);
            if (lane == 0u) {
                if (nb == 0u) t[0] = 0x80u;
                else if (fl == 1u) t[0] = f[31];
                else t[0] = (uint8_t)(0x80u + nb);
            }
            if (fl > 1u && lane < nb) t[1u + lane] = f[32u - nb + lane];
            t += fl;
        }
        if (nf >= 17u) {
            if (lane == 0u) t[0] = 0xa0u;
            if (lane < 32u) t[1u + lane] = in.withdrawals_root[32ull * i + lane];
            t += 33u;
        }
        if (nf >= 19u) {
            if (lane == 0u) (void)put_uint(t + put_uint(t, in.blob_gas_used[i]), in.excess_blob_gas[i]);
            t += uint_len(in.blob_gas_used[i]) + uint_len(in.excess_blob_gas[i]);
        }
        if (nf >= 20u) {
            if (lane == 0u) t[0] = 0xa0u;
            if (lane < 32u) t[1u + lane] = in.parent_beacon_root[32ull * i + lane];
            t += 33u;
        }
        if (nf >= 21u) {
            if (lane == 0u) t[0] = 0xa0u;
            if (lane < 32u) t[1u + lane] = in.requests_hash[32ull * i + lane];
        }
    }
}

// hashes = the digests of all n headers (stream order: behind the Keccak launch); lane 0 notes the encodings' bytes for the host
__global__ void __launch_bounds__(256) hdr_check_kernel(In in, const uint8_t* __restrict__ hashes, const uint64_t* __restrict__ enc_off,
                                                        uint32_t* __restrict__ flags, uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= in.n) return;
    if (i == 0u) ctl[2] = (uint32_t)enc_off[in.n], ctl[3] = (uint32_t)(enc_off[in.n] >> 32);
    bool anchor = i == 0u;
    if (in.seg_first && i) anchor = in.seg_first[upper_bound(in.seg_first, in.n_segs + 1u, i) - 1u] == i;
    uint32_t f = anchor ? 0u : check_pair(in, i, hashes + 32ull * (i - 1u));
    if (in.expected_hash && !same32(in.expected_hash + 32ull * i, hashes + 32ull * i)) f |= PHANT_HDR_EXPECTED_HASH;
    if (flags) flags[i] = f;
    if (f) atomicMax(ctl + 1, in.n - i);
}

// what the host form refuses before anything is copied
inline int32_t check_host(const In& in, std::string& err) {
    const uint32_t nulls = null_mask(in);
    if (in.seg_first)
        for (uint32_t j = 0; j < in.n_segs; ++j)
            if (!seg_args_ok(in, j)) return err = "header_chain: seg_first does not increase from 0 to n", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < in.n; ++i)
        if (!header_args_ok(in, i, nulls))
            return err = "header_chain: an n_fields outside 15, 16, 17, 19, 20, 21, a NULL array that a header needs, or extra_off not running up from 0", PHANT_E_INVALID_ARG;
    return PHANT_OK;
}

// the arrays with a fixed width per header: X(member, element type, elements per header)
#define HD_ARRAYS(X)                                                                                                                  \
    X(parent_hash, uint8_t, 32) X(uncle_hash, uint8_t, 32) X(fee_recipient, uint8_t, 20) X(state_root, uint8_t, 32)                     \
    X(transactions_root, uint8_t, 32) X(receipts_root, uint8_t, 32) X(logs_bloom, uint8_t, 256) X(difficulty, uint64_t, 1)              \
    X(number, uint64_t, 1) X(gas_limit, uint64_t, 1) X(gas_used, uint64_t, 1) X(timestamp, uint64_t, 1) X(prev_randao, uint8_t, 32)     \
    X(nonce, uint8_t, 8) X(base_fee, uint8_t, 32) X(withdrawals_root, uint8_t, 32) X(blob_gas_used, uint64_t, 1)                        \
    X(excess_blob_gas, uint64_t, 1) X(parent_beacon_root, uint8_t, 32) X(requests_hash, uint8_t, 32) X(n_fields, uint8_t, 1)            \
    X(expected_hash, uint8_t, 32)

}  // namespace hd

int32_t header_chain(Workspaces& ws, hipStream_t st, const phant_headers_in& hin, phant_headers_out& out, bool dev, std::string& err) {
    using namespace hd;
    const uint32_t n = hin.n, nulls = null_mask(hin);
    const bool small = n < SMALL_MAX;  // (n + 1 offsets, eight a lane)
    const uint32_t grid = blocks_of((uint64_t)n, 256);
    CALL_TRY("header_chain", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_HEADERS_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_HEADERS;

    // ---- the arguments: the host form checks before anything is copied, the device form on the device -- and reads the verdict
    // before any kernel indexes with the caller's offsets.  Either way the extra data's bytes are known afterwards.
    uint64_t extra_bytes = 0;
    uint32_t* d_ctl = nullptr;
    if (!dev) {
        const int32_t rc = check_host(hin, err);
        if (rc) return rc;
        extra_bytes = hin.extra_off[n];
    } else {
        // (the control words alone, in the trie builder's first arena, which this call does not use otherwise: the call's own
        // arena is sized from what this launch reports)
        auto carve_ctl = [&](auto& t1) { d_ctl = t1.template take<uint32_t>(CTL_WORDS); };
        if (const int32_t rc = lay_out_status(lay_out_arena(ws.t1, st, carve_ctl), "header_chain_dev", "workspace", err)) return rc;
        CALL_TRY("header_chain", hipMemsetAsync(d_ctl, 0, 4 * CTL_WORDS, st));
        hipLaunchKernelGGL(hdr_check_args_kernel, dim3(grid), dim3(256), 0, st, hin, nulls, d_ctl);
        CALL_TRY("header_chain", hipGetLastError());
        CALL_TRY("header_chain", ws.read_words(Workspaces::MAILBOX_HEADERS, d_ctl, CTL_WORDS, st));
        if (mb[0] & F_INVALID)
            return err = "header_chain_dev: an n_fields outside 15, 16, 17, 19, 20, 21, a NULL array that a header needs, extra_off not running up from 0, "
                         "or seg_first not increasing from 0 to n",
                   PHANT_E_INVALID_ARG;
        extra_bytes = mb[4];
    }
    const uint64_t enc_bound = HEADER_BOUND * n + extra_bytes;
    if (enc_bound > 0xffffffffull) return err = "header_chain: the encodings may take 4 GiB or more (700 n + the extra data's bytes)", PHANT_E_UNSUPPORTED;

    // ---- the arena: (host form) the caller's arrays first, so that a small call crosses the bus in one copy
    In d = hin;
    uint32_t *d_len = nullptr, *d_scan = nullptr, *d_flags = nullptr;
    uint64_t* d_enc_off = nullptr;
    uint8_t *d_hashes = nullptr, *d_enc = nullptr;
    auto carve = [&](auto& io) {
        if (!dev) {
#define X(m, T, k) d.m = hin.m ? io.template take<T>((size_t)n * k + 16) : nullptr;
            HD_ARRAYS(X)
#undef X
            d.extra_data = hin.extra_data ? io.template take<uint8_t>((size_t)extra_bytes + 16) : nullptr;
            d.extra_off = io.template take<uint32_t>((size_t)n + 1);
            d.seg_first = hin.seg_first ? io.template take<uint32_t>((size_t)hin.n_segs + 1) : nullptr;
            d_ctl = io.template take<uint32_t>(CTL_WORDS);
        }
        // what goes back to the caller, in one piece behind the control words: digests, flags, offsets, encodings
        d_hashes = io.template take<uint8_t>(32 * (size_t)n);
        d_flags = io.template take<uint32_t>((size_t)n);
        d_enc_off = io.template take<uint64_t>((size_t)n + 1);
        d_enc = io.template take<uint8_t>((size_t)enc_bound + 16);
        if (!small) {
            d_len = io.template take<uint32_t>((size_t)n + 4);
            d_scan = io.template take<uint32_t>(scan_scratch_entries(n + 1u) + 4);
        }
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "header_chain", "workspace", err)) return rc;

    // ---- in
    if (!dev) {
        StagedInputs ins(ws, st, ws.io.base, d_ctl);
#define X(m, T, k) ins.put(d.m, hin.m, (size_t)n * k * sizeof(T));
        HD_ARRAYS(X)
#undef X
        ins.put(d.extra_data, hin.extra_data, (size_t)extra_bytes);
        ins.put(d.extra_off, hin.extra_off, 4 * ((size_t)n + 1));
        ins.put(d.seg_first, hin.seg_first, 4 * ((size_t)hin.n_segs + 1));
        CALL_TRY("header_chain", ins.finish());
        CALL_TRY("header_chain", hipMemsetAsync(d_ctl, 0, 4 * CTL_WORDS, st));
    }

    // ---- lengths and offsets, encodings, digests, checks
    if (small) hipLaunchKernelGGL(hdr_plan_small_kernel, dim3(1), dim3(256), 0, st, d, d_enc_off);
    else {
        hipLaunchKernelGGL(hdr_size_kernel, dim3(grid), dim3(256), 0, st, d, d_len);
        CALL_TRY("header_chain", hipMemsetAsync(d_len + n, 0, 4, st));
        CALL_TRY("header_chain", launch_exclusive_scan_u32(d_len, n + 1u, d_scan, st));
    }
    const uint32_t waves = 4u * std::min(blocks_of(n, 4), 4096u);
    hipLaunchKernelGGL(hdr_encode_kernel, dim3(waves / 4u), dim3(256), 0, st, d, small ? nullptr : d_len, d_enc_off, d_enc, enc_bound, waves);
    CALL_TRY("header_chain", hipGetLastError());
    CALL_TRY("header_chain", launch_keccak256_var(d_enc, d_enc_off, n, d_hashes, st));
    hipLaunchKernelGGL(hdr_check_kernel, dim3(grid), dim3(256), 0, st, d, d_hashes, d_enc_off, d_flags, d_ctl);
    CALL_TRY("header_chain", hipGetLastError());

    // ---- out: the control words, digests, flags and offsets lie next to each other (one span in the host form while it fits the pinned
    // stage); the control words first, since only they tell the encodings' size, which follow by a copy of their own when wanted
    CallOutputs outs(ws, st, dev, d_ctl, d_ctl, Workspaces::MAILBOX_HEADERS, CTL_WORDS);
    outs.cover(d_enc_off + n + 1);
    CALL_TRY("header_chain", outs.deliver());
    const uint32_t bad_from_end = outs.ctl()[1];
    const uint64_t total = (uint64_t)outs.ctl()[2] | ((uint64_t)outs.ctl()[3] << 32);
    const bool fits = !out.enc || total <= out.enc_cap;  // (a buffer nobody wants has no capacity to exceed)
    outs.add(out.hashes, d_hashes, 32 * (size_t)n);
    outs.add(out.flags, d_flags, 4 * (size_t)n);
    if (fits) {
        outs.add(out.enc_off, d_enc_off, 8 * ((size_t)n + 1));
        outs.add(out.enc, d_enc, (size_t)total);
    }
    CALL_TRY("header_chain", outs.deliver());
    out.first_bad = n - bad_from_end;
    out.enc_len = total;
    return PHANT_OK;
}

#undef HD_HD
#undef HD_ARRAYS

}  // namespace phant
