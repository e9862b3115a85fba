// filters.hip.h -- log filters over a chain segment (included by bulk_keccak.hip behind requests.hip.h): which
// logs of the rows block_receipt_segments leaves decoded does each of many filters select (phant_block_log_filters), and which 2048-bit
// blooms can hold a match at all (phant_log_filters_bloom).  include/phant_gpu.h has the contract, tests/filters_ref.py the same in Python.
//
// A set is a run of entries: filter f's address set is the entries [addr_first[f], addr_first[f + 1]) of `addr`, its topic set of
// position p the entries [topic_first[4 f + p], topic_first[4 f + p + 1]) of `topic`.  An entry has ONE number over both arrays -- an
// address its index, a topic n_addr + its index --, so "entry e belongs to set s" is a range test, and a table slot that holds e names
// the set with it.
//
//   lf_check_kernel   device form only: seg::first_flags over every first array of the rows and of the filters, the filters' ranges,
//                     and the entries of the sets above linear_max; the host reads the verdict before anything indexes with them
//   lf_table_kernel   only when a set is above linear_max: a lane per entry of such a set claims a slot of ONE keyed:: table, keyed by
//                     (the set's first entry, the value) with the ctx's salts; equal values of one set share a slot
//   lf_count_kernel   a wave per (filter, 64 consecutive logs): the filter's sets are uniform across the wave -- a set of up to linear_max
//                     entries is compared entry by entry from wave-uniform loads, a larger one looked up in the table, the set and all
//                     value bytes compared on a hit; a wave whose logs lie wholly outside [block_lo, block_hi) leaves before it reads a
//                     log; its 64-bit ballot and the ballot's popcount
//   (exclusive scan)  radix_sort.hip's over the popcounts
//   lf_emit_kernel    a wave per ballot: the set lanes write their log's index where the scan says; behind them a lane per filter:
//                     filter_first, filter_count
//   lf_bits_kernel    (bloom call) a lane per entry: keccak256_global over its 20 or 32 bytes, the three bit positions kept
//   lf_screen_kernel  (bloom call) a workgroup per tile of 64 blooms: the tile (16 KB) into LDS once with 16-byte loads, transposed --
//                     dword w of bloom j in row w --, then its four waves loop over all filters, a lane per bloom; a wave's ballot is
//                     the `may` word, its popcount goes to may_count by one atomic add
//
// Three launches (the scan's among them; four with a table), two for the bloom call, the device forms' check one more, whatever
// n_filters, n_logs and n_blooms are.  Plain C++ plus the cross-lane builtins keyed_table.hip.h uses: tests/emu.py compiles this file
// for the host.
#pragma once
#include "absorb.hip.h"
#include "filters_check.h"
#include "keyed_table.hip.h"
#include "segment_lists.hip.h"
#include "staging.h"

namespace phant {
namespace lf {

// the call's control words (device memory, zeroed): [0] = seg::F_INVALID of the check, [1] = entries of the sets above linear_max (the
// device form's check counts them), [2] = n_matches
constexpr uint32_t CTL_WORDS = 4, CTL_LARGE = 1, CTL_MATCHES = 2;
constexpr uint32_t TILE_BLOOMS = 64, BLOOM_DWORDS = 64;

struct Filters {
    const uint32_t *addr_first, *topic_first, *block_lo, *block_hi;
    const uint8_t *addr, *topic;
    uint32_t n_filters, n_addr, n_topic;
    uint32_t n_range;  // blocks, or blooms: what block_lo / block_hi index

    PHANT_DEV uint32_t lo(uint32_t f) const { return block_lo ? block_lo[f] : 0u; }
    PHANT_DEV uint32_t hi(uint32_t f) const { return block_hi ? block_hi[f] : n_range; }
};

struct Match {
    Filters f;
    const uint32_t *block_first, *log_first, *topic_first;
    const uint8_t *address, *topics;
    uint32_t n_blocks, n, n_logs, n_topics;
    uint32_t n_chunks;  // ceil(n_logs / 64)
    uint32_t n_waves;   // n_filters x n_chunks: ballot f * n_chunks + c
    uint32_t match_cap, linear_max;
    uint32_t* table;  // PHANT_ROW_NONE, or an entry
    uint32_t mask, salt0, salt1;
    uint32_t* ctl;
    uint64_t* ballots;  // n_waves
    uint32_t* counts;   // n_waves + 1, the last zeroed; scanned in place: a ballot's first row, [n_waves] = n_matches
    uint32_t *filter_first, *filter_count, *match_log;
};

struct __attribute__((packed, aligned(1))) PackedWord { uint32_t x; };

// a value as words: 5 of an address, 8 of a topic (bytes of any alignment, and none behind the value)
template <int N>
PHANT_DEV void load_value(const uint8_t* __restrict__ p, uint32_t (&w)[8]) {
    const PackedU32x4 a = *reinterpret_cast<const PackedU32x4*>(p);
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    if (N == 5) {
        w[4] = reinterpret_cast<const PackedWord*>(p + 16)->x;
        w[5] = w[6] = w[7] = 0u;
    } else {
        const PackedU32x4 b = *reinterpret_cast<const PackedU32x4*>(p + 16);
        w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    }
}
template <int N>
PHANT_DEV bool same_value(const uint8_t* __restrict__ p, const uint32_t (&w)[8]) {
    uint32_t v[8];
    load_value<N>(p, v);
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) d |= v[k] ^ w[k];
    return d == 0u;
}
// where (set, value) is looked for first: every word of the value and the set's first entry, under the ctx's key
PHANT_DEV uint32_t home_of(uint32_t set_first, const uint32_t (&w)[8], uint32_t salt0, uint32_t salt1) {
    const uint32_t more[5] = {w[5], w[6], w[7], set_first, 0u};
    return keyed::home_slot(more, keyed::home_slot(w, salt0, salt1), salt1);
}

// entry e (an address below n_addr, a topic from there on): its bytes
PHANT_DEV const uint8_t* entry_bytes(const Filters& f, uint32_t e) { return e < f.n_addr ? f.addr + 20ull * e : f.topic + 32ull * (e - f.n_addr); }

// ---- the device form's check: a lane per entry of each first array
__global__ void __launch_bounds__(256) lf_check_kernel(Match q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const Filters& f = q.f;
    uint32_t bad = 0, large = 0;
    if (i < q.n_blocks) bad |= seg::first_flags(q.block_first, i, q.n_blocks, q.n);
    if (i < q.n) bad |= seg::first_flags(q.log_first, i, q.n, q.n_logs);
    if (i < q.n_logs) bad |= seg::first_flags(q.topic_first, i, q.n_logs, q.n_topics);
    if (i < f.n_filters) {
        bad |= seg::first_flags(f.addr_first, i, f.n_filters, f.n_addr);
        const uint32_t lo = f.lo(i), hi = f.hi(i), size = f.addr_first[i + 1u] - f.addr_first[i];
        if (lo > hi || hi > f.n_range) bad |= seg::F_INVALID;
        if (!bad && size > q.linear_max) large += size;
    }
    if (i < 4u * f.n_filters) {
        const uint32_t flags = seg::first_flags(f.topic_first, i, 4u * f.n_filters, f.n_topic), size = f.topic_first[i + 1u] - f.topic_first[i];
        bad |= flags;
        if (!flags && size > q.linear_max) large += size;
    }
    if (bad) atomicOr(q.ctl, bad);
    if (large) atomicAdd(q.ctl + CTL_LARGE, large);
}

// ---- the table over the entries of the sets above linear_max
__global__ void __launch_bounds__(256) lf_table_kernel(Match q) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const Filters& f = q.f;
    if (e >= f.n_addr + f.n_topic) return;
    const bool is_addr = e < f.n_addr;
    uint32_t s0, s1;  // my set's entries
    if (is_addr) {
        const uint32_t s = upper_bound(f.addr_first, f.n_filters + 1u, e) - 1u;
        s0 = f.addr_first[s], s1 = f.addr_first[s + 1u];
    } else {
        const uint32_t s = upper_bound(f.topic_first, 4u * f.n_filters + 1u, e - f.n_addr) - 1u;
        s0 = f.n_addr + f.topic_first[s], s1 = f.n_addr + f.topic_first[s + 1u];
    }
    if (s1 - s0 <= q.linear_max) return;
    uint32_t w[8];
    if (is_addr) load_value<5>(entry_bytes(f, e), w);
    else load_value<8>(entry_bytes(f, e), w);
    keyed::claim(q.table, q.mask, home_of(s0, w, q.salt0, q.salt1), e, [&](uint32_t old) {
        if (old < s0 || old >= s1) return false;
        return is_addr ? same_value<5>(entry_bytes(f, old), w) : same_value<8>(entry_bytes(f, old), w);
    });
}

// is the value w (N words at 20- or 32-byte entries) in the set of entries [s0, s1) (numbered over both arrays), s1 > s0
template <int N>
PHANT_DEV bool in_set(const Match& q, uint32_t s0, uint32_t s1, const uint32_t (&w)[8]) {
    const Filters& f = q.f;
    if (s1 - s0 <= q.linear_max) {  // (uniform across the wave: s0, s1 and the entries' addresses)
        bool hit = false;
        for (uint32_t e = s0; e < s1; ++e) hit = hit || same_value<N>(entry_bytes(f, e), w);
        return hit;
    }
    return keyed::find(q.table, q.mask, home_of(s0, w, q.salt0, q.salt1),
                       [&](uint32_t j) { return j >= s0 && j < s1 && same_value<N>(entry_bytes(f, j), w); }) != PHANT_ROW_NONE;
}

PHANT_DEV uint32_t block_of_log(const Match& q, uint32_t l) { return seg::block_of(q.block_first, q.n_blocks, upper_bound(q.log_first, q.n + 1u, l) - 1u); }

PHANT_DEV bool log_matches(const Match& q, uint32_t fi, uint32_t l, uint32_t lo, uint32_t hi) {
    const Filters& f = q.f;
    const uint32_t b = block_of_log(q, l);
    if (b < lo || b >= hi) return false;
    uint32_t w[8];
    const uint32_t a0 = f.addr_first[fi], a1 = f.addr_first[fi + 1u];
    if (a1 != a0) {
        load_value<5>(q.address + 20ull * l, w);
        if (!in_set<5>(q, a0, a1, w)) return false;
    }
    const uint32_t t = q.topic_first[l], tc = q.topic_first[l + 1u] - t;
    for (uint32_t p = 0; p < 4u; ++p) {
        const uint32_t t0 = f.topic_first[4u * fi + p], t1 = f.topic_first[4u * fi + p + 1u];
        if (t1 == t0) continue;
        if (tc <= p) return false;
        load_value<8>(q.topics + 32ull * (t + p), w);
        if (!in_set<8>(q, f.n_addr + t0, f.n_addr + t1, w)) return false;
    }
    return true;
}

// ---- count: a wave per (filter, 64 logs)
__global__ void __launch_bounds__(256) lf_count_kernel(Match q) {
    const uint32_t wv = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (wv >= q.n_waves) return;  // (whole waves)
    const uint32_t fi = wv / q.n_chunks, c = wv - fi * q.n_chunks, l0 = 64u * c, l = l0 + lane;
    const uint32_t last = l0 + 63u < q.n_logs ? l0 + 63u : q.n_logs - 1u;
    const uint32_t lo = q.f.lo(fi), hi = q.f.hi(fi);
    // the blocks of the wave's first and last log: nothing of [lo, hi) between them -- no log is read
    if (lo >= hi || block_of_log(q, last) < lo || block_of_log(q, l0) >= hi) {
        if (lane == 0u) q.ballots[wv] = 0ull, q.counts[wv] = 0u;
        return;
    }
    const bool hit = l < q.n_logs && log_matches(q, fi, l, lo, hi);
    const unsigned long long ballot = __ballot(hit);
    if (lane == 0u) q.ballots[wv] = ballot, q.counts[wv] = (uint32_t)__popcll(ballot);
}

// ---- emit: counts scanned; a wave per ballot, then a lane per filter and one more
__global__ void __launch_bounds__(256) lf_emit_kernel(Match q) {
    const uint64_t t = blockIdx.x * 256ull + threadIdx.x, per_wave = 64ull * q.n_waves;
    const uint32_t total = q.counts[q.n_waves];
    if (t >= per_wave) {
        const uint64_t fi = t - per_wave;
        if (fi > q.f.n_filters) return;
        const uint32_t first = q.counts[fi * q.n_chunks];  // (fi == n_filters: counts[n_waves])
        q.filter_first[fi] = first;
        if (fi < q.f.n_filters) q.filter_count[fi] = q.counts[(fi + 1u) * q.n_chunks] - first;
        else q.ctl[CTL_MATCHES] = total;
        return;
    }
    if (total > q.match_cap) return;  // (match_log has match_cap rows at most: nothing of it is written)
    const uint32_t wv = (uint32_t)(t >> 6), lane = (uint32_t)t & 63u;
    const unsigned long long ballot = q.ballots[wv];
    if (!(ballot >> lane & 1ull)) return;
    const uint32_t row = q.counts[wv] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    q.match_log[row] = 64u * (wv % q.n_chunks) + lane;
}

// ---- the bloom call
struct Screen {
    Filters f;
    const uint8_t* blooms;
    uint32_t n_blooms, n_words;  // ceil(n_blooms / 64)
    uint64_t* bits;              // per entry: its three positions, 11 bits each: (dword of the bloom) << 5 | (bit of that dword)
    uint32_t* ctl;
    uint64_t* may;        // n_filters x n_words
    uint32_t* may_count;  // n_filters, zeroed
};

__global__ void __launch_bounds__(256) lf_bloom_check_kernel(Screen q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const Filters& f = q.f;
    uint32_t bad = 0;
    if (i < f.n_filters) {
        bad |= seg::first_flags(f.addr_first, i, f.n_filters, f.n_addr);
        const uint32_t lo = f.lo(i), hi = f.hi(i);
        if (lo > hi || hi > f.n_range) bad |= seg::F_INVALID;
    }
    if (i < 4u * f.n_filters) bad |= seg::first_flags(f.topic_first, i, 4u * f.n_filters, f.n_topic);
    if (bad) atomicOr(q.ctl, bad);
}

__global__ void __launch_bounds__(256) lf_bits_kernel(Screen q) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= q.f.n_addr + q.f.n_topic) return;
    Sponge s;
    keccak256_global(s, entry_bytes(q.f, e), e < q.f.n_addr ? 20u : 32u);
    // digest bytes 0..5 = three big-endian 16-bit words (bloom_add_digest of receipts.hip.h sets the same bits)
    const uint32_t v[3] = {((s.lo[0] & 0xffu) << 8) | ((s.lo[0] >> 8) & 0xffu), (((s.lo[0] >> 16) & 0xffu) << 8) | (s.lo[0] >> 24),
                           ((s.hi[0] & 0xffu) << 8) | ((s.hi[0] >> 8) & 0xffu)};
    uint64_t code = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint32_t bit_index = 0x07FFu - (v[i] & 0x07FFu), byte_index = bit_index >> 3;
        const uint32_t in_dword = 8u * (byte_index & 3u) + (7u - (bit_index & 7u));  // the bloom's byte k in dword k / 4, little-endian
        code |= (uint64_t)((byte_index >> 2) << 5 | in_dword) << (11 * i);
    }
    q.bits[e] = code;
}

// dword w of the tile's bloom j: row w, and inside the row turned by 2 (w / 4) columns -- the 32 lanes of a half wave that STORE the
// dwords 4 m + k (m = 0 .. 15) of two neighbouring blooms then hit 32 different banks, and the lanes that READ one dword of 64
// neighbouring blooms still read 64 consecutive columns (modulo 64)
PHANT_DEV uint32_t tile_at(uint32_t w, uint32_t j) { return w * TILE_BLOOMS + ((j + ((w >> 2) << 1)) & (TILE_BLOOMS - 1u)); }

// some entry of [s0, s1) has its three bits in bloom j of the tile (s1 > s0)
PHANT_DEV bool any_in_bloom(const uint64_t* __restrict__ bits, uint32_t s0, uint32_t s1, const uint32_t* tile, uint32_t j) {
    bool any = false;
    for (uint32_t e = s0; e < s1; ++e) {
        const uint64_t code = bits[e];  // (uniform across the wave)
        uint32_t all = 1u;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t c = (uint32_t)(code >> (11 * i)) & 0x7ffu;
            all &= tile[tile_at(c >> 5, j)] >> (c & 31u);
        }
        any = any || (all & 1u);
    }
    return any;
}

__global__ void __launch_bounds__(256) lf_screen_kernel(Screen q) {
    __shared__ uint32_t tile[BLOOM_DWORDS * TILE_BLOOMS];
    const uint32_t tile_no = blockIdx.x, b0 = TILE_BLOOMS * tile_no;
    // 1 024 pieces of 16 bytes, consecutive lanes consecutive pieces; blooms behind the last are zeros and are not read
    for (uint32_t piece = threadIdx.x; piece < BLOOM_DWORDS * TILE_BLOOMS / 4u; piece += 256u) {
        const uint32_t j = piece >> 4, w = 4u * (piece & 15u);
        PackedU32x4 v = {0u, 0u, 0u, 0u};
        if (b0 + j < q.n_blooms) v = *reinterpret_cast<const PackedU32x4*>(q.blooms + 256ull * (b0 + j) + 4u * w);
        tile[tile_at(w, j)] = v.x, tile[tile_at(w + 1u, j)] = v.y, tile[tile_at(w + 2u, j)] = v.z, tile[tile_at(w + 3u, j)] = v.w;
    }
    __syncthreads();
    const Filters& f = q.f;
    const uint32_t lane = threadIdx.x & 63u, b = b0 + lane;
    for (uint32_t fi = threadIdx.x >> 6; fi < f.n_filters; fi += 4u) {  // (uniform across the wave)
        bool ok = b < q.n_blooms && b >= f.lo(fi) && b < f.hi(fi);
        const uint32_t a0 = f.addr_first[fi], a1 = f.addr_first[fi + 1u];
        if (ok && a1 != a0) ok = any_in_bloom(q.bits, a0, a1, tile, lane);
        for (uint32_t p = 0; p < 4u; ++p) {
            const uint32_t t0 = f.topic_first[4u * fi + p], t1 = f.topic_first[4u * fi + p + 1u];
            if (ok && t1 != t0) ok = any_in_bloom(q.bits, f.n_addr + t0, f.n_addr + t1, tile, lane);
        }
        const unsigned long long ballot = __ballot(ok);
        if (lane == 0u) {
            q.may[(uint64_t)fi * q.n_words + tile_no] = ballot;
            if (ballot) atomicAdd(q.may_count + fi, (uint32_t)__popcll(ballot));
        }
    }
}

// the filters' arrays into the arena (host form), or as they came (device form)
template <class IO>
void take_filters(IO& io, Filters& f, const phant_log_filters& in) {
    take_input(io, f.addr_first, (size_t)in.n_filters + 1, true);
    take_input(io, f.topic_first, 4 * (size_t)in.n_filters + 1, true);
    take_input(io, f.addr, 20 * (size_t)in.n_addr, in.n_addr != 0u);
    take_input(io, f.topic, 32 * (size_t)in.n_topic, in.n_topic != 0u);
    take_input(io, f.block_lo, (size_t)in.n_filters, in.block_lo != nullptr);
    take_input(io, f.block_hi, (size_t)in.n_filters, in.block_hi != nullptr);
}
inline void put_filters(StagedInputs& ins, const Filters& f, const phant_log_filters& in) {
    ins.put(f.addr_first, in.addr_first, 4 * ((size_t)in.n_filters + 1));
    ins.put(f.topic_first, in.topic_first, 4 * (4 * (size_t)in.n_filters + 1));
    ins.put(f.addr, in.addr, 20 * (size_t)in.n_addr);
    ins.put(f.topic, in.topic, 32 * (size_t)in.n_topic);
    ins.put(f.block_lo, in.block_lo, 4 * (size_t)in.n_filters);
    ins.put(f.block_hi, in.block_hi, 4 * (size_t)in.n_filters);
}
inline Filters filters_of(const phant_log_filters& in, uint32_t n_range) {
    return Filters{in.addr_first, in.topic_first, in.block_lo, in.block_hi, in.addr, in.topic, in.n_filters, in.n_addr, in.n_topic, n_range};
}

}  // namespace lf

// phant_block_log_filters[_dev]: check_match_args has passed and n_filters != 0.  sets: PHANT_DIAG_LOGFILTER_SETS
int32_t block_log_filters(Workspaces& ws, hipStream_t st, const phant_logmatch_in& in, const phant_log_filters& fl, phant_logmatch_out& out, bool dev,
                          const uint32_t salt[2], uint32_t linear_max, std::string& err) {
    using namespace lf;
    const char* const call = dev ? "block_log_filters_dev" : "block_log_filters";
    const uint32_t nb = in.n_blocks, n = in.n, nl = in.n_logs, nt = in.n_topics, nf = fl.n_filters;
    CALL_TRY("block_log_filters", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_LF_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_LF;
    if (!dev) {
        if (nb)
            if (const int32_t rc = check_rows_host(call, in, err)) return rc;
        if (const int32_t rc = check_filters_host(call, fl, nb, err)) return rc;
    }
    if (too_many_words(nf, nl)) return err = std::string(call) + ": n_filters x ceil(n_logs / 64) is 2^31 or more", PHANT_E_UNSUPPORTED;
    if ((uint64_t)fl.n_addr + fl.n_topic >= 0x40000000ull) return err = std::string(call) + ": 2^30 or more entries in the filters' sets", PHANT_E_UNSUPPORTED;

    Match q;
    std::memset(&q, 0, sizeof q);
    q.f = filters_of(fl, nb);
    q.block_first = in.block_first, q.log_first = in.log_first, q.topic_first = in.topic_first, q.address = in.address, q.topics = in.topics;
    q.n_blocks = nb, q.n = n, q.n_logs = nl, q.n_topics = nt, q.n_chunks = blocks_of(nl, 64), q.n_waves = nf * q.n_chunks;
    q.match_cap = in.match_cap, q.linear_max = linear_max, q.salt0 = salt[0], q.salt1 = salt[1];
    const uint32_t waves = q.n_waves, entries = fl.n_addr + fl.n_topic, slots = keyed::table_slots(entries);
    const size_t rows = (size_t)std::min<uint64_t>(in.match_cap, (uint64_t)nf * nl);
    q.mask = slots - 1u;
    uint32_t* d_scan = nullptr;
    const void *zero_end = nullptr, *outputs_end = nullptr, *inputs_begin = nullptr, *inputs_end = nullptr;
    auto carve = [&](auto& io) {
        q.ctl = io.template take<uint32_t>(CTL_WORDS);
        zero_end = io.template take<uint8_t>(0);
        q.filter_first = io.template take<uint32_t>((size_t)nf + 1);
        q.filter_count = io.template take<uint32_t>((size_t)nf);
        q.match_log = io.template take<uint32_t>(rows);
        outputs_end = io.template take<uint8_t>(0);
        q.counts = io.template take<uint32_t>((size_t)waves + 1 + 4);
        q.ballots = io.template take<uint64_t>((size_t)waves);
        q.table = io.template take<uint32_t>((size_t)slots);
        d_scan = io.template take<uint32_t>(scan_scratch_entries(waves + 1u));
        if (!dev) {
            inputs_begin = io.template take<uint8_t>(0);
            take_input(io, q.block_first, (size_t)nb + 1, nb != 0u);
            take_input(io, q.log_first, (size_t)n + 1, n != 0u);
            take_input(io, q.address, 20 * (size_t)nl, nl != 0u);
            take_input(io, q.topic_first, (size_t)nl + 1, nl != 0u);
            take_input(io, q.topics, 32 * (size_t)nt, nt != 0u);
            take_filters(io, q.f, fl);
            inputs_end = io.template take<uint8_t>(0);
        }
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_log_filters", "workspace", err)) return rc;
    CALL_TRY("block_log_filters", hipMemsetAsync(q.ctl, 0, (size_t)(static_cast<const uint8_t*>(zero_end) - reinterpret_cast<uint8_t*>(q.ctl)), st));
    CALL_TRY("block_log_filters", hipMemsetAsync(q.counts + waves, 0, 4, st));

    // ---- in: (host form) every input in ONE copy through the pinned stage where they fit it; (device form) the check
    uint64_t large = 0;
    if (!dev) {
        StagedInputs ins(ws, st, inputs_begin, inputs_end);
        if (nb) ins.put(q.block_first, in.block_first, 4 * ((size_t)nb + 1));
        if (n) ins.put(q.log_first, in.log_first, 4 * ((size_t)n + 1));
        if (nl) {
            ins.put(q.address, in.address, 20 * (size_t)nl);
            ins.put(q.topic_first, in.topic_first, 4 * ((size_t)nl + 1));
            ins.put(q.topics, in.topics, 32 * (size_t)nt);
        }
        put_filters(ins, q.f, fl);
        CALL_TRY("block_log_filters", ins.finish());
        large = large_entries_host(fl, linear_max);
    } else {
        const uint32_t most = std::max(std::max(nb, n), std::max(nl, 4u * nf));
        hipLaunchKernelGGL(lf_check_kernel, dim3(blocks_of(most, 256)), dim3(256), 0, st, q);
        CALL_TRY("block_log_filters", hipGetLastError());
        CALL_TRY("block_log_filters", ws.read_words(Workspaces::MAILBOX_LF, q.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID)
            return err = "block_log_filters_dev: block_first, log_first, topic_first or a first array of the filters does not run from 0 to its total, or goes "
                         "backwards, or a filter's blocks are no range of the segment's",
                   PHANT_E_INVALID_ARG;
        large = mb[CTL_LARGE];
    }

    // ---- the table (only when a set goes through it), the ballots, one scan, the rows
    if (large) {
        CALL_TRY("block_log_filters", hipMemsetAsync(q.table, 0xff, 4 * (size_t)slots, st));
        hipLaunchKernelGGL(lf_table_kernel, dim3(blocks_of(entries, 256)), dim3(256), 0, st, q);
    }
    hipLaunchKernelGGL(lf_count_kernel, dim3(std::max(blocks_of(waves, 4), 1u)), dim3(256), 0, st, q);
    CALL_TRY("block_log_filters", hipGetLastError());
    CALL_TRY("block_log_filters", launch_exclusive_scan_u32(q.counts, waves + 1u, d_scan, st));
    hipLaunchKernelGGL(lf_emit_kernel, dim3(blocks_of(64ull * waves + nf + 1u, 256)), dim3(256), 0, st, q);
    CALL_TRY("block_log_filters", hipGetLastError());

    // ---- out: one span from the control words to the last per-filter output; the rows whose count only the control words tell follow
    CallOutputs outs(ws, st, dev, q.ctl, q.ctl, Workspaces::MAILBOX_LF, CTL_WORDS);
    if (!dev) outs.cover(q.match_log);
    outs.add(out.filter_first, q.filter_first, 4 * ((size_t)nf + 1));
    outs.add(out.filter_count, q.filter_count, 4 * (size_t)nf);
    CALL_TRY("block_log_filters", outs.deliver());
    out.n_matches = outs.ctl()[CTL_MATCHES];
    if (out.n_matches <= in.match_cap) outs.add(out.match_log, q.match_log, 4 * (size_t)out.n_matches);
    CALL_TRY("block_log_filters", outs.deliver());
    return PHANT_OK;
}

// phant_log_filters_bloom[_dev]: check_bloom_args has passed and n_filters != 0
int32_t log_filters_bloom(Workspaces& ws, hipStream_t st, const uint8_t* blooms, uint32_t n_blooms, const phant_log_filters& fl, uint64_t* may, uint32_t* may_count,
                          bool dev, std::string& err) {
    using namespace lf;
    const char* const call = dev ? "log_filters_bloom_dev" : "log_filters_bloom";
    const uint32_t nf = fl.n_filters;
    CALL_TRY("log_filters_bloom", ws.ensure_mailbox());
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_LF;
    if (!dev)
        if (const int32_t rc = check_filters_host(call, fl, n_blooms, err)) return rc;
    if (too_many_words(nf, n_blooms)) return err = std::string(call) + ": n_filters x ceil(n_blooms / 64) is 2^31 or more", PHANT_E_UNSUPPORTED;
    if ((uint64_t)fl.n_addr + fl.n_topic >= 0x40000000ull) return err = std::string(call) + ": 2^30 or more entries in the filters' sets", PHANT_E_UNSUPPORTED;

    Screen q;
    std::memset(&q, 0, sizeof q);
    q.f = filters_of(fl, n_blooms);
    q.blooms = blooms, q.n_blooms = n_blooms, q.n_words = blocks_of(n_blooms, 64);
    const size_t words = (size_t)nf * q.n_words, entries = (size_t)fl.n_addr + fl.n_topic;
    const void *zero_end = nullptr, *outputs_end = nullptr, *inputs_begin = nullptr, *inputs_end = nullptr;
    auto carve = [&](auto& io) {
        q.ctl = io.template take<uint32_t>(CTL_WORDS);
        q.may_count = io.template take<uint32_t>((size_t)nf);
        zero_end = io.template take<uint8_t>(0);
        q.may = io.template take<uint64_t>(words);
        outputs_end = io.template take<uint8_t>(0);
        q.bits = io.template take<uint64_t>(entries);
        if (!dev) {
            inputs_begin = io.template take<uint8_t>(0);
            take_input(io, q.blooms, 256 * (size_t)n_blooms, true);
            take_filters(io, q.f, fl);
            inputs_end = io.template take<uint8_t>(0);
        }
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "log_filters_bloom", "workspace", err)) return rc;
    CALL_TRY("log_filters_bloom", hipMemsetAsync(q.ctl, 0, (size_t)(static_cast<const uint8_t*>(zero_end) - reinterpret_cast<uint8_t*>(q.ctl)), st));
    if (!dev) {
        StagedInputs ins(ws, st, inputs_begin, inputs_end);
        ins.put(q.blooms, blooms, 256 * (size_t)n_blooms);
        put_filters(ins, q.f, fl);
        CALL_TRY("log_filters_bloom", ins.finish());
    } else {
        hipLaunchKernelGGL(lf_bloom_check_kernel, dim3(blocks_of(4ull * nf, 256)), dim3(256), 0, st, q);
        CALL_TRY("log_filters_bloom", hipGetLastError());
        CALL_TRY("log_filters_bloom", ws.read_words(Workspaces::MAILBOX_LF, q.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID)
            return err = "log_filters_bloom_dev: a first array of the filters does not run from 0 to its total, or goes backwards, or a filter's blooms are no range of the call's",
                   PHANT_E_INVALID_ARG;
    }
    hipLaunchKernelGGL(lf_bits_kernel, dim3(std::max(blocks_of(entries, 256), 1u)), dim3(256), 0, st, q);
    if (q.n_words) hipLaunchKernelGGL(lf_screen_kernel, dim3(q.n_words), dim3(256), 0, st, q);
    CALL_TRY("log_filters_bloom", hipGetLastError());

    CallOutputs outs(ws, st, dev, q.may_count);
    outs.add(may_count, q.may_count, 4 * (size_t)nf);
    outs.add(may, q.may, 8 * words);
    CALL_TRY("log_filters_bloom", outs.deliver());
    if (dev) CALL_TRY("log_filters_bloom", hipStreamSynchronize(st));
    return PHANT_OK;
}

}  // namespace phant
