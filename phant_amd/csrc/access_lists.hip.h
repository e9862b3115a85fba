// access_lists.hip.h -- a block's access lists (EIP-2930) decoded and joined with the pre-state tables of a witness (included by
// bulk_keccak.hip): what src/blockchain/blockchain.zig:284-295 turns into warm sets before the EVM runs, and the
// (account, slot) join the EVM host's getStorage needs for every warm slot.
//
//   al_check_args_kernel   device form only: every span inside [0, tx_bytes), slot_first from 0 to n_slots without going backwards, the
//                          bytes of all spans; the host reads the verdict before any other kernel indexes with those arrays
//   al_walk_kernel         a lane per transaction: the tuples' HEADERS alone (a tuple's two headers tell where the next one starts; a key
//                          list is a whole number of 33-byte items or the row is malformed) -> the row's tuples and keys, PROVISIONAL
//   (exclusive scan)       radix_sort.hip's tiled scan over {tuples per row, keys per row} in one array
//   al_emit_kernel         a lane per transaction: the same walk again, a record per tuple at its provisional place
//   al_keys_kernel         a lane per provisional key: its tuple (a search of the tuples' first keys), its item's first byte is 0xa0 or the
//                          row gets PHANT_AL_MALFORMED (one atomic OR)
//   al_verdict_kernel      a lane per transaction: a flagged row counts nothing; the least flagged row
//   (exclusive scan)       the same scan over the final counts: tuple_first, and where every row's keys begin.  A row EMITS CONDITIONALLY:
//                          the kernels below skip the records of a flagged row, and a record's final place is its provisional one minus
//                          what the flagged rows before it had claimed
//   (txst_insert_kernel)   txstate.hip.h's address table over the witness's addresses, as it is
//   al_insert_kernel       a lane per witness slot into the SLOT TABLE -- open addressing on a keyed mix of (account row, all 32 key bytes),
//                          a slot = the witness slot's index claimed by compare-and-swap, an equal (row, key) found there lowered by
//                          atomic min -- and a lane per tuple into the table of (transaction, address), the same mechanism
//   al_tuples_kernel       a lane per tuple: account_row by txstate.hip.h's row_of, tuple_same from its table, the per-tuple outputs
//   al_key_insert_kernel   a lane per key into the table of (tuple_same, key)
//   al_key_finish_kernel   a lane per key: key_same from its table, slot_row from the slot table, the per-key outputs
// No lane loops over the keys of a tuple or over the earlier tuples of its transaction; the per-row counts are ONE atomic per distinct
// row and wave.
//
// With PHANT_AL_WALK_ONLY defined only the lane functions that walk, compare and mix are declared, without any HIP header:
// tests/native/access_main.cpp builds them as a program of its own.
#pragma once
#include <stdint.h>

#include "../../include/phant_gpu.h"

#ifdef PHANT_AL_WALK_ONLY
#ifndef PHANT_TX_DECODE_ONLY
#define PHANT_TX_DECODE_ONLY
#endif
#ifndef PHANT_TXST_RULE_ONLY
#define PHANT_TXST_RULE_ONLY
#endif
#define AL_HD inline
#else
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "access_lists.h"
#include "launch.h"
#include "staging.h"
#define AL_HD __host__ __device__ inline
#endif
#include "keyed_table.hip.h"   // the keyed mix; claim and find over the slot, tuple and key tables
#include "transactions.hip.h"  // tx::rlp_item: rlp.h's decoder over a span
#include "txstate.hip.h"       // txst::Args, txst_insert_kernel, row_of: the address table over the witness's addresses

namespace phant {
namespace al {

enum : uint32_t { NONE = PHANT_ROW_NONE, MIN_TUPLE_BYTES = 23, KEY_ITEM_BYTES = 33 };

// One tuple [address20, [key32, ...]] inside a span; positions count from the span's first byte.
struct Tuple {
    uint32_t addr;    // the address's 20 bytes
    uint32_t keys;    // the key list's payload: n_keys items of 33 bytes
    uint32_t n_keys;
    uint32_t next;    // where the tuple ends
};
// The tuple at p[pos ..) with everything up to `end` left, by its HEADERS: the rules of tx::access_list without its loop over the
// keys.  A key list whose payload is no whole number of 33-byte items cannot be one of 32-byte strings; whether every item begins
// with 0xa0 (key_ok) is left to the lanes that own the keys.  Nothing at or behind `end` is read.
AL_HD bool walk_tuple(const uint8_t* p, uint32_t pos, uint32_t end, Tuple& t) {
    uint32_t tp, te, ip, ie, kp, ke;
    bool list;
    if (!tx::rlp_item(p, pos, end, tp, te, list) || !list) return false;             // the tuple
    if (!tx::rlp_item(p, tp, te, ip, ie, list) || list || ie - ip != 20u) return false;  // the address
    if (!tx::rlp_item(p, ie, te, kp, ke, list) || !list || ke != te) return false;   // the keys, and nothing after
    if ((ke - kp) % KEY_ITEM_BYTES) return false;
    t.addr = ip, t.keys = kp, t.n_keys = (ke - kp) / KEY_ITEM_BYTES, t.next = te;
    return true;
}
// item j of the key list whose payload begins at `keys` is a string of 32 bytes (0xa0, then the key); where that key lies
AL_HD bool key_ok(const uint8_t* p, uint32_t keys, uint32_t j) { return p[keys + KEY_ITEM_BYTES * j] == 0xa0u; }
AL_HD uint32_t key_at(uint32_t keys, uint32_t j) { return keys + KEY_ITEM_BYTES * j + 1u; }
// the span p[0, len) by its tuples' headers -> how many tuples and keys it claims
AL_HD bool walk_count(const uint8_t* p, uint32_t len, uint32_t& tuples, uint32_t& keys) {
    tuples = keys = 0;
    Tuple t;
    for (uint32_t pos = 0; pos < len; pos = t.next) {
        if (!walk_tuple(p, pos, len, t)) return false;
        ++tuples, keys += t.n_keys;
    }
    return true;
}

AL_HD void load_key(const uint8_t* p, uint32_t w[8]) {
    for (int k = 0; k < 8; ++k) w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
}
AL_HD bool same_key(const uint8_t* p, const uint32_t w[8]) {
    uint32_t v[8];
    load_key(p, v);
    bool same = true;
    for (int k = 0; k < 8; ++k) same = same && v[k] == w[k];
    return same;
}
// The keyed mix of the address table carried on over four more words: keyed::home_slot again, keyed with what it made of the words
// before.  Witness keys and access-list keys are attacker-chosen bytes; without the ctx's key nobody aims them at one slot.
AL_HD uint32_t mix_on(uint32_t h, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t salt1) {
    const uint32_t w[5] = {x0, x1, x2, x3, 0u};
    return keyed::home_slot(w, h, salt1);
}
// where (row, key) is looked for first: all 32 key bytes and the row
AL_HD uint32_t slot_home(uint32_t row, const uint32_t key[8], uint32_t salt0, uint32_t salt1) {
    return mix_on(keyed::home_slot(key, salt0, salt1), key[5], key[6], key[7], row, salt1);
}
// where (transaction, address) is looked for first
AL_HD uint32_t tuple_home(uint32_t txi, const uint32_t addr[5], uint32_t salt0, uint32_t salt1) {
    return mix_on(keyed::home_slot(addr, salt0, salt1), txi, 0u, 0u, 0u, salt1);
}

#ifndef PHANT_AL_WALK_ONLY

// ctl: what the arguments' check found; the final totals; first occurrences without a row; max(n - i) over the flagged rows; the bytes
// of all spans (device form, 64 bits)
enum : uint32_t { C_BAD = 0, C_TUPLES, C_KEYS, C_MISS_ACCOUNTS, C_MISS_SLOTS, C_MALFORMED, C_BYTES_LO, C_BYTES_HI, CTL_WORDS };
enum : uint32_t { BAD_SPAN = 1, BAD_SLOT_FIRST = 2 };

// the call's device arrays
struct Args {
    phant_access_in in;   // every pointer device memory
    phant_access_out o;   // (host form: inside the arena; device form: the arena's too, copied out at the end)
    uint32_t* ctl;
    uint32_t* s1;         // 2n + 2: {tuples per row, 0, keys per row, 0} as the headers claim them, scanned in place
    uint32_t* s2;         // 2n + 2: the same without the flagged rows, scanned in place; its first n + 1 entries ARE tuple_first
    uint32_t tuple_bound, key_bound;  // the records the arena holds: no span of b bytes has more than b / 23 tuples or b / 33 keys
    // per provisional tuple: its transaction, where its address and its keys lie in the span, its first key (provisional), the least
    // provisional tuple of the same transaction with its address, its witness row
    uint32_t *t_tx, *t_addr, *t_keys, *t_kfirst, *t_same, *t_row;
    uint32_t* k_tuple;    // per provisional key: its tuple
    uint32_t *slot_table, *tuple_table, *key_table;  // mask + 1 slots each: an index or NONE
    uint32_t slot_mask, tuple_mask, key_mask, salt0, salt1;
};

__device__ inline const uint8_t* span_of(const Args& a, uint32_t txi) { return a.in.txs + a.in.al_off[txi]; }
__device__ inline bool flagged(const Args& a, uint32_t txi) { return (a.o.al_flags[txi] & PHANT_AL_MALFORMED) != 0u; }
// the provisional totals
__device__ inline uint32_t tuples_claimed(const Args& a) { return a.s1[a.in.n]; }
__device__ inline uint32_t keys_claimed(const Args& a) { return a.s1[2u * a.in.n + 1u] - a.s1[a.in.n]; }
// what the flagged rows before transaction txi had claimed: a record's final place is its provisional one minus this
__device__ inline uint32_t tuple_shift(const Args& a, uint32_t txi) { return a.s1[txi] - a.s2[txi]; }
__device__ inline uint32_t key_shift(const Args& a, uint32_t txi) {
    const uint32_t n = a.in.n;
    return (a.s1[n + 1u + txi] - a.s1[n]) - (a.s2[n + 1u + txi] - a.s2[n]);
}
// the last e in [0, cnt) with first[e] <= k (first does not go backwards, first[0] <= k, cnt >= 1)
__device__ inline uint32_t last_at_or_below(const uint32_t* first, uint32_t cnt, uint32_t k) {
    uint32_t lo = 0, hi = cnt;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}
// where key k (provisional) lies: its tuple's record and its place in the span
__device__ inline const uint8_t* key_bytes(const Args& a, uint32_t k) {
    const uint32_t e = a.k_tuple[k];
    return span_of(a, a.t_tx[e]) + key_at(a.t_keys[e], k - a.t_kfirst[e]);
}

// Of the lanes of a wave that have a record of the same transaction, the lowest adds the group's first occurrences to the row's
// count and marks the row when the group has a repeat: ONE atomic of each kind per distinct row and wave (four thousand keys of one
// transaction are not four thousand atomics on one word).  Every lane of the wave calls this.
__device__ inline void tally(const Args& a, bool has, uint32_t txi, bool first, uint32_t* warm) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(has);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t theirs = (uint32_t)__shfl((int)txi, (int)leader);
        const unsigned long long same = __ballot(has && txi == theirs);
        const unsigned long long firsts = __ballot(has && txi == theirs && first);
        if (lane == leader) {
            if (firsts) atomicAdd(warm + txi, (uint32_t)__popcll(firsts));
            if (firsts != same) atomicOr(a.o.al_flags + txi, (uint32_t)PHANT_AL_DUPLICATES);
        }
        todo &= ~same;
    }
}
// ... and the wave's first occurrences without a row, one atomic per wave
__device__ inline void tally_missing(uint32_t* counter, bool missing) {
    const unsigned long long m = __ballot(missing);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(256) al_check_args_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const phant_access_in& in = a.in;
    uint32_t f = 0;
    unsigned long long bytes = 0;
    if (i < in.n) {
        const uint64_t off = in.al_off[i];
        const uint32_t len = in.al_len[i];
        if (off > in.tx_bytes || len > in.tx_bytes - off) f |= BAD_SPAN;
        else bytes = len;
    }
    if (in.n_accounts && i <= in.n_accounts) {
        const uint32_t v = in.slot_first[i];
        if ((i == 0u && v != 0u) || (i == in.n_accounts && v != in.n_slots) || (i < in.n_accounts && in.slot_first[i + 1u] < v)) f |= BAD_SLOT_FIRST;
    }
    if (f) atomicOr(a.ctl + C_BAD, f);
    for (uint32_t d = 1; d < 64u; d <<= 1) {  // the wave's bytes in its last lane: one atomic per wave
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)bytes, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(bytes >> 32), d);
        if (lane >= d) bytes += (unsigned long long)hi << 32 | lo;
    }
    if (lane == 63u && bytes) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + C_BYTES_LO), bytes);
}

__global__ void __launch_bounds__(256) al_walk_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = a.in.n;
    if (i >= n) return;
    uint32_t tuples = 0, keys = 0;
    const bool ok = walk_count(span_of(a, i), a.in.al_len[i], tuples, keys);
    a.o.al_flags[i] = ok ? 0u : (uint32_t)PHANT_AL_MALFORMED;
    a.s1[i] = ok ? tuples : 0u;
    a.s1[n + 1u + i] = ok ? keys : 0u;
    if (i == 0u) a.s1[n] = 0u, a.s1[2u * n + 1u] = 0u;
}

__global__ void __launch_bounds__(256) al_emit_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = a.in.n;
    if (i >= n || flagged(a, i)) return;
    const uint8_t* const p = span_of(a, i);
    const uint32_t len = a.in.al_len[i];
    uint32_t e = a.s1[i], k = a.s1[n + 1u + i] - a.s1[n];
    Tuple t;
    for (uint32_t pos = 0; pos < len && e < a.tuple_bound; pos = t.next, ++e) {  // (the bound holds by arithmetic; it is not relied on)
        if (!walk_tuple(p, pos, len, t)) return;                                 // (the walk kernel has seen the same bytes succeed)
        a.t_tx[e] = i, a.t_addr[e] = t.addr, a.t_keys[e] = t.keys, a.t_kfirst[e] = k;
        k += t.n_keys;
    }
}

__global__ void __launch_bounds__(256) al_keys_kernel(Args a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= keys_claimed(a) || k >= a.key_bound) return;
    const uint32_t e = last_at_or_below(a.t_kfirst, tuples_claimed(a), k);  // (tuples without keys stand in front of the one that has k)
    a.k_tuple[k] = e;
    const uint32_t txi = a.t_tx[e];
    if (!key_ok(span_of(a, txi), a.t_keys[e], k - a.t_kfirst[e])) atomicOr(a.o.al_flags + txi, (uint32_t)PHANT_AL_MALFORMED);
}

__global__ void __launch_bounds__(256) al_verdict_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = a.in.n;
    if (i >= n) return;
    const bool bad = flagged(a, i);
    a.s2[i] = bad ? 0u : a.s1[i + 1u] - a.s1[i];
    a.s2[n + 1u + i] = bad ? 0u : a.s1[n + 2u + i] - a.s1[n + 1u + i];
    if (i == 0u) a.s2[n] = 0u, a.s2[2u * n + 1u] = 0u;
    if (bad) atomicMax(a.ctl + C_MALFORMED, n - i);
}

// slot_blocks: the workgroups of the witness's slots; the tuples' follow
__global__ void __launch_bounds__(256) al_insert_kernel(Args a, uint32_t slot_blocks) {
    const phant_access_in& in = a.in;
    if (blockIdx.x < slot_blocks) {
        const uint32_t s = blockIdx.x * 256u + threadIdx.x;
        if (s >= in.n_slots) return;
        const uint32_t row = last_at_or_below(in.slot_first, in.n_accounts, s);  // (rows without slots stand in front of the one that has s)
        const uint32_t lo = in.slot_first[row], hi = in.slot_first[row + 1u];
        uint32_t w[8];
        load_key(in.slots + 32ull * s, w);
        keyed::claim(a.slot_table, a.slot_mask, slot_home(row, w, a.salt0, a.salt1), s,
                     [&](uint32_t old) { return old >= lo && old < hi && same_key(in.slots + 32ull * old, w); });
    } else {
        const uint32_t e = (blockIdx.x - slot_blocks) * 256u + threadIdx.x;
        if (e >= tuples_claimed(a) || e >= a.tuple_bound) return;
        const uint32_t txi = a.t_tx[e];
        if (flagged(a, txi)) return;
        const uint8_t* const p = span_of(a, txi);
        uint32_t w[5];
        keyed::load_addr(p + a.t_addr[e], w);
        keyed::claim(a.tuple_table, a.tuple_mask, tuple_home(txi, w, a.salt0, a.salt1), e,
                     [&](uint32_t old) { return a.t_tx[old] == txi && keyed::same_addr(p + a.t_addr[old], w); });
    }
}

// ta: the address table (txstate.hip.h), filled by txst_insert_kernel
__global__ void __launch_bounds__(256) al_tuples_kernel(Args a, txst::Args ta) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e == 0u) {  // the totals, and the entry behind the last tuple
        const uint32_t n = a.in.n, tuples = a.s2[n], keys = a.s2[2u * n + 1u] - a.s2[n];
        a.ctl[C_TUPLES] = tuples, a.ctl[C_KEYS] = keys;
        if (tuples < a.tuple_bound + 1u) a.o.key_first[tuples] = keys;
    }
    uint32_t txi = 0, row = NONE;
    bool has = e < tuples_claimed(a) && e < a.tuple_bound, first = false;
    if (has) {
        txi = a.t_tx[e];
        has = !flagged(a, txi);
    }
    if (has) {
        const uint8_t* const p = span_of(a, txi);
        uint32_t w[5];
        keyed::load_addr(p + a.t_addr[e], w);
        const uint32_t same = keyed::find(a.tuple_table, a.tuple_mask, tuple_home(txi, w, a.salt0, a.salt1),
                                          [&](uint32_t j) { return a.t_tx[j] == txi && keyed::same_addr(p + a.t_addr[j], w); });
        row = ta.in.n_accounts ? txst::row_of(ta, ta.table, ta.mask, p + a.t_addr[e]) : (uint32_t)NONE;
        a.t_same[e] = same, a.t_row[e] = row;
        first = same == e;
        const uint32_t shift = tuple_shift(a, txi), out = e - shift;
        uint32_t* const o = reinterpret_cast<uint32_t*>(a.o.address) + 5ull * out;
        for (int q = 0; q < 5; ++q) o[q] = w[q];
        a.o.key_first[out] = a.t_kfirst[e] - key_shift(a, txi);
        a.o.account_row[out] = row;
        a.o.tuple_same[out] = same - shift;
    }
    tally(a, has, txi, first, a.o.warm_addresses);
    tally_missing(a.ctl + C_MISS_ACCOUNTS, has && first && row == NONE);
}

__global__ void __launch_bounds__(256) al_key_insert_kernel(Args a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= keys_claimed(a) || k >= a.key_bound) return;
    const uint32_t e = a.k_tuple[k];
    if (flagged(a, a.t_tx[e])) return;
    const uint32_t under = a.t_same[e];
    uint32_t w[8];
    load_key(key_bytes(a, k), w);
    keyed::claim(a.key_table, a.key_mask, slot_home(under, w, a.salt0, a.salt1), k,
                 [&](uint32_t old) { return a.t_same[a.k_tuple[old]] == under && same_key(key_bytes(a, old), w); });
}

__global__ void __launch_bounds__(256) al_key_finish_kernel(Args a) {
    const phant_access_in& in = a.in;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t txi = 0, srow = NONE, e = 0;
    bool has = k < keys_claimed(a) && k < a.key_bound, first = false;
    if (has) {
        e = a.k_tuple[k];
        txi = a.t_tx[e];
        has = !flagged(a, txi);
    }
    if (has) {
        const uint32_t under = a.t_same[e], row = a.t_row[e];
        uint32_t w[8];
        load_key(key_bytes(a, k), w);
        const uint32_t same = keyed::find(a.key_table, a.key_mask, slot_home(under, w, a.salt0, a.salt1),
                                          [&](uint32_t j) { return a.t_same[a.k_tuple[j]] == under && same_key(key_bytes(a, j), w); });
        if (row != NONE) {
            const uint32_t lo = in.slot_first[row], hi = in.slot_first[row + 1u];
            srow = keyed::find(a.slot_table, a.slot_mask, slot_home(row, w, a.salt0, a.salt1),
                               [&](uint32_t s) { return s >= lo && s < hi && same_key(in.slots + 32ull * s, w); });
        }
        first = same == k;
        const uint32_t shift = key_shift(a, txi), out = k - shift;
        uint32_t* const o = reinterpret_cast<uint32_t*>(a.o.key) + 8ull * out;
        for (int q = 0; q < 8; ++q) o[q] = w[q];
        a.o.slot_row[out] = srow;
        a.o.key_same[out] = same - shift;
    }
    tally(a, has, txi, first, a.o.warm_keys);
    tally_missing(a.ctl + C_MISS_SLOTS, has && first && srow == NONE);
}

// what the host form refuses before anything is copied -> the bytes of all spans in `total`
inline const char* check_host(const phant_access_in& in, uint64_t& total) {
    total = 0;
    for (uint32_t i = 0; i < in.n; ++i) {
        if (in.al_off[i] > in.tx_bytes || in.al_len[i] > in.tx_bytes - in.al_off[i]) return "a span leaves [0, tx_bytes)";
        total += in.al_len[i];
    }
    if (in.n_accounts) {
        if (in.slot_first[0] != 0u || in.slot_first[in.n_accounts] != in.n_slots) return "slot_first does not run from 0 to n_slots";
        for (uint32_t j = 0; j < in.n_accounts; ++j)
            if (in.slot_first[j + 1u] < in.slot_first[j]) return "slot_first goes backwards";
    }
    return nullptr;
}

}  // namespace al

int32_t block_access_lists(Workspaces& ws, hipStream_t st, const phant_access_in& in, phant_access_out& out, bool dev, const uint32_t salt[2],
                           std::string& err) {
    using namespace al;
    const char* const who = dev ? "block_access_lists_dev: " : "block_access_lists: ";
    const uint32_t n = in.n, na = in.n_accounts, ns = na ? in.n_slots : 0u;
    CALL_TRY("block_access_lists", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_AL_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_AL;
    Args a;
    std::memset(&a, 0, sizeof a);
    a.in = in, a.in.n_slots = ns;
    a.salt0 = salt[0], a.salt1 = salt[1];

    // ---- the arguments' check and the bytes of all spans: on the host, or (device form) by a kernel on the control words alone
    uint64_t total = 0;
    if (!dev) {
        if (const char* what = check_host(in, total)) return err = std::string(who) + what, PHANT_E_INVALID_ARG;
    } else {
        if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, [&](auto& io) { a.ctl = io.template take<uint32_t>(CTL_WORDS); }),
                                              "block_access_lists_dev", "workspace", err))
            return rc;
        CALL_TRY("block_access_lists", hipMemsetAsync(a.ctl, 0, 4 * CTL_WORDS, st));
        const uint64_t lanes = std::max<uint64_t>(n, na ? (uint64_t)na + 1u : 0u);
        hipLaunchKernelGGL(al_check_args_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, st, a);
        CALL_TRY("block_access_lists", hipGetLastError());
        CALL_TRY("block_access_lists", ws.read_words(Workspaces::MAILBOX_AL, a.ctl, CTL_WORDS, st));
        if (mb[C_BAD] & BAD_SPAN) return err = std::string(who) + "a span leaves [0, tx_bytes)", PHANT_E_INVALID_ARG;
        if (mb[C_BAD] & BAD_SLOT_FIRST) return err = std::string(who) + "slot_first does not run from 0 to n_slots without going backwards", PHANT_E_INVALID_ARG;
        total = (uint64_t)mb[C_BYTES_LO] | (uint64_t)mb[C_BYTES_HI] << 32;
    }
    if (total >= 1ull << 31) return err = std::string(who) + "the spans hold 2^31 bytes or more", PHANT_E_UNSUPPORTED;

    // ---- the arena: the zeroed words (control, flags and warm counts) and the outputs in front (one span goes back), (host form) the
    // inputs, then the records and the tables
    const uint32_t tb = (uint32_t)(total / MIN_TUPLE_BYTES), kb = (uint32_t)(total / KEY_ITEM_BYTES);
    const uint32_t addr_slots = keyed::table_slots(na), slot_slots = keyed::table_slots(ns), tuple_slots = keyed::table_slots(tb), key_slots = keyed::table_slots(kb);
    const size_t zero_words = (size_t)CTL_WORDS + 3 * (size_t)n, scan_n = 2 * (size_t)n + 2;
    a.tuple_bound = tb, a.key_bound = kb;
    a.slot_mask = slot_slots - 1u, a.tuple_mask = tuple_slots - 1u, a.key_mask = key_slots - 1u;
    uint32_t *zero = nullptr, *ones = nullptr, *scan = nullptr;
    uint64_t* d_off = nullptr;
    uint8_t *d_blob = nullptr, *in_begin = nullptr, *in_end = nullptr;
    auto carve = [&](auto& io) {
        zero = io.template take<uint32_t>(zero_words);
        a.s2 = io.template take<uint32_t>(scan_n);
        a.o.address = io.template take<uint8_t>(20 * (size_t)tb);
        a.o.key_first = io.template take<uint32_t>((size_t)tb + 1);
        a.o.account_row = io.template take<uint32_t>(tb);
        a.o.tuple_same = io.template take<uint32_t>(tb);
        a.o.key = io.template take<uint8_t>(32 * (size_t)kb);
        a.o.slot_row = io.template take<uint32_t>(kb);
        a.o.key_same = io.template take<uint32_t>(kb);
        in_begin = io.template take<uint8_t>(0);
        if (!dev) {
            d_off = io.template take<uint64_t>(n);
            a.in.al_len = io.template take<uint32_t>(n);
            d_blob = io.template take<uint8_t>(total);
            a.in.addresses = io.template take<uint8_t>(20 * (size_t)na);
            a.in.slot_first = io.template take<uint32_t>(na ? (size_t)na + 1 : 0);
            a.in.slots = io.template take<uint8_t>(32 * (size_t)ns);
        }
        in_end = io.template take<uint8_t>(0);
        a.s1 = io.template take<uint32_t>(scan_n);
        scan = io.template take<uint32_t>(scan_scratch_entries((uint32_t)scan_n) + 4);
        a.t_tx = io.template take<uint32_t>(tb);
        a.t_addr = io.template take<uint32_t>(tb);
        a.t_keys = io.template take<uint32_t>(tb);
        a.t_kfirst = io.template take<uint32_t>(tb);
        a.t_same = io.template take<uint32_t>(tb);
        a.t_row = io.template take<uint32_t>(tb);
        a.k_tuple = io.template take<uint32_t>(kb);
        ones = io.template take<uint32_t>((size_t)addr_slots + slot_slots + tuple_slots + key_slots);
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve, dev), dev ? "block_access_lists_dev" : "block_access_lists", "workspace", err))
        return rc;
    a.ctl = zero;
    a.o.al_flags = zero + CTL_WORDS, a.o.warm_addresses = a.o.al_flags + n, a.o.warm_keys = a.o.warm_addresses + n;
    a.o.tuple_first = a.s2;
    txst::Args ta;  // the address table of txstate.hip.h: what its insert kernel and row_of read
    std::memset(&ta, 0, sizeof ta);
    ta.in.n_accounts = na, ta.in.addresses = a.in.addresses;
    ta.table = ones, ta.mask = addr_slots - 1u, ta.salt0 = salt[0], ta.salt1 = salt[1];
    a.slot_table = ones + addr_slots, a.tuple_table = a.slot_table + slot_slots, a.key_table = a.tuple_table + tuple_slots;
    CALL_TRY("block_access_lists", hipMemsetAsync(zero, 0, 4 * zero_words, st));
    CALL_TRY("block_access_lists", hipMemsetAsync(ones, 0xff, 4 * ((size_t)addr_slots + slot_slots + tuple_slots + key_slots), st));

    // ---- in, host form: the spans' bytes back to back (nothing else of the transactions crosses the bus), where they begin, the tables
    std::vector<uint64_t> off;
    std::vector<uint8_t> blob;
    if (!dev) {
        StagedInputs ins(ws, st, in_begin, in_end);
        CALL_TRY("block_access_lists", ins.e);
        off.resize(n);
        if (!ins.staged) blob.resize(total);
        uint8_t* const pack = ins.staged ? ws.staged(d_blob) : blob.data();
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; ++i) {
            off[i] = at;
            if (in.al_len[i]) memcpy(pack + at, in.txs + in.al_off[i], in.al_len[i]);
            at += in.al_len[i];
        }
        ins.put(d_off, off.data(), 8 * (size_t)n);  // (`off` and `blob` outlive the call's last synchronisation)
        ins.put(a.in.al_len, in.al_len, 4 * (size_t)n);
        if (!ins.staged) ins.put(d_blob, blob.data(), total);
        ins.put(a.in.addresses, in.addresses, 20 * (size_t)na);
        if (na) ins.put(a.in.slot_first, in.slot_first, 4 * ((size_t)na + 1));
        ins.put(a.in.slots, in.slots, 32 * (size_t)ns);
        CALL_TRY("block_access_lists", ins.finish());
        a.in.txs = d_blob, a.in.al_off = d_off, a.in.tx_bytes = total;
        ta.in.addresses = a.in.addresses;
    }

    // ---- the walk, the verdicts, the final places
    const auto blocks = [](uint64_t lanes) { return dim3((uint32_t)((lanes + 255u) / 256u)); };
    hipLaunchKernelGGL(al_walk_kernel, blocks(n), dim3(256), 0, st, a);
    CALL_TRY("block_access_lists", hipGetLastError());
    CALL_TRY("block_access_lists", launch_exclusive_scan_u32(a.s1, (uint32_t)scan_n, scan, st));
    if (tb) {
        hipLaunchKernelGGL(al_emit_kernel, blocks(n), dim3(256), 0, st, a);
        CALL_TRY("block_access_lists", hipGetLastError());
    }
    if (kb) {
        hipLaunchKernelGGL(al_keys_kernel, blocks(kb), dim3(256), 0, st, a);
        CALL_TRY("block_access_lists", hipGetLastError());
    }
    hipLaunchKernelGGL(al_verdict_kernel, blocks(n), dim3(256), 0, st, a);
    CALL_TRY("block_access_lists", hipGetLastError());
    CALL_TRY("block_access_lists", launch_exclusive_scan_u32(a.s2, (uint32_t)scan_n, scan, st));

    // ---- the tables, the joins
    if (na && tb) {
        hipLaunchKernelGGL(txst::txst_insert_kernel, blocks(na), dim3(256), 0, st, ta);
        CALL_TRY("block_access_lists", hipGetLastError());
    }
    const uint32_t slot_blocks = kb ? blocks(ns).x : 0u;  // (without a key nobody asks the slot table)
    if (slot_blocks + blocks(tb).x) {
        hipLaunchKernelGGL(al_insert_kernel, dim3(slot_blocks + blocks(tb).x), dim3(256), 0, st, a, slot_blocks);
        CALL_TRY("block_access_lists", hipGetLastError());
    }
    hipLaunchKernelGGL(al_tuples_kernel, blocks(std::max(tb, 1u)), dim3(256), 0, st, a, ta);
    CALL_TRY("block_access_lists", hipGetLastError());
    if (kb) {
        hipLaunchKernelGGL(al_key_insert_kernel, blocks(kb), dim3(256), 0, st, a);
        CALL_TRY("block_access_lists", hipGetLastError());
        hipLaunchKernelGGL(al_key_finish_kernel, blocks(kb), dim3(256), 0, st, a);
        CALL_TRY("block_access_lists", hipGetLastError());
    }

    // ---- out: the control words and the per-transaction outputs; the host form's one span also reaches over the per-tuple and per-key
    // outputs somebody wants, up to what their rows can be at most, so that they need no copy of their own once the totals are known
    CallOutputs outs(ws, st, dev, a.ctl, a.ctl, Workspaces::MAILBOX_AL, CTL_WORDS);
    outs.add(out.al_flags, a.o.al_flags, 4 * (size_t)n);
    outs.add(out.warm_addresses, a.o.warm_addresses, 4 * (size_t)n);
    outs.add(out.warm_keys, a.o.warm_keys, 4 * (size_t)n);
    outs.add(out.tuple_first, a.o.tuple_first, 4 * ((size_t)n + 1));
    const bool want_tuples = out.address || out.key_first || out.account_row || out.tuple_same, want_keys = out.key || out.slot_row || out.key_same;
    const uint64_t tcap = std::min<uint64_t>(tb, out.tuple_cap), kcap = std::min<uint64_t>(kb, out.key_cap);
    if (!dev) {
        if (out.address) outs.cover(a.o.address + 20 * tcap);
        if (out.key_first) outs.cover(a.o.key_first + tcap + 1);
        if (out.account_row) outs.cover(a.o.account_row + tcap);
        if (out.tuple_same) outs.cover(a.o.tuple_same + tcap);
        if (out.key) outs.cover(a.o.key + 32 * kcap);
        if (out.slot_row) outs.cover(a.o.slot_row + kcap);
        if (out.key_same) outs.cover(a.o.key_same + kcap);
    }
    CALL_TRY("block_access_lists", outs.deliver());
    const uint32_t tuples = outs.ctl()[C_TUPLES], keys = outs.ctl()[C_KEYS];
    out.n_tuples = tuples, out.n_keys = keys;
    out.n_missing_accounts = outs.ctl()[C_MISS_ACCOUNTS], out.n_missing_slots = outs.ctl()[C_MISS_SLOTS];
    out.first_malformed = n - outs.ctl()[C_MALFORMED];
    // (a buffer nobody wants has no capacity to exceed)
    if ((want_tuples && tuples > out.tuple_cap) || (want_keys && keys > out.key_cap)) return PHANT_OK;
    outs.add(out.address, a.o.address, 20 * (size_t)tuples);
    outs.add(out.key_first, a.o.key_first, 4 * ((size_t)tuples + 1));
    outs.add(out.account_row, a.o.account_row, 4 * (size_t)tuples);
    outs.add(out.tuple_same, a.o.tuple_same, 4 * (size_t)tuples);
    outs.add(out.key, a.o.key, 32 * (size_t)keys);
    outs.add(out.slot_row, a.o.slot_row, 4 * (size_t)keys);
    outs.add(out.key_same, a.o.key_same, 4 * (size_t)keys);
    CALL_TRY("block_access_lists", outs.deliver());
    if (dev) CALL_TRY("block_access_lists", hipStreamSynchronize(st));
    return PHANT_OK;
}


}  // namespace phant
#else
}  // namespace al
}  // namespace phant
#endif  // PHANT_AL_WALK_ONLY
#undef AL_HD
