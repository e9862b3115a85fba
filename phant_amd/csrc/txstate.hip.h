// txstate.hip.h -- a block's transactions against the pre-state a witness proves (included by bulk_keccak.hip): the
// join of the rows phant_block_transactions[_ex] answers with the rows phant_exec_witness_prestate answers, and what
// src/blockchain/blockchain.zig:270-276 checks first (InvalidTxNonce, NotEnoughBalance, SenderIsNotEOA) as far as it can be decided for
// the whole block before any transaction runs.
//
//   txst_check_args_kernel  device form only: auth_first, code_off and code_index are what the header asks, a lane per entry; a lane that
//                           has found its own code's span sound marks a delegation designator (code_kind).  The host reads the verdict
//                           before any other kernel indexes with those arrays (the host form checks, and marks, on the host)
//   txst_insert_kernel      a lane per pre-state row: the row into the ADDRESS TABLE -- open addressing on a keyed mix of all 160 bits,
//                           a slot = the row's index, claimed by compare-and-swap; an equal address found there lowers the slot to the
//                           lower row (atomic min), so duplicates resolve to the lowest row whatever the order of arrival
//   txst_locate_kernel      a lane per transaction, per authorization tuple, per probe (each kind in workgroups of its own): the rows
//                           of sender, recipient, authority and probe by a walk of the table that compares all 20 bytes; the sort key
//                           of every transaction (its sender's row); roles, and per row the first transaction that carries a
//                           genuine tuple of it, ONE atomic per distinct row and wave
//   (radix sort)            radix_sort.hip's stable pairs sort over the keys: the rows of one sender adjacent, in block order
//   txst_scan_tiles_kernel  the SEGMENTED inclusive scan of {1, upfront cost} in 32 + 288 bits over the sorted order, a lane per row:
//                           wave level by shuffles, workgroup level through LDS; what a tile of 256 rows hands to the next
//   txst_scan_aggr_kernel   one workgroup: the same scan over the tiles' aggregates
//   txst_rules_kernel       a lane per transaction: rank and sum so far from its place in the sorted order, txst::sender_rule, the outputs,
//                           the least flagged index by one atomic; the last row of a sequence writes its row's `sends`
//   txst_small_kernel       up to 256 transactions against up to 2 048 pre-state rows (an ordinary block): all of the above in ONE workgroup,
//                           the table and the order (a bitonic sort) in LDS
// No lane runs a loop over the transactions of a sender: ten thousand transactions of one address cost what ten thousand of distinct
// addresses cost.
//
// The 288-bit arithmetic is wide_uint.h's, the address table keyed_table.hip.h's, the scan seg_scan.hip.h's (L = 9).
//
// With PHANT_TXST_RULE_ONLY defined only the per-row rule is declared, without any HIP header: tests/native/txstate_main.cpp builds it
// and wide_uint.h as a program of its own.
#pragma once
#include <stdint.h>

#include "../../include/phant_gpu.h"
#include "keyed_table.hip.h"
#include "wide_uint.h"

#ifdef PHANT_TXST_RULE_ONLY
#define TXST_HD inline
#else
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "launch.h"
#include "seg_scan.hip.h"
#include "staging.h"
#include "txstate.h"
#define TXST_HD __host__ __device__ inline
#endif

namespace phant {
namespace txst {

// ---- sums are 288-bit unsigned integers, nine little-endian limbs: the sum of 2^32 costs of at most 2^256 each fits.  The rule code's
// names for wide_uint.h at nine limbs, and for keyed_table.hip.h's address functions (tests/native/ calls them by these names)
TXST_HD void add288(uint32_t a[9], const uint32_t b[9]) { wide::add<9>(a, b); }
TXST_HD void sub288(uint32_t a[9], const uint32_t b[9]) { wide::sub<9>(a, b); }  // for a >= b
TXST_HD bool less288(const uint32_t a[9], const uint32_t b[9]) { return wide::less<9>(a, b); }
TXST_HD void load_be256(const uint8_t* row, uint32_t w[9]) { wide::load_be256<9>(row, w); }  // (w[8] = 0)
using wide::store_be256;
using keyed::home_slot;
using keyed::load_addr;
using keyed::same_addr;
// what a row adds to its sender's sequence: upfront_cost, or 2^256 for a row the transactions call marked PHANT_TX_COST_OVERFLOW
TXST_HD void cost_of(const uint8_t* row, uint32_t tx_flags, uint32_t w[9]) {
    if (tx_flags & PHANT_TX_COST_OVERFLOW) {
        for (int k = 0; k < 8; ++k) w[k] = 0u;
        w[8] = 1u;
    } else {
        load_be256(row, w);
    }
}
TXST_HD bool participates(uint8_t sig_status, uint32_t tx_flags) {
    return sig_status == PHANT_SIG_OK && !(tx_flags & (PHANT_TX_UNDECODABLE | PHANT_TX_BAD_V | PHANT_TX_SIGNATURE));
}
TXST_HD bool proven(uint8_t account_status) { return account_status == PHANT_PROOF_PRESENT || account_status == PHANT_PROOF_ABSENT; }
// EIP-7702: 0xef0100 || address (only a code of 23 bytes is looked into)
TXST_HD bool is_designator_code(const uint8_t* code, uint64_t len) { return len == 23u && code[0] == 0xefu && code[1] == 0x01u && code[2] == 0x00u; }
// keccak256 of the empty string
TXST_HD bool is_empty_code_hash(const uint8_t* h) {
    const uint64_t want[4] = {0xc5d2460186f7233cull, 0x927e7db2dcc703c0ull, 0xe500b653ca82273bull, 0x7bfad8045d85a470ull};
    for (int q = 0; q < 4; ++q) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v = v << 8 | h[8 * q + k];
        if (v != want[q]) return false;
    }
    return true;
}

// One row of a sequence: everything the sender rules of include/phant_gpu.h read.
struct RowIn {
    uint32_t fork, i, rank;      // i: the transaction's index in the block; rank: the rows of its sequence before it
    uint64_t nonce, acc_nonce;   // the transaction's; the pre-state's
    uint32_t own[9], incl[9];    // cost_of the row; the sum over the sequence up to AND including the row
    uint32_t balance[9];
    bool code_empty, code_none, code_designator;  // codeHash is the empty one; code_index is PHANT_CODE_NONE; else: the code is a designator
    bool authorized;             // an earlier participating transaction carries a genuine tuple of this sender
};
struct RowOut {
    uint32_t flags;
    uint64_t expected_nonce;
    uint32_t spent[8];
};
TXST_HD void sender_rule(const RowIn& r, RowOut& o) {
    o.flags = 0u;
    o.expected_nonce = r.acc_nonce + r.rank;
    if (o.expected_nonce < r.acc_nonce) o.expected_nonce = ~0ull;
    uint32_t before[9];
    for (int k = 0; k < 9; ++k) before[k] = r.incl[k];
    sub288(before, r.own);
    if (before[8]) o.flags |= PHANT_TXST_SPENT_SATURATED;
    for (int k = 0; k < 8; ++k) o.spent[k] = before[8] ? 0xffffffffu : before[k];
    if (r.fork >= PHANT_TXS_FORK_PRAGUE && ((!r.code_empty && !r.code_none && r.code_designator) || r.authorized)) {
        o.flags |= PHANT_TXST_UNDETERMINED;  // delegated code may CREATE, a tuple may bump the nonce: the caller's
        return;
    }
    if (r.nonce < o.expected_nonce) o.flags |= PHANT_TXST_NONCE_LOW;
    if (r.nonce > o.expected_nonce) o.flags |= PHANT_TXST_NONCE_HIGH;
    if (!r.code_empty) o.flags |= (r.fork >= PHANT_TXS_FORK_PRAGUE && r.code_none) ? PHANT_TXST_CODE_MISSING : PHANT_TXST_NOT_EOA;
    if (less288(r.balance, r.incl)) o.flags |= PHANT_TXST_NEEDS_INFLOW | (r.i == 0u ? PHANT_TXST_BALANCE_SHORT : 0u);
}

#ifndef PHANT_TXST_RULE_ONLY

enum : uint32_t { CTL_WORDS = 4 };  // ctl[0]: what the arguments' check found, [1]: max(n - i) over the flagged rows, [2]: undetermined rows
enum : uint32_t { BAD_AUTH_FIRST = 1, BAD_CODE_OFF = 2, BAD_CODE_INDEX = 4 };
enum : uint32_t { NONE = PHANT_ROW_NONE, SEG_WORDS = seg::SEG_WORDS, TILE = seg::TILE };
using Seg = seg::Seg<9>;  // {sum of costs, rows, "a sequence starts at or before me in what was combined"}

// the call's device arrays
struct Args {
    phant_txstate_in in;    // every pointer device memory
    phant_txstate_out o;
    uint8_t* code_kind;     // n_codes: 1 = a delegation designator
    uint32_t* ctl;
    uint32_t* table;        // mask + 1 slots: a row's index or NONE
    uint32_t mask, salt0, salt1;
    uint32_t* first_auth;   // n_accounts: the least participating transaction with a genuine tuple of this row, or NONE
    uint64_t* keys;         // n: the sender's row (n_accounts: none) -- the sort's input
    uint32_t* vals;         // n: i
    uint32_t* inv;          // n: where row i stands in the sorted order
    uint32_t* loc;          // n x SEG_WORDS: the scan inside a tile
    uint32_t* agg;          // tiles x SEG_WORDS: a tile's last
    uint32_t* tp;           // tiles x SEG_WORDS: what runs into a tile
};

__global__ void __launch_bounds__(256) txst_check_args_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const phant_txstate_in& in = a.in;
    uint32_t f = 0;
    if (in.auth_first && i <= in.n) {
        const uint32_t v = in.auth_first[i];
        if (v > in.n_auth || (i < in.n && in.auth_first[i + 1u] < v)) f |= BAD_AUTH_FIRST;
    }
    if (i < in.n_codes) {
        const uint64_t b = in.code_off[i], e = in.code_off[i + 1u];
        if (b > e || e > in.code_bytes) f |= BAD_CODE_OFF;
        else a.code_kind[i] = is_designator_code(in.codes + b, e - b) ? 1u : 0u;  // (this span is sound: its first three bytes exist)
    }
    if (i < in.n_accounts) {
        const uint32_t ci = in.code_index[i];
        if (ci != PHANT_CODE_NONE && ci >= in.n_codes) f |= BAD_CODE_INDEX;
    }
    if (f) atomicOr(a.ctl, f);
}

// row j into the address table (global memory, or the small path's in LDS): duplicates resolve to the lowest row
__device__ inline void insert_row(const Args& a, uint32_t* table, uint32_t mask, uint32_t j) {
    uint32_t w[5];
    load_addr(a.in.addresses + 20ull * j, w);
    keyed::claim(table, mask, home_slot(w, a.salt0, a.salt1), j, [&](uint32_t old) { return same_addr(a.in.addresses + 20ull * old, w); });
}
__global__ void __launch_bounds__(256) txst_insert_kernel(Args a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < a.in.n_accounts) insert_row(a, a.table, a.mask, j);
}

__device__ inline uint32_t row_of(const Args& a, const uint32_t* table, uint32_t mask, const uint8_t* addr) {
    uint32_t w[5];
    load_addr(addr, w);
    return keyed::find(table, mask, home_slot(w, a.salt0, a.salt1), [&](uint32_t j) { return same_addr(a.in.addresses + 20ull * j, w); });
}
__device__ inline void add_role(const Args& a, uint32_t row, uint32_t role) {
    atomicOr(reinterpret_cast<uint32_t*>(a.o.roles) + (row >> 2), role << (8u * (row & 3u)));
}

// transaction i: its rows into the outputs -> its sender's row, its flags so far (SKIPPED, SENDER_UNKNOWN, TO_UNKNOWN), its recipient's row
__device__ inline void locate_tx(const Args& a, const uint32_t* table, uint32_t mask, uint32_t i, uint32_t& s, uint32_t& f, uint32_t& to_row) {
    const phant_txstate_in& in = a.in;
    const uint32_t tf = in.tx_flags[i];
    s = NONE, to_row = NONE, f = PHANT_TXST_SKIPPED;
    if (participates(in.sig_status[i], tf)) {
        f = 0u;
        s = row_of(a, table, mask, in.sender + 20ull * i);
        if (s == NONE || !proven(in.account_status[s])) f |= PHANT_TXST_SENDER_UNKNOWN;
        if (!(tf & PHANT_TX_IS_CREATE)) {
            to_row = row_of(a, table, mask, in.to + 20ull * i);
            if (to_row == NONE || !proven(in.account_status[to_row])) f |= PHANT_TXST_TO_UNKNOWN;
        }
    }
    a.o.sender_row[i] = s;
    a.o.to_row[i] = to_row;
}
// tuple k (the call has auth_first and a transaction): a genuine tuple of a participating transaction -> its authority's row, that transaction
__device__ inline uint32_t locate_auth(const Args& a, const uint32_t* table, uint32_t mask, uint32_t k, uint32_t& first_tx) {
    const phant_txstate_in& in = a.in;
    if (k >= in.n_auth || k >= in.auth_first[in.n] || k < in.auth_first[0] || in.auth_status[k] != PHANT_SIG_OK) return NONE;
    uint32_t lo = 0, hi = in.n;  // the transaction j with auth_first[j] <= k < auth_first[j + 1]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (in.auth_first[mid] <= k) lo = mid;
        else hi = mid;
    }
    if (!participates(in.sig_status[lo], in.tx_flags[lo])) return NONE;
    first_tx = lo;
    return row_of(a, table, mask, in.authority + 20ull * k);
}
// a role for `row` (NONE: nothing to say), ONE atomic per distinct row and wave; every lane of the wave calls this.  (The lanes of a
// call hold one kind: the role is the group's; the lowest tuple of a group is the earliest.)
__device__ inline void publish(const Args& a, uint32_t* first_auth, uint32_t row, uint32_t role, uint32_t first_tx) {
    if (keyed::wave_first_of(row != NONE, row)) {
        add_role(a, row, role);
        if (first_tx != NONE) atomicMin(first_auth + row, first_tx);
    }
}

// tx_blocks, auth_blocks: the workgroups of the transactions and of the tuples; the probes' follow
__global__ void __launch_bounds__(256) txst_locate_kernel(Args a, uint32_t tx_blocks, uint32_t auth_blocks) {
    const phant_txstate_in& in = a.in;
    uint32_t row = NONE, role = 0, first_tx = NONE;
    if (blockIdx.x < tx_blocks) {
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        if (i < in.n) {
            uint32_t s, f;
            locate_tx(a, a.table, a.mask, i, s, f, row);
            a.o.state_flags[i] = f;
            a.keys[i] = s == NONE ? in.n_accounts : s;
            a.vals[i] = i;
        }
        role = PHANT_ROLE_RECIPIENT;
    } else if (blockIdx.x < tx_blocks + auth_blocks) {
        row = locate_auth(a, a.table, a.mask, (blockIdx.x - tx_blocks) * 256u + threadIdx.x, first_tx);
        role = PHANT_ROLE_AUTHORITY;
    } else {
        const uint32_t q = (blockIdx.x - tx_blocks - auth_blocks) * 256u + threadIdx.x;
        if (q < in.n_probe) a.o.probe_row[q] = row = row_of(a, a.table, a.mask, in.probe + 20ull * q);
        role = PHANT_ROLE_PROBE;
    }
    publish(a, a.first_auth, row, role, first_tx);
}

__global__ void __launch_bounds__(256) txst_scan_tiles_kernel(Args a, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
    __shared__ Seg s_wave[4];
    const uint32_t tid = threadIdx.x, p = blockIdx.x * TILE + tid;
    const bool valid = p < a.in.n;
    Seg s;
    seg::zero(s);
    uint32_t i = 0;
    if (valid) {
        i = vals[p];
        cost_of(a.in.upfront_cost + 32ull * i, a.in.tx_flags[i], s.w);
        s.cnt = 1u;
        s.f = (p == 0u || keys[p - 1u] != keys[p]) ? 1u : 0u;
    }
    seg::scan_block(s, tid, s_wave);
    if (valid) {
        seg::store(a.loc + (size_t)SEG_WORDS * p, s);
        a.inv[i] = p;
    }
    if (tid == TILE - 1u) seg::store(a.agg + (size_t)SEG_WORDS * blockIdx.x, s);  // (the last tile's is never read)
}

// tp[t] = what runs into tile t: the tiles before it combined (one workgroup)
__global__ void __launch_bounds__(256) txst_scan_aggr_kernel(Args a, uint32_t tiles) {
    __shared__ Seg s_wave[4];
    __shared__ Seg s_carry;
    seg::aggregate(a.agg, a.tp, 0u, tiles, threadIdx.x, s_wave, &s_carry);
}

// Row i, whose sender's row is s (NONE: the witness lacks it, or the row was skipped) and whose flags so far are f: `here` = the scan up to and
// including it, `last` = its sequence ends with it.  The sender rules, the outputs, the call's two counts.
__device__ inline void finish_row(const Args& a, uint32_t i, uint32_t s, uint32_t f, const Seg& here, bool last, const uint32_t* first_auth) {
    const phant_txstate_in& in = a.in;
    uint64_t expected = 0;
    uint32_t spent[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s != NONE) {  // (a sender the witness has: a sequence was scanned for it, proven or not)
        if (last) add_role(a, s, PHANT_ROLE_SENDER);
        if (!(f & PHANT_TXST_SENDER_UNKNOWN)) {
            if (last) a.o.sends[s] = here.cnt;
            RowIn r;
            r.fork = in.fork, r.i = i, r.rank = here.cnt - 1u;
            r.nonce = in.nonce[i], r.acc_nonce = in.nonces[s];
            cost_of(in.upfront_cost + 32ull * i, in.tx_flags[i], r.own);
#pragma unroll
            for (int k = 0; k < 9; ++k) r.incl[k] = here.w[k];
            load_be256(in.balances + 32ull * s, r.balance);
            const uint32_t ci = in.code_index[s];
            r.code_empty = is_empty_code_hash(in.code_hashes + 32ull * s);
            r.code_none = ci == PHANT_CODE_NONE;
            r.code_designator = !r.code_none && a.code_kind[ci] != 0u;
            r.authorized = first_auth[s] < i;
            RowOut o;
            sender_rule(r, o);
            f |= o.flags, expected = o.expected_nonce;
#pragma unroll
            for (int k = 0; k < 8; ++k) spent[k] = o.spent[k];
        }
    }
    a.o.state_flags[i] = f;
    a.o.expected_nonce[i] = expected;
    store_be256(a.o.spent_before + 32ull * i, spent);
    if (f & PHANT_TXST_ERROR_BITS) atomicMax(a.ctl + 1, in.n - i);
    if (f & PHANT_TXST_UNDETERMINED) atomicAdd(a.ctl + 2, 1u);
}

__global__ void __launch_bounds__(64) txst_rules_kernel(Args a, const uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= a.in.n) return;
    const uint32_t s = a.o.sender_row[i];
    Seg here;
    seg::zero(here);
    bool last = false;
    if (s != NONE) {
        const uint32_t p = a.inv[i];
        seg::scan_at(a.loc, a.tp, p, here);
        last = p + 1u == a.in.n || keys[p + 1u] != s;
    }
    finish_row(a, i, s, a.o.state_flags[i], here, last, a.first_auth);  // (the locate kernel's flags: SKIPPED, SENDER_UNKNOWN, TO_UNKNOWN)
}

// ---- the small path: a block of up to SMALL_ROWS transactions against up to SMALL_ACCOUNTS pre-state rows in ONE workgroup -- the table,
// the first-tuple words and the order live in LDS, and the lane that holds a row's place in the sorted order finishes that row.  The
// order is a bitonic sort of {sender's row, i} in 64 bits: the keys are distinct, so it is the stable order.
enum : uint32_t { SMALL_ROWS = 256, SMALL_ACCOUNTS = 2048, SMALL_SLOTS = 4096 };
__global__ void __launch_bounds__(256) txst_small_kernel(Args a, uint32_t n_auth) {
    __shared__ uint32_t s_table[SMALL_SLOTS];
    __shared__ uint32_t s_first_auth[SMALL_ACCOUNTS];
    __shared__ unsigned long long s_key[SMALL_ROWS];
    __shared__ uint32_t s_flags[SMALL_ROWS];
    __shared__ Seg s_wave[4];
    const phant_txstate_in& in = a.in;
    const uint32_t tid = threadIdx.x, mask = SMALL_SLOTS - 1u;
    for (uint32_t k = tid; k < SMALL_SLOTS; k += 256u) s_table[k] = NONE;
    for (uint32_t k = tid; k < SMALL_ACCOUNTS; k += 256u) s_first_auth[k] = NONE;
    __syncthreads();
    for (uint32_t j = tid; j < in.n_accounts; j += 256u) insert_row(a, s_table, mask, j);
    __syncthreads();
    {
        uint32_t s = NONE, f = 0, to_row = NONE;
        unsigned long long key = ~0ull;  // (no row: behind every row)
        if (tid < in.n) {
            locate_tx(a, s_table, mask, tid, s, f, to_row);
            key = (unsigned long long)(s == NONE ? in.n_accounts : s) << 32 | tid;
        }
        s_key[tid] = key, s_flags[tid] = f;
        publish(a, s_first_auth, to_row, PHANT_ROLE_RECIPIENT, NONE);
    }
    for (uint32_t k0 = 0; k0 < n_auth; k0 += 256u) {  // (every lane takes every turn: publish is the whole wave's)
        uint32_t first_tx = NONE;
        const uint32_t row = locate_auth(a, s_table, mask, k0 + tid, first_tx);
        publish(a, s_first_auth, row, PHANT_ROLE_AUTHORITY, first_tx);
    }
    for (uint32_t q0 = 0; q0 < in.n_probe; q0 += 256u) {
        const uint32_t q = q0 + tid;
        uint32_t row = NONE;
        if (q < in.n_probe) a.o.probe_row[q] = row = row_of(a, s_table, mask, in.probe + 20ull * q);
        publish(a, s_first_auth, row, PHANT_ROLE_PROBE, NONE);
    }
    __syncthreads();
    for (uint32_t k = 2; k <= SMALL_ROWS; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            const uint32_t other = tid ^ j;
            if (other > tid) {
                const unsigned long long x = s_key[tid], y = s_key[other];
                if ((x > y) == ((tid & k) == 0u)) s_key[tid] = y, s_key[other] = x;
            }
            __syncthreads();
        }
    const unsigned long long key = s_key[tid];
    const bool valid = tid < in.n;  // (the sorted order holds the n rows in front)
    const uint32_t i = (uint32_t)key, srow = (uint32_t)(key >> 32);
    Seg s;
    seg::zero(s);
    s.f = 1u;
    if (valid) {
        cost_of(in.upfront_cost + 32ull * i, in.tx_flags[i], s.w);
        s.cnt = 1u;
        s.f = (tid == 0u || (uint32_t)(s_key[tid - 1u] >> 32) != srow) ? 1u : 0u;
    }
    seg::scan_block(s, tid, s_wave);
    if (valid) {
        const bool last = tid + 1u == in.n || (uint32_t)(s_key[tid + 1u] >> 32) != srow;
        finish_row(a, i, srow == in.n_accounts ? (uint32_t)NONE : srow, s_flags[i], s, last, s_first_auth);
    }
}

// the arrays that cross the bus in the host form: (member, type, elements)
#define TXST_INPUTS(X)                                                                                                                     \
    X(sender, uint8_t, 20 * (size_t)n) X(sig_status, uint8_t, n) X(tx_flags, uint32_t, n) X(nonce, uint64_t, n) X(upfront_cost, uint8_t, 32 * (size_t)n) \
    X(to, uint8_t, 20 * (size_t)n) X(auth_first, uint32_t, (in.auth_first ? (size_t)n + 1 : 0)) X(authority, uint8_t, 20 * (size_t)n_auth)                \
    X(auth_status, uint8_t, n_auth) X(addresses, uint8_t, 20 * (size_t)na) X(account_status, uint8_t, na) X(nonces, uint64_t, na)                         \
    X(balances, uint8_t, 32 * (size_t)na) X(code_hashes, uint8_t, 32 * (size_t)na) X(code_index, uint32_t, na) X(probe, uint8_t, 20 * (size_t)np)
// the outputs behind the zeroed words (which hold sends and roles)
#define TXST_OUTPUTS(X)                                                                                                                      \
    X(sender_row, uint32_t, n) X(to_row, uint32_t, n) X(expected_nonce, uint64_t, n) X(spent_before, uint8_t, 32 * (size_t)n) X(state_flags, uint32_t, n) \
    X(probe_row, uint32_t, np)

// what the host form refuses before anything is copied; kind: a byte per code, 1 = a delegation designator
inline const char* check_host(const phant_txstate_in& in, std::vector<uint8_t>& kind) {
    if (in.auth_first)
        for (uint32_t i = 0; i <= in.n; ++i)
            if (in.auth_first[i] > in.n_auth || (i < in.n && in.auth_first[i + 1u] < in.auth_first[i]))
                return "auth_first does not run within [0, n_auth] without going backwards";
    kind.assign(in.n_codes, 0);
    for (uint32_t k = 0; k < in.n_codes; ++k) {
        const uint64_t b = in.code_off[k], e = in.code_off[k + 1u];
        if (b > e || e > in.code_bytes) return "code_off does not run within [0, code_bytes] without going backwards";
        kind[k] = is_designator_code(in.codes + b, e - b) ? 1 : 0;
    }
    for (uint32_t j = 0; j < in.n_accounts; ++j)
        if (in.code_index[j] != PHANT_CODE_NONE && in.code_index[j] >= in.n_codes) return "a code_index names no code";
    return nullptr;
}

}  // namespace txst

int32_t block_txs_prestate(Workspaces& ws, hipStream_t st, const phant_txstate_in& in, phant_txstate_out& out, bool dev, const uint32_t salt[2],
                           std::string& err) {
    using namespace txst;
    const uint32_t n = in.n, na = in.n_accounts, nc = in.n_codes, np = in.n_probe;
    const uint32_t n_auth = in.auth_first && n ? in.n_auth : 0u;  // (without auth_first, or without a transaction, a tuple belongs to none)
    CALL_TRY("block_txs_prestate", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_TXST_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_TXST;
    std::vector<uint8_t> kind;
    if (!dev)
        if (const char* what = check_host(in, kind)) return err = std::string("block_txs_prestate: ") + what, PHANT_E_INVALID_ARG;

    // ---- the arena: the zeroed words (control, the sort's digit totals, sends, roles) and the outputs in front (one span goes back), (host
    // form) the inputs, then the table and what the sort and the scan need
    const uint32_t slots = keyed::table_slots(na);  // (n_accounts < 2^31 is checked by the caller)
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TILE - 1u) / TILE);
    const size_t zero_words = (size_t)CTL_WORDS + 512 + na + ((size_t)na + 3) / 4;
    Args a;
    std::memset(&a, 0, sizeof a);
    a.in = in;
    a.mask = slots - 1u, a.salt0 = salt[0], a.salt1 = salt[1];
    uint32_t *zero = nullptr, *ones = nullptr, *digit_totals = nullptr, *hist = nullptr, *vals_alt = nullptr;
    uint64_t* keys_alt = nullptr;
    uint8_t* in_end = nullptr;
    auto carve = [&](auto& io) {
        zero = io.template take<uint32_t>(zero_words);
#define X(m, T, e) a.o.m = io.template take<T>(e);
        TXST_OUTPUTS(X)
#undef X
        if (!dev) {
#define X(m, T, e) a.in.m = io.template take<T>(e);
            TXST_INPUTS(X)
#undef X
        }
        a.code_kind = io.template take<uint8_t>(nc);
        in_end = io.template take<uint8_t>(0);
        ones = io.template take<uint32_t>((size_t)slots + na);
        a.keys = io.template take<uint64_t>(n);
        keys_alt = io.template take<uint64_t>(n);
        a.vals = io.template take<uint32_t>(n);
        vals_alt = io.template take<uint32_t>(n);
        hist = io.template take<uint32_t>(sort_hist_entries(n));
        a.inv = io.template take<uint32_t>(n);
        a.loc = io.template take<uint32_t>((size_t)SEG_WORDS * n);
        a.agg = io.template take<uint32_t>((size_t)SEG_WORDS * tiles);
        a.tp = io.template take<uint32_t>((size_t)SEG_WORDS * (tiles ? tiles : 1u));
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_txs_prestate", "workspace", err)) return rc;
    if (!in.auth_first) a.in.auth_first = nullptr;
    a.ctl = zero, digit_totals = zero + CTL_WORDS;
    a.o.sends = digit_totals + 512;
    a.o.roles = reinterpret_cast<uint8_t*>(a.o.sends + na);
    a.table = ones, a.first_auth = ones + slots;
    CALL_TRY("block_txs_prestate", hipMemsetAsync(zero, 0, 4 * zero_words, st));
    const bool small = n != 0u && n <= SMALL_ROWS && na <= SMALL_ACCOUNTS;  // (its table and first-tuple words are in LDS)
    if (!small) CALL_TRY("block_txs_prestate", hipMemsetAsync(ones, 0xff, 4 * ((size_t)slots + na), st));

    // ---- in: (host form) every array and the codes' kinds in ONE copy through the pinned stage where they fit it; (device form) the check
    if (!dev) {
        StagedInputs ins(ws, st, a.in.sender, in_end);
#define X(m, T, e) ins.put(a.in.m, in.m, (size_t)(e) * sizeof(T));
        TXST_INPUTS(X)
#undef X
        ins.put(a.code_kind, kind.data(), nc);  // (`kind` outlives the call's last synchronisation)
        CALL_TRY("block_txs_prestate", ins.finish());
        a.in.code_off = nullptr, a.in.codes = nullptr;  // (no kernel of the host form reads them: the kinds are there)
    } else {
        const uint64_t lanes = std::max<uint64_t>(std::max<uint64_t>((uint64_t)n + 1u, nc), na);
        hipLaunchKernelGGL(txst_check_args_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, st, a);
        CALL_TRY("block_txs_prestate", hipGetLastError());
        CALL_TRY("block_txs_prestate", ws.read_words(Workspaces::MAILBOX_TXST, a.ctl, CTL_WORDS, st));
        if (mb[0] & BAD_AUTH_FIRST) return err = "block_txs_prestate_dev: auth_first does not run within [0, n_auth] without going backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & BAD_CODE_OFF) return err = "block_txs_prestate_dev: code_off does not run within [0, code_bytes] without going backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & BAD_CODE_INDEX) return err = "block_txs_prestate_dev: a code_index names no code", PHANT_E_INVALID_ARG;
    }

    // ---- the join, the order, the scan, the rules
    const uint32_t tx_blocks = tiles, auth_blocks = (n_auth + 255u) / 256u, probe_blocks = (np + 255u) / 256u;
    if (small) {
        hipLaunchKernelGGL(txst_small_kernel, dim3(1), dim3(256), 0, st, a, n_auth);
        CALL_TRY("block_txs_prestate", hipGetLastError());
    } else if (na) {
        hipLaunchKernelGGL(txst_insert_kernel, dim3((na + 255u) / 256u), dim3(256), 0, st, a);
        CALL_TRY("block_txs_prestate", hipGetLastError());
    }
    if (!small && tx_blocks + auth_blocks + probe_blocks) {
        hipLaunchKernelGGL(txst_locate_kernel, dim3(tx_blocks + auth_blocks + probe_blocks), dim3(256), 0, st, a, tx_blocks, auth_blocks);
        CALL_TRY("block_txs_prestate", hipGetLastError());
    }
    if (n && !small) {
        uint64_t* keys = nullptr;
        uint32_t* vals = nullptr;
        CALL_TRY("block_txs_prestate", launch_sort_pairs(a.keys, a.vals, keys_alt, vals_alt, n, sort_key_bits(na), hist, digit_totals, &keys, &vals, st));
        hipLaunchKernelGGL(txst_scan_tiles_kernel, dim3(tiles), dim3(256), 0, st, a, (const uint64_t*)keys, (const uint32_t*)vals);
        CALL_TRY("block_txs_prestate", hipGetLastError());
        hipLaunchKernelGGL(txst_scan_aggr_kernel, dim3(1), dim3(256), 0, st, a, tiles);
        CALL_TRY("block_txs_prestate", hipGetLastError());
        hipLaunchKernelGGL(txst_rules_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, a, (const uint64_t*)keys);
        CALL_TRY("block_txs_prestate", hipGetLastError());
    }

    // ---- out: the control words and everything up to the last wanted output (one span in the host form while it fits the pinned stage)
    CallOutputs outs(ws, st, dev, a.ctl, a.ctl, Workspaces::MAILBOX_TXST, CTL_WORDS);
    outs.add(out.sends, a.o.sends, 4 * (size_t)na);
    outs.add(out.roles, a.o.roles, na);
#define X(m, T, e) outs.add(out.m, a.o.m, (size_t)(e) * sizeof(T));
    TXST_OUTPUTS(X)
#undef X
    CALL_TRY("block_txs_prestate", outs.deliver());
    out.first_bad = n - outs.ctl()[1], out.n_undetermined = outs.ctl()[2];
    return PHANT_OK;
}

#undef TXST_INPUTS
#undef TXST_OUTPUTS

}  // namespace phant
#else
}  // namespace txst
}  // namespace phant
#endif  // PHANT_TXST_RULE_ONLY
#undef TXST_HD
