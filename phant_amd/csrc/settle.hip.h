// settle.hip.h -- a block of plain transfers settled on the device (included by bulk_keccak.hip behind txstate.hip.h; DESIGN.md section
// 7n): what src/blockchain/blockchain.zig:155-205 `applyBody` and :262-343 `processTransaction` do for the transactions that meet no
// code -- gas, the exact balance checks, the coinbase's and the withdrawals' credits, the account writes -- as ONE sort and ONE scan.
// Every plain transaction is up to three signed balance EVENTS (its sender's debit, its recipient's and the coinbase's credit), every
// withdrawal one; events are numbered in time order (3 i, 3 i + 1, 3 i + 2, then 3 n + j), so the STABLE sort of the event numbers by
// account row alone is the (row, time) order, and a running balance is the segmented inclusive scan of the signed values over it.
//
//   settle_check_kernel    device form only: sender_row, to_row and wd_row are < n_accounts or PHANT_ROW_NONE, a lane per entry.  The host
//                          reads the verdict before any other kernel indexes with them (the host form checks on the host)
//   settle_classify_kernel a lane per transaction and per withdrawal: the row's class and gas_used (settle::classify), the sort key of each
//                          of its events (its account row; n_accounts for an event that does not exist), the touched marks -- ONE atomic
//                          per distinct row and wave, so that n credits to one coinbase do not queue on one word --, the counts
//   (radix sort)           radix_sort.hip's stable pairs sort: key = account row, value = event number
//   settle_scan_tiles_kernel  tiles of 256: the SEGMENTED inclusive scan of {signed value in 320 bits, sender events} over the sorted
//                          events (values are recomputed from the event number, never stored), and in workgroups of their own the plain
//                          prefix sum of gas_used in block order through the same code (no segment ever starts)
//   settle_scan_aggr_kernel   two workgroups: the same scan over the tiles' aggregates, events and gas
//   settle_finish_kernel   a lane per sorted event and per pre-state row: the lane at a transaction's sender slot writes that row's
//                          outputs (an excluded slot: the zeros of a row that is not plain) and lowers first_bad; the lane at a segment's
//                          last event writes that row's account outputs; the lanes beyond the events write the untouched rows
// No lane runs a loop over the events of an account: ten thousand credits to one coinbase cost what ten thousand to distinct rows cost.
//
// The 320-bit arithmetic is wide_uint.h's, the scan seg_scan.hip.h's (L = 10), the wave's vote on a row keyed_table.hip.h's.
//
// With PHANT_SETTLE_RULE_ONLY (and PHANT_TXST_RULE_ONLY) defined only the per-row functions are declared, without any HIP header:
// tests/native/settle_main.cpp builds them and wide_uint.h as a program of its own.
#pragma once
#include <stdint.h>

#include "../../include/phant_gpu.h"
#include "keyed_table.hip.h"
#include "txstate.hip.h"  // txst::is_empty_code_hash, proven; the PHANT_TXST_* flag rules
#include "wide_uint.h"

#ifdef PHANT_SETTLE_RULE_ONLY
#define SETTLE_HD inline
#else
#include <algorithm>
#include <cstring>
#include <string>

#include "launch.h"
#include "seg_scan.hip.h"
#include "settle.h"
#include "staging.h"
#define SETTLE_HD __host__ __device__ inline
#endif

namespace phant {
namespace settle {

// ---- 320-bit two's-complement integers, ten little-endian limbs (wide_uint.h): 2^32 events of magnitude below 2^256 and a balance sum
// exactly
enum : uint32_t { LIMBS = 10 };
SETTLE_HD void add320(uint32_t a[LIMBS], const uint32_t b[LIMBS]) { wide::add<LIMBS>(a, b); }
SETTLE_HD void sub320(uint32_t a[LIMBS], const uint32_t b[LIMBS]) { wide::sub<LIMBS>(a, b); }
SETTLE_HD void neg320(uint32_t a[LIMBS]) { wide::neg<LIMBS>(a); }
SETTLE_HD bool negative(const uint32_t a[LIMBS]) { return (a[LIMBS - 1] >> 31) != 0u; }
// 32 bytes big-endian -> ten limbs
SETTLE_HD void load256(const uint8_t* row, uint32_t w[LIMBS]) { wide::load_be256<LIMBS>(row, w); }
// g x p, p < 2^256
SETTLE_HD void mul_u64_u256(uint64_t g, const uint32_t p[8], uint32_t out[LIMBS]) {
    const uint32_t g0 = (uint32_t)g, g1 = (uint32_t)(g >> 32);
    uint64_t c = 0;
    for (int k = 0; k < 8; ++k) {
        c += (uint64_t)g0 * p[k];
        out[k] = (uint32_t)c, c >>= 32;
    }
    out[8] = (uint32_t)c, out[9] = 0u;
    c = 0;
    for (int k = 0; k < 8; ++k) {
        c += (uint64_t)g1 * p[k] + out[k + 1];
        out[k + 1] = (uint32_t)c, c >>= 32;
    }
    out[9] = (uint32_t)c;
}
// a, clamped to [0, 2^256 - 1] -> PHANT_SETTLE_ACCT_NEGATIVE / _OVERFLOW when it was
SETTLE_HD uint32_t clamp256(const uint32_t a[LIMBS], uint32_t out[8]) {
    const bool neg = negative(a), over = !neg && (a[8] | a[9]) != 0u;
    for (int k = 0; k < 8; ++k) out[k] = neg ? 0u : over ? 0xffffffffu : a[k];
    return neg ? PHANT_SETTLE_ACCT_NEGATIVE : over ? PHANT_SETTLE_ACCT_OVERFLOW : 0u;
}
// a < c, for 0 <= c < 2^256 (its limbs 8 and 9 are zero)
SETTLE_HD bool below(const uint32_t a[LIMBS], const uint32_t c[LIMBS]) { return negative(a) || wide::less<LIMBS>(a, c); }
SETTLE_HD bool less_be256(const uint8_t* a, const uint8_t* b) {
    uint32_t x[LIMBS], y[LIMBS];
    load256(a, x);
    load256(b, y);
    return below(x, y);
}
SETTLE_HD bool is_precompile(uint32_t fork, const uint8_t* to) {
    uint32_t high = 0u;  // (no early return: nineteen nested branches cost a lane's exec mask each)
    for (int k = 0; k < 19; ++k) high |= to[k];
    const uint32_t last = fork >= PHANT_TXS_FORK_PRAGUE ? 0x11u : fork == PHANT_TXS_FORK_CANCUN ? 0x0au : 0x09u;
    return high == 0u && to[19] >= 1u && to[19] <= last;
}

// every error bit of phant_block_transactions[_ex]: all of PHANT_TX_* but PHANT_TX_IS_CREATE
enum : uint32_t { TX_ERROR_BITS = 0x7ffu | 0x7f000u };

// the value of an event of a plain transaction; kind 0: the sender's debit (negative), 1: the recipient's credit, 2: the coinbase's
SETTLE_HD void tx_event(uint32_t kind, uint64_t gas, const uint8_t* value, const uint8_t* price, const uint8_t* base_fee, uint32_t w[LIMBS]) {
    uint32_t p[LIMBS], t[LIMBS];
    if (kind == 1u) {
        load256(value, w);
        return;
    }
    load256(price, p);
    if (kind == 2u) {  // (price >= base_fee: the row is plain)
        load256(base_fee, t);
        sub320(p, t);
    }
    mul_u64_u256(gas, p, w);
    if (kind == 0u) {
        load256(value, t);
        add320(w, t);
        neg320(w);
    }
}
SETTLE_HD void wd_event(uint64_t gwei, uint32_t w[LIMBS]) {
    const uint32_t giga[8] = {1000000000u, 0, 0, 0, 0, 0, 0, 0};
    mul_u64_u256(gwei, giga, w);
}

// One transaction's own inputs: everything its class reads.  to_code_hash: code_hashes[to_row], or nullptr when to_row is NONE.
struct TxRow {
    uint32_t fork, type, tx_flags, state_flags, sender_row, to_row;
    uint64_t intrinsic_gas, floor_gas;
    const uint8_t *value, *price, *to, *base_fee, *to_code_hash;
};
// -> PHANT_SETTLE_UPSTREAM, PHANT_SETTLE_NOT_PLAIN or 0 (plain); gas = gas_used of a plain row, else 0
SETTLE_HD uint32_t classify(const TxRow& r, uint64_t& gas) {
    gas = 0;
    const uint64_t g = r.intrinsic_gas > r.floor_gas ? r.intrinsic_gas : r.floor_gas;
    if ((r.tx_flags & TX_ERROR_BITS) || (r.state_flags & (PHANT_TXST_SKIPPED | PHANT_TXST_ERROR_BITS)) || less_be256(r.price, r.base_fee))
        return PHANT_SETTLE_UPSTREAM;
    if (r.sender_row == PHANT_ROW_NONE || (r.to_row == PHANT_ROW_NONE && !(r.tx_flags & PHANT_TX_IS_CREATE))) return PHANT_SETTLE_UPSTREAM;
    uint32_t debit[LIMBS];
    tx_event(0u, g, r.value, r.price, r.base_fee, debit);
    neg320(debit);
    if (debit[8] | debit[9]) return PHANT_SETTLE_UPSTREAM;  // (beyond 2^256 - 1: never behind an upfront_cost that fits)
    if (r.type == 3u || r.type == 4u || (r.tx_flags & PHANT_TX_IS_CREATE) || (r.state_flags & PHANT_TXST_UNDETERMINED)) return PHANT_SETTLE_NOT_PLAIN;
    if (!txst::is_empty_code_hash(r.to_code_hash) || is_precompile(r.fork, r.to)) return PHANT_SETTLE_NOT_PLAIN;
    gas = g;
    return 0u;
}

// A plain row against the two running sums.  cum: the gas of the plain rows up to AND including it (96 bits); before: its sender's
// balance with every earlier event.  -> the error bits; cum_out: cumulative_gas_used
SETTLE_HD uint32_t row_rule(uint64_t gas, uint64_t gas_limit, uint64_t block_gas_limit, const uint32_t cum[3], const uint32_t before[LIMBS],
                            const uint8_t* upfront_cost, uint64_t& cum_out) {
    uint32_t f = 0u;
    // cum_before + gas_limit against block_gas_limit, in 128 bits
    uint32_t s[4] = {cum[0], cum[1], cum[2], 0u};
    const uint32_t sub[4] = {(uint32_t)gas, (uint32_t)(gas >> 32), 0u, 0u}, add[4] = {(uint32_t)gas_limit, (uint32_t)(gas_limit >> 32), 0u, 0u};
    wide::sub<4>(s, sub);
    wide::add<4>(s, add);
    if ((s[2] | s[3]) != 0u || ((uint64_t)s[1] << 32 | s[0]) > block_gas_limit) f |= PHANT_SETTLE_GAS_LIMIT;
    cum_out = cum[2] ? ~0ull : (uint64_t)cum[1] << 32 | cum[0];
    uint32_t cost[LIMBS];
    load256(upfront_cost, cost);
    if (below(before, cost)) f |= PHANT_SETTLE_BALANCE_SHORT;
    return f;
}

// A touched pre-state row: total = its balance plus all its events -> account_op; nonce_after, balance[8], flags
SETTLE_HD uint32_t account_rule(uint8_t status, uint64_t nonce, uint32_t sends, const uint32_t total[LIMBS], bool code_empty, uint64_t& nonce_after,
                                uint32_t balance[8], uint32_t& flags) {
    nonce_after = nonce + sends;
    if (nonce_after < nonce) nonce_after = ~0ull;
    flags = clamp256(total, balance);
    uint32_t any = 0u;
    for (int k = 0; k < 8; ++k) any |= balance[k];
    if (nonce_after == 0u && any == 0u && code_empty) return status == PHANT_PROOF_PRESENT ? PHANT_POST_DELETE : PHANT_POST_KEEP;  // EIP-161
    return PHANT_POST_SET;
}

#ifndef PHANT_SETTLE_RULE_ONLY

// ctl[0]: what the rows' check found, [1]: max(n - i) over the rows with an error bit, [2]: rows that are not plain, [3]: max(n - i)
// over those, [4]: block_flags, [5]: withdrawals dropped, [6 .. 7]: the block's gas_used
enum : uint32_t { CTL_WORDS = 8 };
enum : uint32_t { NONE = PHANT_ROW_NONE, SEG_WORDS = seg::SEG_WORDS, TILE = seg::TILE };
using Seg = seg::Seg<LIMBS>;  // {signed sum, sender events, "a segment starts at or before me in what was combined"}

// the call's device arrays
struct Args {
    phant_settle_in in;   // every pointer device memory
    phant_settle_out o;
    uint32_t* ctl;
    uint32_t* touched;    // a bit per pre-state row
    uint64_t* gas;        // n: gas_used of a plain row, else 0
    uint64_t* keys;       // events: the account row (n_accounts: the event does not exist) -- the sort's input
    uint32_t* vals;       // events: the event number
    uint32_t* loc;        // (ev_tiles + gas_tiles) x TILE x SEG_WORDS: the scan inside a tile
    uint32_t* agg;        // a tile's last
    uint32_t* tp;         // what runs into a tile
    uint32_t events;      // 3 n + n_wd
    uint32_t ev_tiles, gas_tiles;
};

__global__ void __launch_bounds__(256) settle_check_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const phant_settle_in& in = a.in;
    bool bad = false;
    if (i < in.n) {
        const uint32_t s = in.sender_row[i], r = in.to_row[i];
        bad = (s != NONE && s >= in.n_accounts) || (r != NONE && r >= in.n_accounts);
    }
    if (i < in.n_wd) {
        const uint32_t w = in.wd_row[i];
        bad = bad || (w != NONE && w >= in.n_accounts);
    }
    if (bad) atomicOr(a.ctl, 1u);
}

__device__ inline void touch(const Args& a, uint32_t row) {
    if (keyed::wave_first_of(row != NONE, row)) atomicOr(a.touched + (row >> 5), 1u << (row & 31u));
}

__global__ void __launch_bounds__(256) settle_classify_kernel(Args a) {
    const phant_settle_in& in = a.in;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, na = in.n_accounts;
    const bool coinbase_known = in.coinbase_row != NONE && txst::proven(in.account_status[in.coinbase_row]);
    uint32_t row0 = NONE, row1 = NONE, row2 = NONE;
    bool not_plain = false, no_coinbase = false, dropped = false;
    if (g < in.n) {
        TxRow r;
        r.fork = in.fork, r.type = in.type[g], r.tx_flags = in.tx_flags[g], r.state_flags = in.state_flags[g];
        r.sender_row = in.sender_row[g], r.to_row = in.to_row[g];
        r.intrinsic_gas = in.intrinsic_gas[g], r.floor_gas = in.floor_gas ? in.floor_gas[g] : 0ull;
        r.value = in.value + 32ull * g, r.price = in.effective_gas_price + 32ull * g, r.to = in.to + 20ull * g, r.base_fee = in.base_fee;
        r.to_code_hash = r.to_row == NONE ? nullptr : in.code_hashes + 32ull * r.to_row;
        uint64_t gas;
        const uint32_t cls = classify(r, gas);
        a.o.settle_flags[g] = cls;
        a.gas[g] = gas;
        if (!cls) row0 = r.sender_row, row1 = r.to_row, row2 = coinbase_known ? in.coinbase_row : (uint32_t)NONE;
        not_plain = cls == PHANT_SETTLE_NOT_PLAIN, no_coinbase = !cls && !coinbase_known;
        const uint32_t e = 3u * g;
        a.keys[e] = row0 == NONE ? na : row0, a.keys[e + 1u] = row1 == NONE ? na : row1, a.keys[e + 2u] = row2 == NONE ? na : row2;
        a.vals[e] = e, a.vals[e + 1u] = e + 1u, a.vals[e + 2u] = e + 2u;
    } else if (g - in.n < in.n_wd) {
        const uint32_t j = g - in.n, w = in.wd_row[j], e = 3u * in.n + j;
        dropped = w == NONE || !txst::proven(in.account_status[w]);
        if (!dropped) row0 = w;
        a.o.wd_flags[j] = dropped ? PHANT_SETTLE_WD_UNKNOWN : 0u;
        a.keys[e] = dropped ? na : w, a.vals[e] = e;
    }
    touch(a, row0);
    touch(a, row1);
    touch(a, row2);
    // the counts: one atomic per wave each (the lowest lane that has something to say holds the lowest index)
    const unsigned long long m_np = __ballot(not_plain), m_cb = __ballot(no_coinbase), m_wd = __ballot(dropped);
    if (m_np && lane == (uint32_t)__builtin_ctzll(m_np)) {
        atomicAdd(a.ctl + 2, (uint32_t)__builtin_popcountll(m_np));
        atomicMax(a.ctl + 3, in.n - g);
    }
    if (m_cb && lane == (uint32_t)__builtin_ctzll(m_cb)) atomicOr(a.ctl + 4, PHANT_SETTLE_COINBASE_UNKNOWN);
    if (m_wd && lane == (uint32_t)__builtin_ctzll(m_wd)) atomicAdd(a.ctl + 5, (uint32_t)__builtin_popcountll(m_wd));
}

// the value of event e, which exists
__device__ inline void event_of(const Args& a, uint32_t e, uint32_t w[LIMBS]) {
    const phant_settle_in& in = a.in;
    const uint32_t n3 = 3u * in.n;
    if (e >= n3) {
        wd_event(in.wd_amount_gwei[e - n3], w);
        return;
    }
    const uint32_t i = e / 3u;
    tx_event(e - 3u * i, a.gas[i], in.value + 32ull * i, in.effective_gas_price + 32ull * i, in.base_fee, w);
}
__device__ inline bool is_sender_event(const Args& a, uint32_t e) { return e < 3u * a.in.n && e % 3u == 0u; }

// workgroups [0, ev_tiles): the sorted events; [ev_tiles, ev_tiles + gas_tiles): gas_used in block order (f stays 0: one plain sum)
__global__ void __launch_bounds__(256) settle_scan_tiles_kernel(Args a, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
    __shared__ Seg s_wave[4];
    const uint32_t tid = threadIdx.x;
    Seg s;
    seg::zero(s);
    if (blockIdx.x < a.ev_tiles) {
        const uint32_t p = blockIdx.x * TILE + tid;
        if (p < a.events) {
            const uint64_t key = keys[p];
            s.f = (p == 0u || keys[p - 1u] != key) ? 1u : 0u;
            if (key != a.in.n_accounts) {
                const uint32_t e = vals[p];
                event_of(a, e, s.w);
                s.cnt = is_sender_event(a, e) ? 1u : 0u;
            }
        }
    } else {
        const uint32_t i = (blockIdx.x - a.ev_tiles) * TILE + tid;
        if (i < a.in.n) {
            const uint64_t g = a.gas[i];
            s.w[0] = (uint32_t)g, s.w[1] = (uint32_t)(g >> 32);
        }
    }
    seg::scan_block(s, tid, s_wave);
    seg::store(a.loc + (size_t)SEG_WORDS * ((size_t)blockIdx.x * TILE + tid), s);
    if (tid == TILE - 1u) seg::store(a.agg + (size_t)SEG_WORDS * blockIdx.x, s);
}

// tp[t] = what runs into tile t: the tiles of its kind before it combined.  Workgroup 0: the events' tiles, 1: the gas's
__global__ void __launch_bounds__(256) settle_scan_aggr_kernel(Args a) {
    __shared__ Seg s_wave[4];
    __shared__ Seg s_carry;
    seg::aggregate(a.agg, a.tp, blockIdx.x ? a.ev_tiles : 0u, blockIdx.x ? a.gas_tiles : a.ev_tiles, threadIdx.x, s_wave, &s_carry);
}

// transaction i, whose sender event stands at sorted slot p with the scan `here` (exists: the row is plain)
__device__ inline void finish_row(const Args& a, uint32_t i, bool exists, const Seg& here) {
    const phant_settle_in& in = a.in;
    uint32_t f = a.o.settle_flags[i];  // (the class, from the classify kernel)
    uint64_t cum_out = 0;
    uint32_t bal[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Seg gas;  // (the gas of row i stands at slot ev_tiles x TILE + i)
    seg::scan_at(a.loc, a.tp, (size_t)a.ev_tiles * TILE + i, gas);
    if (exists) {
        const uint32_t s = in.sender_row[i];
        uint32_t before[LIMBS], own[LIMBS];
        event_of(a, 3u * i, own);
        load256(in.balances + 32ull * s, before);
        add320(before, here.w);
        sub320(before, own);
        f |= row_rule(a.gas[i], in.gas_limit[i], in.block_gas_limit, gas.w, before, in.upfront_cost + 32ull * i, cum_out);
        (void)clamp256(before, bal);
    }
    a.o.settle_flags[i] = f;
    a.o.cumulative_gas_used[i] = cum_out;
    wide::store_be256(a.o.balance_before + 32ull * i, bal);
    if (f & PHANT_SETTLE_ERROR_BITS) atomicMax(a.ctl + 1, in.n - i);
    if (i + 1u == in.n) a.ctl[6] = gas.w[2] ? 0xffffffffu : gas.w[0], a.ctl[7] = gas.w[2] ? 0xffffffffu : gas.w[1];
}

__device__ inline void copy32(uint8_t* dst, const uint8_t* src) {
    for (int k = 0; k < 32; ++k) dst[k] = src[k];
}

// lanes [0, events): the sorted events; [events, events + n_accounts): the pre-state rows
__global__ void __launch_bounds__(256) settle_finish_kernel(Args a, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
    const phant_settle_in& in = a.in;
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g < a.events) {
        const uint32_t p = (uint32_t)g, e = vals[p];
        const uint64_t key = keys[p];
        const bool exists = key != in.n_accounts;
        Seg here;
        seg::zero(here);
        if (exists) seg::scan_at(a.loc, a.tp, p, here);
        if (is_sender_event(a, e)) finish_row(a, e / 3u, exists, here);
        if (exists && (p + 1u == a.events || keys[p + 1u] != key)) {  // the last event of row j's segment
            const uint32_t j = (uint32_t)key;
            uint32_t total[LIMBS], bal[8], flags;
            uint64_t nonce_after;
            load256(in.balances + 32ull * j, total);
            add320(total, here.w);
            const uint32_t op = account_rule(in.account_status[j], in.nonces[j], here.cnt, total, txst::is_empty_code_hash(in.code_hashes + 32ull * j),
                                             nonce_after, bal, flags);
            a.o.account_op[j] = (uint8_t)op;
            a.o.nonces_after[j] = nonce_after;
            wide::store_be256(a.o.balances_after + 32ull * j, bal);
            a.o.account_flags[j] = (uint8_t)flags;
        }
    } else if (g - a.events < in.n_accounts) {
        const uint32_t j = (uint32_t)(g - a.events);
        copy32(a.o.code_hashes_after + 32ull * j, in.code_hashes + 32ull * j);
        if (!((a.touched[j >> 5] >> (j & 31u)) & 1u)) {
            a.o.account_op[j] = PHANT_POST_KEEP;
            a.o.nonces_after[j] = in.nonces[j];
            copy32(a.o.balances_after + 32ull * j, in.balances + 32ull * j);
            a.o.account_flags[j] = 0u;
        }
    }
}

// the arrays that cross the bus in the host form: (member, type, elements)
#define SETTLE_INPUTS(X)                                                                                                                        \
    X(base_fee, uint8_t, 32) X(type, uint8_t, n) X(tx_flags, uint32_t, n) X(gas_limit, uint64_t, n) X(intrinsic_gas, uint64_t, n)                  \
    X(floor_gas, uint64_t, (in.floor_gas ? n : 0u)) X(value, uint8_t, 32 * (size_t)n) X(effective_gas_price, uint8_t, 32 * (size_t)n)              \
    X(upfront_cost, uint8_t, 32 * (size_t)n) X(to, uint8_t, 20 * (size_t)n) X(sender_row, uint32_t, n) X(to_row, uint32_t, n) X(state_flags, uint32_t, n) \
    X(account_status, uint8_t, na) X(nonces, uint64_t, na) X(balances, uint8_t, 32 * (size_t)na) X(code_hashes, uint8_t, 32 * (size_t)na)          \
    X(wd_row, uint32_t, nw) X(wd_amount_gwei, uint64_t, nw)
#define SETTLE_OUTPUTS(X)                                                                                                                       \
    X(settle_flags, uint32_t, n) X(cumulative_gas_used, uint64_t, n) X(balance_before, uint8_t, 32 * (size_t)n) X(account_op, uint8_t, na)         \
    X(nonces_after, uint64_t, na) X(balances_after, uint8_t, 32 * (size_t)na) X(code_hashes_after, uint8_t, 32 * (size_t)na) X(account_flags, uint8_t, na) \
    X(wd_flags, uint8_t, nw)

// what the host form refuses before anything is copied
inline const char* check_host(const phant_settle_in& in) {
    auto ok = [&](uint32_t r) { return r == NONE || r < in.n_accounts; };
    for (uint32_t i = 0; i < in.n; ++i)
        if (!ok(in.sender_row[i]) || !ok(in.to_row[i])) return "a sender_row / to_row is neither a pre-state row nor the NONE value";
    for (uint32_t j = 0; j < in.n_wd; ++j)
        if (!ok(in.wd_row[j])) return "a wd_row is neither a pre-state row nor the NONE value";
    return nullptr;
}

}  // namespace settle

int32_t block_settle(Workspaces& ws, hipStream_t st, const phant_settle_in& in, phant_settle_out& out, bool dev, std::string& err) {
    using namespace settle;
    const uint32_t n = in.n, na = in.n_accounts, nw = in.n_wd;
    const uint32_t events = 3u * n + nw;  // (below 2^31: checked by the caller)
    CALL_TRY("block_settle", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_SETTLE_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_SETTLE;
    if (!dev)
        if (const char* what = check_host(in)) return err = std::string("block_settle: ") + what, PHANT_E_INVALID_ARG;

    // ---- the arena: the zeroed words (control, the sort's digit totals, the touched marks) and the outputs in front (one span goes
    // back), (host form) the inputs, then what the sort and the scan need
    const uint32_t ev_tiles = (events + TILE - 1u) / TILE, gas_tiles = (n + TILE - 1u) / TILE, tiles = ev_tiles + gas_tiles;
    const size_t zero_words = (size_t)CTL_WORDS + 512 + ((size_t)na + 31) / 32;
    Args a;
    std::memset(&a, 0, sizeof a);
    a.in = in;
    a.events = events, a.ev_tiles = ev_tiles, a.gas_tiles = gas_tiles;
    uint32_t *zero = nullptr, *digit_totals = nullptr, *hist = nullptr, *vals_alt = nullptr;
    uint64_t* keys_alt = nullptr;
    uint8_t* in_end = nullptr;
    auto carve = [&](auto& io) {
        zero = io.template take<uint32_t>(zero_words);
#define X(m, T, e) a.o.m = io.template take<T>(e);
        SETTLE_OUTPUTS(X)
#undef X
        if (!dev) {
#define X(m, T, e) a.in.m = io.template take<T>(e);
            SETTLE_INPUTS(X)
#undef X
        }
        in_end = io.template take<uint8_t>(0);
        a.gas = io.template take<uint64_t>(n);
        a.keys = io.template take<uint64_t>(events);
        keys_alt = io.template take<uint64_t>(events);
        a.vals = io.template take<uint32_t>(events);
        vals_alt = io.template take<uint32_t>(events);
        hist = io.template take<uint32_t>(sort_hist_entries(events));
        a.loc = io.template take<uint32_t>((size_t)SEG_WORDS * TILE * tiles);
        a.agg = io.template take<uint32_t>((size_t)SEG_WORDS * tiles);
        a.tp = io.template take<uint32_t>((size_t)SEG_WORDS * (tiles ? tiles : 1u));
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_settle", "workspace", err)) return rc;
    if (!in.floor_gas) a.in.floor_gas = nullptr;
    a.ctl = zero, digit_totals = zero + CTL_WORDS;
    a.touched = digit_totals + 512;
    CALL_TRY("block_settle", hipMemsetAsync(zero, 0, 4 * zero_words, st));

    // ---- in: (host form) every array in ONE copy through the pinned stage where they fit it; (device form) the check
    if (!dev) {
        StagedInputs ins(ws, st, a.in.base_fee, in_end);
#define X(m, T, e) ins.put(a.in.m, in.m, (size_t)(e) * sizeof(T));
        SETTLE_INPUTS(X)
#undef X
        CALL_TRY("block_settle", ins.finish());
    } else if (std::max(n, nw)) {
        hipLaunchKernelGGL(settle_check_kernel, dim3((std::max(n, nw) + 255u) / 256u), dim3(256), 0, st, a);
        CALL_TRY("block_settle", hipGetLastError());
        CALL_TRY("block_settle", ws.read_words(Workspaces::MAILBOX_SETTLE, a.ctl, CTL_WORDS, st));
        if (mb[0]) return err = "block_settle_dev: a sender_row / to_row / wd_row is neither a pre-state row nor the NONE value", PHANT_E_INVALID_ARG;
    }

    // ---- the classes, the order, the scans, the outputs
    const uint64_t* keys = a.keys;
    const uint32_t* vals = a.vals;
    if (events) {
        hipLaunchKernelGGL(settle_classify_kernel, dim3((n + nw + 255u) / 256u), dim3(256), 0, st, a);
        CALL_TRY("block_settle", hipGetLastError());
        uint64_t* k_out = nullptr;
        uint32_t* v_out = nullptr;
        CALL_TRY("block_settle", launch_sort_pairs(a.keys, a.vals, keys_alt, vals_alt, events, sort_key_bits(na), hist, digit_totals, &k_out, &v_out, st));
        keys = k_out, vals = v_out;
        hipLaunchKernelGGL(settle_scan_tiles_kernel, dim3(tiles), dim3(256), 0, st, a, keys, vals);
        CALL_TRY("block_settle", hipGetLastError());
        hipLaunchKernelGGL(settle_scan_aggr_kernel, dim3(2), dim3(256), 0, st, a);
        CALL_TRY("block_settle", hipGetLastError());
    }
    if ((uint64_t)events + na) {
        hipLaunchKernelGGL(settle_finish_kernel, dim3((uint32_t)(((uint64_t)events + na + 255u) / 256u)), dim3(256), 0, st, a, keys, vals);
        CALL_TRY("block_settle", hipGetLastError());
    }

    // ---- out: the control words and everything up to the last wanted output (one span in the host form while it fits the pinned stage)
    CallOutputs outs(ws, st, dev, a.ctl, a.ctl, Workspaces::MAILBOX_SETTLE, CTL_WORDS);
#define X(m, T, e) outs.add(out.m, a.o.m, (size_t)(e) * sizeof(T));
    SETTLE_OUTPUTS(X)
#undef X
    CALL_TRY("block_settle", outs.deliver());
    const volatile uint32_t* const c = outs.ctl();
    out.first_bad = n - c[1], out.n_not_plain = c[2], out.first_not_plain = n - c[3], out.block_flags = c[4], out.n_wd_unknown = c[5];
    out.gas_used = (uint64_t)c[7] << 32 | c[6];
    return PHANT_OK;
}

#undef SETTLE_INPUTS
#undef SETTLE_OUTPUTS

}  // namespace phant
#else
}  // namespace settle
}  // namespace phant
#endif  // PHANT_SETTLE_RULE_ONLY
#undef SETTLE_HD
