// fee_history.hip.h -- the reward percentiles of a chain segment (included by bulk_keccak.hip behind filters.hip.h):
// per block the priority fee at chosen percentiles of its gas used, eth_feeHistory's `reward`, from the effective_gas_price rows
// phant_block_bodies leaves and the gas_used rows phant_block_receipt_segments leaves.  include/phant_gpu.h has the contract,
// tests/feehist_ref.py the same in Python integers.
//
//   fh_check_kernel       device form only: seg::first_flags over block_first and the cap on a block's rows; the host reads the verdict
//                         before anything indexes with them
//   fh_tip_kernel         a lane per row: tip = price - the block's base fee in 256 bits (wide_uint.h), zero and the block's
//                         PHANT_FEE_BELOW_BASE where that would borrow; the tip's bytes and its limbs
//   fh_rank_kernel        a wave per 64 consecutive rows: the blocks of its lanes cover ONE contiguous range of rows, which the wave
//                         walks once -- the walked key is wave-uniform (scalar loads), each lane holds its own key in 8 VGPRs and counts
//                         the walked rows of its block that come before it by (tip, row); order[block_first[b] + rank] = row.  A
//                         stable sort without atomics, LDS or a lane that loops on its own; quadratic in a block's rows, hence the cap
//   fh_scan_tiles_kernel  tiles of 256: seg_scan.hip.h's SEGMENTED inclusive scan (L = 3: 96 bits) of gas_used[order[p]] over the slots
//                         in sorted order, a segment starting at every block's first slot
//   fh_scan_aggr_kernel   one workgroup: the same scan over the tiles' aggregates
//   fh_select_kernel      a lane per (block, percentile): G from the scan at the block's last slot, a bisection of the block's slots
//                         for the least rank whose sum reaches the threshold (fh::reaches: no division), that row's tip; behind them a
//                         lane per block: block_gas_used, block_flags, first_bad_block
//
// Five launches, the device form's check one more, whatever n_blocks, n and n_percentiles are.  Plain C++ plus readfirstlane:
// tests/emu.py compiles this file for the host.
#pragma once
#include "feehist_check.h"
#include "seg_scan.hip.h"
#include "segment_lists.hip.h"
#include "staging.h"

namespace phant {
namespace fh {

// the call's control words (device memory): [0] = seg::F_INVALID / F_TOO_LONG of the check (zeroed), [1] = first_bad_block (the tip
// kernel sets it to n_blocks, the select kernel lowers it)
constexpr uint32_t CTL_WORDS = 4, CTL_FIRST_BAD = 1;using Seg = seg::Seg<3>;
using seg::SEG_WORDS;
using seg::TILE;

struct Args {
    const uint32_t* block_first;
    const uint8_t *price, *base_fee;
    const uint64_t* gas_used;
    const uint32_t* percentile;  // device memory
    uint32_t n_blocks, n, n_pct, block_max;
    uint32_t tiles;  // ceil(n / 256)
    uint32_t* ctl;
    uint8_t *reward, *tip;
    uint32_t* order;
    uint64_t* block_gas_used;
    uint32_t* block_flags;  // zeroed
    uint32_t* tipw;         // n x 8 limbs
    uint32_t *loc, *agg, *tp;
};

// ---- the device form's check: a lane per block
__global__ void __launch_bounds__(256) fh_check_kernel(Args a) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.n_blocks) return;
    uint32_t bad = seg::first_flags(a.block_first, b, a.n_blocks, a.n);
    if (!bad && a.block_first[b + 1u] - a.block_first[b] > a.block_max) bad = seg::F_TOO_LONG;
    if (bad) atomicOr(a.ctl, bad);
}

// ---- tips: a lane per row
__global__ void __launch_bounds__(256) fh_tip_kernel(Args a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) a.ctl[CTL_FIRST_BAD] = a.n_blocks;
    if (i >= a.n) return;
    const uint32_t b = seg::block_of(a.block_first, a.n_blocks, i);
    uint32_t t[8], base[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    wide::load_be256<8>(a.price + 32ull * i, t);
    if (a.base_fee) wide::load_be256<8>(a.base_fee + 32ull * b, base);
    if (wide::less<8>(t, base)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = 0u;
        atomicOr(a.block_flags + b, (uint32_t)PHANT_FEE_BELOW_BASE);
    } else {
        wide::sub<8>(t, base);
    }
    wide::store_be256(a.tip + 32ull * i, t);
    uint4* const w = reinterpret_cast<uint4*>(a.tipw + 8ull * i);
    w[0] = make_uint4(t[0], t[1], t[2], t[3]);
    w[1] = make_uint4(t[4], t[5], t[6], t[7]);
}

// ---- ranks: a wave per 64 consecutive rows
__global__ void __launch_bounds__(256) fh_rank_kernel(Args a) {
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))), lane = threadIdx.x & 63u;
    const uint32_t i0 = 64u * wv;
    if (i0 >= a.n) return;  // (whole waves)
    // the rows the wave walks: from the first row of its first lane's block to the last row of its last lane's block (uniform)
    const uint32_t last = a.n - i0 > 64u ? i0 + 63u : a.n - 1u;
    const uint32_t lo = a.block_first[seg::block_of(a.block_first, a.n_blocks, i0)];
    const uint32_t hi = a.block_first[seg::block_of(a.block_first, a.n_blocks, last) + 1u];
    const uint32_t i = i0 + lane <= last ? i0 + lane : last;  // (the lanes behind the last row repeat it and write nothing)
    const uint32_t b = seg::block_of(a.block_first, a.n_blocks, i), s = a.block_first[b], e = a.block_first[b + 1u];
    uint32_t mine[8];
    {
        const uint4 x = reinterpret_cast<const uint4*>(a.tipw + 8ull * i)[0], y = reinterpret_cast<const uint4*>(a.tipw + 8ull * i)[1];
        mine[0] = x.x, mine[1] = x.y, mine[2] = x.z, mine[3] = x.w, mine[4] = y.x, mine[5] = y.y, mine[6] = y.z, mine[7] = y.w;
    }
    uint32_t rank = 0;
    for (uint32_t u = lo; u < hi; ++u) {  // (u and the key at u are uniform across the wave)
        const uint32_t* const key = a.tipw + 8ull * u;
        // mine - key - (u >= i): no borrow out exactly when (key, u) < (mine, i) -- equal tips count for the rows in front of i only
        // (the chain's borrow alone, limb by limb: out = mine < key, or mine == key and in -- two compares a limb, no difference kept)
        bool borrow = u >= i;
#pragma unroll
        for (int k = 0; k < 8; ++k) borrow = mine[k] < key[k] || (mine[k] == key[k] && borrow);
        if (u >= s && u < e && !borrow) ++rank;
    }
    if (i0 + lane <= last) a.order[s + rank] = i;  // (rank < e - s: only rows of [s, e) other than i were counted)
}

// ---- the running sums of gas_used in sorted order: settle's two scan kernels over one kind of tile
__global__ void __launch_bounds__(256) fh_scan_tiles_kernel(Args a) {
    __shared__ Seg s_wave[4];
    const uint32_t tid = threadIdx.x, p = blockIdx.x * TILE + tid;
    if (blockIdx.x >= a.tiles) return;  // (a segment without a row: the one workgroup of the launch has no tile)
    Seg s;
    seg::zero(s);
    if (p < a.n) {
        const uint64_t g = a.gas_used[a.order[p]];
        s.w[0] = (uint32_t)g, s.w[1] = (uint32_t)(g >> 32);
        s.f =a.block_first[seg::block_of(a.block_first, a.n_blocks, p)] == p ? 1u : 0u;
    }
    seg::scan_block(s, tid, s_wave);
    seg::store(a.loc + (size_t)SEG_WORDS * ((size_t)blockIdx.x * TILE + tid), s);
    if (tid == TILE - 1u) seg::store(a.agg + (size_t)SEG_WORDS * blockIdx.x, s);
}

__global__ void __launch_bounds__(256) fh_scan_aggr_kernel(Args a) {
    __shared__ Seg s_wave[4];
    __shared__ Seg s_carry;
    seg::aggregate(a.agg, a.tp, 0u, a.tiles, threadIdx.x, s_wave, &s_carry);
}

// ---- select: a lane per (block, percentile), then a lane per block
__global__ void __launch_bounds__(256) fh_select_kernel(Args a) {
    const uint64_t t = blockIdx.x * 256ull + threadIdx.x, rewards = (uint64_t)a.n_blocks * a.n_pct;
    if (t >= rewards + a.n_blocks) return;
    const uint32_t b = t < rewards ? (uint32_t)(t / a.n_pct) : (uint32_t)(t - rewards);
    const uint32_t s = a.block_first[b], e = a.block_first[b + 1u];
    Seg all;
    seg::zero(all);
    if (e > s) seg::scan_at(a.loc, a.tp, (size_t)e - 1u, all);
    if (t >= rewards) {
        const uint32_t flags = a.block_flags[b];
        a.block_gas_used[b] = all.w[2] ? ~0ull : (uint64_t)all.w[1] << 32 | all.w[0];
        if (flags) atomicMin(a.ctl + CTL_FIRST_BAD, b);
        return;
    }
    uint4* const out = reinterpret_cast<uint4*>(a.reward + 32ull * t);
    if (e == s) {
        out[0] = out[1] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t p = a.percentile[(uint32_t)(t - (uint64_t)b * a.n_pct)];
    uint32_t lo = s, hi = e - 1u;  // the least slot whose sum reaches the threshold: the block's last does
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        Seg here;
        seg::scan_at(a.loc, a.tp, (size_t)mid, here);
        if (reaches(here.w, all.w, p)) hi = mid;
        else lo = mid + 1u;
    }
    const uint4* const from = reinterpret_cast<const uint4*>(a.tip + 32ull * a.order[lo]);
    out[0] = from[0], out[1] = from[1];
}

}  // namespace fh

// phant_block_fee_history[_dev]: check_args and check_percentiles have passed and n_blocks != 0.  block_max: the cap on a block's rows
int32_t block_fee_history(Workspaces& ws, hipStream_t st, const phant_fee_history_in& in, phant_fee_history_out& out, bool dev, uint32_t block_max, std::string& err) {
    using namespace fh;
    const char* const call = dev ? "block_fee_history_dev" : "block_fee_history";
    const uint32_t nb = in.n_blocks, n = in.n, np = in.n_percentiles;
    if (too_many_rewards(nb, np)) return err = std::string(call) + ": n_blocks x n_percentiles is 2^31 or more", PHANT_E_UNSUPPORTED;
    if (!dev)
        if (const int32_t rc = check_rows_host(call, in, block_max, err)) return rc;
    CALL_TRY("block_fee_history", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_FH_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_FH;

    Args a;
    std::memset(&a, 0, sizeof a);
    a.block_first = in.block_first, a.price = in.price, a.base_fee = in.base_fee, a.gas_used = in.gas_used;
    a.n_blocks = nb, a.n = n, a.n_pct = np, a.block_max = block_max, a.tiles = blocks_of(n, TILE);
    const size_t rewards = (size_t)nb * np, slots = (size_t)a.tiles * TILE;
    uint32_t* d_pct = nullptr;
    const void *zero_end = nullptr, *inputs_begin = nullptr, *inputs_end = nullptr;
    auto carve = [&](auto& io) {
        a.ctl = io.template take<uint32_t>(CTL_WORDS);
        a.block_flags = io.template take<uint32_t>((size_t)nb);
        zero_end = io.template take<uint8_t>(0);
        a.block_gas_used = io.template take<uint64_t>((size_t)nb);
        a.reward = io.template take<uint8_t>(32 * rewards);
        a.order = io.template take<uint32_t>((size_t)n);
        a.tip = io.template take<uint8_t>(32 * (size_t)n);
        a.tipw = io.template take<uint32_t>(8 * (size_t)n);
        a.loc = io.template take<uint32_t>(SEG_WORDS * slots);
        a.agg = io.template take<uint32_t>(SEG_WORDS * (size_t)a.tiles);
        a.tp = io.template take<uint32_t>(SEG_WORDS * ((size_t)a.tiles + 1));
        d_pct = io.template take<uint32_t>((size_t)np);
        if (!dev) {
            inputs_begin = io.template take<uint8_t>(0);
            take_input(io, a.block_first, (size_t)nb + 1, true);
            take_input(io, a.price, 32 * (size_t)n, n != 0u);
            take_input(io, a.base_fee, 32 * (size_t)nb, in.base_fee != nullptr);
            take_input(io, a.gas_used, (size_t)n, n != 0u);
            take_input(io, a.percentile, (size_t)np, np != 0u);
            inputs_end = io.template take<uint8_t>(0);
        }
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_fee_history", "workspace", err)) return rc;
    CALL_TRY("block_fee_history", hipMemsetAsync(a.ctl, 0, (size_t)(static_cast<const uint8_t*>(zero_end) - reinterpret_cast<uint8_t*>(a.ctl)), st));

    // ---- in: (host form) every input in ONE copy through the pinned stage where they fit it; (device form) the percentiles, the check
    if (!dev) {
        StagedInputs ins(ws, st, inputs_begin, inputs_end);
        ins.put(a.block_first, in.block_first, 4 * ((size_t)nb + 1));
        ins.put(a.price, in.price, 32 * (size_t)n);
        ins.put(a.base_fee, in.base_fee, 32 * (size_t)nb);
        ins.put(a.gas_used, in.gas_used, 8 * (size_t)n);
        ins.put(a.percentile, in.percentile, 4 * (size_t)np);
        CALL_TRY("block_fee_history", ins.finish());
    } else {
        a.percentile = d_pct;
        if (np) CALL_TRY("block_fee_history", hipMemcpyAsync(d_pct, in.percentile, 4 * (size_t)np, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(fh_check_kernel, dim3(blocks_of(nb, 256)), dim3(256), 0, st, a);
        CALL_TRY("block_fee_history", hipGetLastError());
        CALL_TRY("block_fee_history", ws.read_words(Workspaces::MAILBOX_FH, a.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID) return err = "block_fee_history_dev: block_first does not run from 0 to n, or goes backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & seg::F_TOO_LONG) return err = "block_fee_history_dev: a block of more than " + std::to_string(block_max) + " rows", PHANT_E_UNSUPPORTED;
    }

    // ---- tips, ranks, the two scan kernels, the selection: five launches whatever the counts are
    const uint32_t row_blocks = std::max(blocks_of(n, 256), 1u);
    hipLaunchKernelGGL(fh_tip_kernel, dim3(row_blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(fh_rank_kernel, dim3(row_blocks), dim3(256), 0, st, a);
    CALL_TRY("block_fee_history", hipGetLastError());
    hipLaunchKernelGGL(fh_scan_tiles_kernel, dim3(std::max(a.tiles, 1u)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(fh_scan_aggr_kernel, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(fh_select_kernel, dim3(blocks_of(rewards + nb, 256)), dim3(256), 0, st, a);
    CALL_TRY("block_fee_history", hipGetLastError());

    // ---- out: one span from the control words to the last wanted output
    CallOutputs outs(ws, st, dev, a.ctl, a.ctl, Workspaces::MAILBOX_FH, CTL_WORDS);
    outs.add(out.block_flags, a.block_flags, 4 * (size_t)nb);
    outs.add(out.block_gas_used, a.block_gas_used, 8 * (size_t)nb);
    outs.add(out.reward, a.reward, 32 * rewards);
    outs.add(out.order, a.order, 4 * (size_t)n);
    outs.add(out.tip, a.tip, 32 * (size_t)n);
    CALL_TRY("block_fee_history", outs.deliver());
    out.first_bad_block = outs.ctl()[CTL_FIRST_BAD];
    return PHANT_OK;
}

}  // namespace phant
