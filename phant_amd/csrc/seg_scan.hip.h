// seg_scan.hip.h -- the SEGMENTED inclusive scan of the block calls, stated ONCE (DESIGN.md sections 7k and 7n): txstate.hip.h scans
// {rows, upfront cost} in 32 + 288 bits (L = 9) over the transactions sorted by sender, settle.hip.h {sender events, signed value} in
// 32 + 320 bits (L = 10) over the events sorted by account.  Two levels: a tile of TILE elements in one workgroup -- the wave by
// shuffles, the waves through LDS --, then ONE workgroup over a range of tiles' aggregates.  The kernels stay with their callers; the
// LDS they need (s_wave[4], s_carry) is theirs and is handed in.
//
// Every function is __forceinline__: tests/emu.py tells the cross-lane operations apart by their call site, and the records stay in
// registers (the limb loops are unrolled).
#pragma once
#include <stdint.h>

#include "wide_uint.h"

namespace phant {
namespace seg {

enum : uint32_t { SEG_WORDS = 12, TILE = 256 };  // a record in memory: L limbs, cnt, f, zero padding

// An element: {sum, count, "a segment starts at or before me in what was combined"}
template <int L>
struct Seg {
    static_assert(L + 2 <= (int)SEG_WORDS, "a record holds the limbs, cnt and f");
    uint32_t w[L], cnt, f;
};
template <int L>
__device__ __forceinline__ void zero(Seg<L>& s) {
#pragma unroll
    for (int k = 0; k < L; ++k) s.w[k] = 0u;
    s.cnt = 0u, s.f = 0u;
}
// s = before (+) s
template <int L>
__device__ __forceinline__ void combine(Seg<L>& s, const Seg<L>& before) {
    if (!s.f) {
        wide::add<L>(s.w, before.w);
        s.cnt += before.cnt;
    }
    s.f |= before.f;
}
template <int L>
__device__ __forceinline__ void load(const uint32_t* p, Seg<L>& s) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1], c = reinterpret_cast<const uint4*>(p)[2];
    const uint32_t r[SEG_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int k = 0; k < L; ++k) s.w[k] = r[k];
    s.cnt = r[L], s.f = r[L + 1];
}
template <int L>
__device__ __forceinline__ void store(uint32_t* p, const Seg<L>& s) {
    uint32_t r[SEG_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < L; ++k) r[k] = s.w[k];
    r[L] = s.cnt, r[L + 1] = s.f;
    reinterpret_cast<uint4*>(p)[0] = make_uint4(r[0], r[1], r[2], r[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(r[4], r[5], r[6], r[7]);
    reinterpret_cast<uint4*>(p)[2] = make_uint4(r[8], r[9], r[10], r[11]);
}
// inclusive over the 256 lanes of a workgroup: the wave by shuffles (six steps), the waves in front through LDS.  Every lane calls it.
template <int L>
__device__ __forceinline__ void scan_block(Seg<L>& s, uint32_t tid, Seg<L>* s_wave /* [4] */) {
    const uint32_t lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        Seg<L> o;
#pragma unroll
        for (int k = 0; k < L; ++k) o.w[k] = (uint32_t)__shfl_up((int)s.w[k], d);
        o.cnt = (uint32_t)__shfl_up((int)s.cnt, d);
        o.f = (uint32_t)__shfl_up((int)s.f, d);
        if (lane >= d) combine(s, o);
    }
    if (lane == 63u) s_wave[wave] = s;
    __syncthreads();
    Seg<L> run;
    zero(run);
#pragma unroll
    for (uint32_t w = 0; w < 3u; ++w)
        if (w < wave) {
            Seg<L> t = s_wave[w];
            combine(t, run);
            run = t;
        }
    combine(s, run);
}
// tp[t] = what runs into tile t of the range [first, first + tiles): the range's tiles before it combined, 256 of them at a time.  Every
// lane of ONE workgroup of 256 calls it.
template <int L>
__device__ __forceinline__ void aggregate(const uint32_t* agg, uint32_t* tp, uint32_t first, uint32_t tiles, uint32_t tid, Seg<L>* s_wave /* [4] */,
                                          Seg<L>* s_carry) {
    Seg<L> carry;
    zero(carry);
    if (tid == 0u && tiles) store(tp + (size_t)SEG_WORDS * first, carry);
    for (uint32_t c0 = 0; c0 < tiles; c0 += 256u) {
        const uint32_t t = c0 + tid;
        Seg<L> s;
        zero(s);
        if (t < tiles) load(agg + (size_t)SEG_WORDS * (first + t), s);
        scan_block(s, tid, s_wave);
        combine(s, carry);
        if (t + 1u < tiles) store(tp + (size_t)SEG_WORDS * (first + t + 1u), s);
        if (tid == 255u) *s_carry = s;
        __syncthreads();
        carry = *s_carry;
        __syncthreads();  // (s_wave and s_carry are written again by the next chunk)
    }
}
// the scan up to and including slot q: what its tile's scan left in loc, and what runs into that tile
template <int L>
__device__ __forceinline__ void scan_at(const uint32_t* loc, const uint32_t* tp, size_t q, Seg<L>& here) {
    Seg<L> into;
    load(loc + (size_t)SEG_WORDS * q, here);
    load(tp + (size_t)SEG_WORDS * (q / TILE), into);
    combine(here, into);
}

}  // namespace seg
}  // namespace phant
