// wide_uint.h -- unsigned integers of L little-endian 32-bit limbs, stated ONCE for the block calls: txstate.hip.h's 288-bit sums
// (L = 9), settle.hip.h's 320-bit two's-complement balances (L = 10) and its 128-bit gas bound (L = 4), seg_scan.hip.h's combine,
// fee_history.hip.h's 256-bit tips (L = 8) and the 128-bit products of its threshold test (L = 4, feehist_check.h).
//
// Plain C++ that needs <stdint.h> only: the same text is compiled for the device, for the host emulation of the kernels
// (tests/emu.py) and by a bare g++ for the stand-alone programs under tests/native/.
#pragma once
#include <stdint.h>

// In a HIP compilation the inlining is forced and the limb loops are unrolled: a scan's records stay in registers.
#if defined(__HIP__)
#define PHANT_WIDE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PHANT_WIDE_FN inline
#endif

namespace phant {
namespace wide {

// a += b, modulo 2^(32 L)
template <int L>
PHANT_WIDE_FN void add(uint32_t* a, const uint32_t* b) {
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        c += (uint64_t)a[k] + b[k];
        a[k] = (uint32_t)c, c >>= 32;
    }
}
// a -= b, modulo 2^(32 L)
template <int L>
PHANT_WIDE_FN void sub(uint32_t* a, const uint32_t* b) {
    uint64_t borrow = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const uint64_t t = (uint64_t)a[k] - b[k] - borrow;
        a[k] = (uint32_t)t, borrow = (t >> 32) & 1u;
    }
}
// a *= m, modulo 2^(32 L)
template <int L>
PHANT_WIDE_FN void mul_small(uint32_t* a, uint32_t m) {
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        c += (uint64_t)a[k] * m;
        a[k] = (uint32_t)c, c >>= 32;
    }
}
// a = -a in two's complement
template <int L>
PHANT_WIDE_FN void neg(uint32_t* a) {
    uint64_t c = 1;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        c += (uint64_t)(~a[k]);
        a[k] = (uint32_t)c, c >>= 32;
    }
}
// a < b, both unsigned
template <int L>
PHANT_WIDE_FN bool less(const uint32_t* a, const uint32_t* b) {
    for (int k = L - 1; k >= 0; --k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}
// 32 bytes big-endian -> L >= 8 limbs (those from the ninth on are zero)
template <int L>
PHANT_WIDE_FN void load_be256(const uint8_t* row, uint32_t* w) {
    for (int k = 0; k < 8; ++k) {
        const uint8_t* p = row + 28 - 4 * k;
        w[k] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
    }
    for (int k = 8; k < L; ++k) w[k] = 0u;
}
PHANT_WIDE_FN void store_be256(uint8_t* row, const uint32_t w[8]) {
    for (int k = 0; k < 8; ++k) {
        uint8_t* p = row + 28 - 4 * k;
        p[0] = (uint8_t)(w[k] >> 24), p[1] = (uint8_t)(w[k] >> 16), p[2] = (uint8_t)(w[k] >> 8), p[3] = (uint8_t)w[k];
    }
}

}  // namespace wide
}  // namespace phant
