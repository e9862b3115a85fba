// wave_util.hip.h -- the three small helpers the block-level encoders (receipts.hip.h, headers.hip.h) share.  Plain C++ only:
// tests/emu.py compiles this file for the host.
#pragma once
#include "keccak_f1600.hip.h"  // PHANT_DEV

namespace phant {

// first j in [0, cnt) with a[j] > v (a ascending, a[cnt - 1] > v)
PHANT_DEV uint32_t upper_bound(const uint32_t* __restrict__ a, uint32_t cnt, uint32_t v) {
    uint32_t lo = 0, hi = cnt - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] > v) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// lanes of a wave copy len bytes (any alignment on either side)
PHANT_DEV void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t len, uint32_t lane) {
    for (uint64_t k = lane; k < len; k += 64u) dst[k] = src[k];
}

inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1u) / per); }

}  // namespace phant
