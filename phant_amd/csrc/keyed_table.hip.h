// keyed_table.hip.h -- the open-addressing index tables of the block calls, stated ONCE (DESIGN.md sections 7k and 7m): a slot holds an
// entry's index or NONE; an entry is looked for first where a KEYED mix of its bytes says (witness keys and access-list keys are
// attacker-chosen bytes: without the ctx's key nobody aims them at one slot) and then slot by slot.  txstate.hip.h keeps its address
// table in one (in global memory, or its small kernel's in LDS), access_lists.hip.h its slot, tuple and key tables.
//
// The first part is plain C++ that needs no HIP header (the stand-alone programs under tests/native/ build it with a bare g++); the
// part that claims, finds and votes is device code.
#pragma once
#include <stdint.h>

#include "../../include/phant_gpu.h"

#if defined(__HIP__)
#define PHANT_KEYED_FN __host__ __device__ inline
#else
#define PHANT_KEYED_FN inline
#endif

namespace phant {
namespace keyed {

// an address as five words, and the compare over all of it
PHANT_KEYED_FN void load_addr(const uint8_t* p, uint32_t w[5]) {
    for (int k = 0; k < 5; ++k) w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
}
PHANT_KEYED_FN bool same_addr(const uint8_t* p, const uint32_t w[5]) {
    uint32_t v[5];
    load_addr(p, v);
    return v[0] == w[0] && v[1] == w[1] && v[2] == w[2] && v[3] == w[3] && v[4] == w[4];
}
// where five words are looked for first: a keyed mix of all of them
PHANT_KEYED_FN uint32_t home_slot(const uint32_t w[5], uint32_t salt0, uint32_t salt1) {
    uint32_t h = salt0;
    for (int k = 0; k < 5; ++k) {
        h = (h ^ w[k]) * 0x9E3779B1u;
        h ^= h >> 15;
        h = (h + salt1) * 0x85EBCA77u;
        h ^= h >> 13;
    }
    return h * 0xC2B2AE3Du;
}
// a table's slots: a power of two, at least twice the entries (entries <= 2^30), at least 64
inline uint32_t table_slots(uint64_t entries) {
    uint32_t slots = 64;
    while (slots < 2ull * entries) slots <<= 1;
    return slots;
}

#if defined(__HIP__) || defined(PHANT_HOST_EMU)

// `me` into a table: a free slot is claimed by compare-and-swap; a slot whose holder is `same` as me is lowered to the lower index, so
// equal entries resolve to the lowest whatever the order of arrival.  (A slot only ever holds entries equal to its first; the table is at
// most half full: the walk ends long before it has gone round.)
template <class Same>
__device__ inline void claim(uint32_t* table, uint32_t mask, uint32_t home, uint32_t me, Same same) {
    uint32_t slot = home & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint32_t old = atomicCAS(table + slot, (uint32_t)PHANT_ROW_NONE, me);
        if (old == PHANT_ROW_NONE) return;
        if (same(old)) {
            atomicMin(table + slot, me);
            return;
        }
        slot = (slot + 1u) & mask;
    }
}
template <class Same>
__device__ inline uint32_t find(const uint32_t* table, uint32_t mask, uint32_t home, Same same) {
    uint32_t slot = home & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint32_t j = table[slot];
        if (j == PHANT_ROW_NONE) return PHANT_ROW_NONE;
        if (same(j)) return j;
        slot = (slot + 1u) & mask;
    }
    return PHANT_ROW_NONE;
}

// Of the lanes of a wave that have something to say about the same row, the lowest: many transactions name one recipient, and atomics
// on one address are served one at a time.  Every lane of the wave calls this; the loop runs once per distinct row in the wave.
__device__ inline bool wave_first_of(bool has, uint32_t row) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(has);
    bool first = false;
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t theirs = (uint32_t)__shfl((int)row, (int)leader);
        const unsigned long long same = __ballot(has && row == theirs);
        if (lane == leader) first = true;
        todo &= ~same;
    }
    return first;
}

#endif

}  // namespace keyed
}  // namespace phant
#undef PHANT_KEYED_FN
