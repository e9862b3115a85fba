// segment_lists.hip.h -- what the calls over a chain segment share (included by receipts.hip.h, transactions.hip.h, bodies.hip.h and
// receipt_segments.hip.h): the order of a list keyed by rlp(index) in its trie, the rules of a segment's offsets and
// firsts in the device form (off_flags, first_flags) and in the host form (check_offsets_host, check_firsts_host), the block of a row
// (block_of), a verdict's bytes_differ, and the index-keyed lists of many blocks as ONE forest for trie_forest_dev (IndexForest):
//
//   forest_len_kernel<Src>    a lane per trie value (its length, in trie order) and per trie (its keys' bytes, its first value)
//   (exclusive scan)          radix_sort.hip's, over both at once
//   forest_pairs_kernel<Src>  a WAVE per value: its offset, its key rlp(index) and that key's offset; Src writes its bytes in trie order
//
// Src is a trivially copyable struct, passed by value, that knows the call's lists (body::Src, rseg::Seg): item(g) = value g's trie, pos
// and index there and its len; trie(t, count) = the first value of trie t and how many it has; write(out, it, lane) = a wave writes it.
// Plain C++ plus the cross-lane builtins keyed_table.hip.h uses: tests/emu.py compiles this file for the host.
#pragma once
#include <string>

#include "../../include/phant_gpu.h"
#include "launch.h"
#include "rlp.h"
#include "segment_checks.h"
#include "trie_build.h"
#include "wave_util.hip.h"

namespace phant {
namespace seg {

#define SEG_HD __host__ __device__ inline

// ---- trie order <-> index order of n items keyed by rlp(index): indices 1 .. 0x7f, then 0 (key 0x80), then 0x80 onward
SEG_HD uint32_t pos_of_index(uint32_t i, uint32_t n) {
    const uint32_t k = n < 128u ? n : 128u;
    if (i == 0u) return k - 1u;
    return i < k ? i - 1u : i;
}
SEG_HD uint32_t index_of_pos(uint32_t p, uint32_t n) {
    const uint32_t k = n < 128u ? n : 128u;
    if (p == k - 1u) return 0u;
    return p < k - 1u ? p + 1u : p;
}
// bytes of the keys in front of position p of one list (positions below 128 hold the one-byte keys of indices 0 .. 0x7f)
SEG_HD uint32_t key_bytes_before(uint32_t p) {
    uint64_t b = p;
    if (p > 0x80u) b += p - 0x80u;
    if (p > 0x100u) b += p - 0x100u;
    if (p > 0x10000u) b += p - 0x10000u;
    if (p > 0x1000000u) b += p - 0x1000000u;
    return (uint32_t)b;
}

// ---- a segment's arguments: 64-bit offsets from 0 to `bytes`, never backwards, no item of 4 GiB; 32-bit firsts from 0 to `total`,
// never backwards.  Device form: the flags of entry i, ORed into the call's first control word
enum : uint32_t { F_INVALID = 1u, F_TOO_LONG = 2u };
PHANT_DEV uint32_t off_flags(const uint64_t* __restrict__ off, uint32_t i, uint32_t n, uint64_t bytes) {
    const uint64_t b = off[i], e = off[i + 1u];
    if (e < b || (i == 0u && b != 0u) || (i + 1u == n && e != bytes)) return F_INVALID;
    return e - b > 0xffffffffull ? (uint32_t)F_TOO_LONG : 0u;
}
PHANT_DEV uint32_t first_flags(const uint32_t* __restrict__ first, uint32_t i, uint32_t n, uint32_t total) {
    const uint32_t b = first[i], e = first[i + 1u];
    return e < b || (i == 0u && b != 0u) || (i + 1u == n && e != total) ? (uint32_t)F_INVALID : 0u;
}
// Host form: check_offsets_host and check_firsts_host of segment_checks.h, plain C++ a host-only program can include

// the block of row i < block_first[n_blocks] (an upper bound: empty blocks are skipped)
PHANT_DEV uint32_t block_of(const uint32_t* __restrict__ block_first, uint32_t n_blocks, uint32_t i) {
    return upper_bound(block_first, n_blocks + 1u, i) - 1u;
}

PHANT_DEV bool bytes_differ(const uint8_t* x, const uint8_t* y, uint32_t n) {
    uint32_t d = 0;
    for (uint32_t k = 0; k < n; ++k) d |= (uint32_t)(x[k] ^ y[k]);
    return d != 0u;
}

// ---- the index-keyed pairs of a forest: `total` values in `tries` lists, each list in trie order
struct IndexForest {
    uint32_t total, tries;
    uint32_t* len;        // total + 1 lengths of values, then tries + 1 of the tries' keys; scanned in place
    uint32_t* seg_first;  // tries + 1
    uint32_t* key_off;
    uint64_t* val_off;
    uint8_t *keys, *vals;
    uint64_t key_cap, val_cap;
    uint32_t scan_n;  // (host side) the entries of len, and the scan's scratch
    uint32_t* scan;

    void size(uint32_t total_, uint32_t tries_, uint64_t val_bytes) {
        total = total_, tries = tries_, scan_n = total + 1u + tries + 1u;
        key_cap = (uint64_t)key_bytes_before(total) + 16u, val_cap = val_bytes;
    }
    template <class IO>
    void carve(IO& io) {
        len = io.template take<uint32_t>((size_t)scan_n + 4);
        scan = io.template take<uint32_t>(scan_scratch_entries(scan_n));
        seg_first = io.template take<uint32_t>((size_t)tries + 1);
        key_off = io.template take<uint32_t>((size_t)total + 1);
        val_off = io.template take<uint64_t>((size_t)total + 1);
        keys = io.template take<uint8_t>((size_t)key_cap);
        vals = io.template take<uint8_t>((size_t)val_cap + 16);
    }
    TriePairs trie_pairs(uint8_t* roots) const { return TriePairs{keys, key_off, key_cap, vals, val_off, val_cap, total, seg_first, tries, roots}; }
};

template <class Src>
__global__ void __launch_bounds__(256) forest_len_kernel(Src s, IndexForest a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total + 1u + a.tries) return;
    uint32_t v = 0;
    if (g < a.total) {
        v = (uint32_t)s.item(g).len;  // (checked: below 4 GiB)
    } else if (g > a.total) {
        const uint32_t t = g - a.total - 1u;
        uint32_t count = 0;  // (the entry behind the last trie: no keys)
        a.seg_first[t] = t == a.tries ? a.total : s.trie(t, count);
        v = key_bytes_before(count);
    }
    a.len[g] = v;
}

// len scanned: S[g] = the bytes of the values in front of g; S[total] = S[total + 1] = all of them; S[total + 1 + t] - S[total] = the bytes
// of the keys of the tries in front of t (modulo 2^32, which the difference undoes)
template <class Src>
__global__ void __launch_bounds__(256) forest_pairs_kernel(Src s, IndexForest a) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (g > a.total) return;
    const uint32_t all = a.len[a.total];
    if (g == a.total) {
        if (lane == 0u) a.val_off[g] = all, a.key_off[g] = a.len[a.total + 1u + a.tries] - all;
        return;
    }
    const auto it = s.item(g);
    const uint32_t at = a.len[g], ko = a.len[a.total + 1u + it.trie] - all + key_bytes_before(it.pos);
    if ((uint64_t)ko + 5u > a.key_cap || (uint64_t)at + it.len > a.val_cap) return;  // (cannot happen: both arrays are sized from the same rules)
    if (lane == 0u) {
        a.val_off[g] = at, a.key_off[g] = ko;
        (void)put_uint(a.keys + ko, it.index);
    }
    s.write(a.vals + at, it, lane);
}

// lengths, one scan, pairs: three launches
template <class Src>
hipError_t launch_forest(const Src& s, const IndexForest& a, hipStream_t st) {
    hipLaunchKernelGGL(forest_len_kernel<Src>, dim3(blocks_of(a.scan_n, 256)), dim3(256), 0, st, s, a);
    if (const hipError_t e = hipGetLastError()) return e;
    if (const hipError_t e = launch_exclusive_scan_u32(a.len, a.scan_n, a.scan, st)) return e;
    hipLaunchKernelGGL(forest_pairs_kernel<Src>, dim3(blocks_of((uint64_t)a.total + 1, 4)), dim3(256), 0, st, s, a);
    return hipGetLastError();
}

}  // namespace seg
}  // namespace phant
