// verify_hash.hip.h -- what the verify pipelines share on the device: the rate-block classes of the hash lists, unaligned loads,
// the canonical-full-branch check done on a rate block while it is in registers, and the three ways a lane hashes a node
// (exactly 532 bytes, one wave-uniform length below the rate, anything).  Used by mpt_verify_v3.hip (a proof per key) and
// mpt_verify_nodeset.hip (a node SET per witness).
//
// What it computes: Keccak-256 (src/crypto/hasher.zig:4-8) over the node encodings of src/mpt/mpt.zig:187-193,216-231,254-261.
#pragma once
#include <phant_platform.h>

#include "absorb.hip.h"

namespace phant {
namespace vh {

constexpr uint32_t N_CLASS = 8;        // class c = (c+1) rate blocks; last class = 8 or more
constexpr uint32_t LIST_B532 = 8;      // list of the nodes that are exactly 532 bytes long
constexpr uint32_t N_LIST = 9;
constexpr uint32_t CLASS_NONE = 0xffu;
constexpr uint32_t STRIPES = 8;        // every class list is kept as STRIPES sub-lists (workgroup b appends to b mod STRIPES):
                                       // returning atomics on ONE address are served one at a time, ~11.6 ns each
                                       // (tools/ubench/atomic_rate.hip) -- thousands of workgroups on one cursor are tens of us
constexpr uint32_t MAX_SHALLOW = 16;   // key prefix of <= 16 nibbles fits 64 bits
constexpr uint32_t STATUS_NEEDS_SLOW = 0xffu;
constexpr uint32_t BRANCH_LEN = 532u;  // f9 02 11 | 16 x (a0 + 32 bytes) | 80


// nstat[] bits
constexpr uint32_t NS_HASHED = 1u, NS_CANON = 2u, NS_LINK_CHECKED = 4u, NS_LINK_OK = 8u;
constexpr uint32_t NS_LAST = 16u;  // the proof's last node, and the lane that hashed it left what it decodes to in last[proof]

PHANT_DEV uint32_t node_list(uint32_t len) {
    if (len == BRANCH_LEN) return LIST_B532;
    const uint32_t nb = len / RATE + 1u;
    return (nb > N_CLASS ? N_CLASS : nb) - 1u;
}

struct __attribute__((packed, aligned(1))) U32x4 { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(1))) U32x3 { uint32_t x, y, z; };
struct __attribute__((packed, aligned(1))) U32x2 { uint32_t x, y; };
struct __attribute__((packed, aligned(1))) U32x1 { uint32_t x; };
PHANT_DEV uint4 load16u(const uint8_t* p) {  // unaligned 16-byte global load
    const U32x4 v = *reinterpret_cast<const U32x4*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
PHANT_DEV uint32_t load4u(const uint8_t* p) { return reinterpret_cast<const U32x1*>(p)->x; }
// value of `v` in lane `i` (wave-uniform i).  The builtin returns int: without the cast a 64-bit
// offset assembled from two halves gets its low half sign-extended (wrong for blobs > 2 GiB).
PHANT_DEV uint32_t lane_u32(uint32_t v, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane(v, i); }
PHANT_DEV uint64_t lane_u64(uint32_t lo, uint32_t hi, uint32_t i) {
    return ((uint64_t)lane_u32(hi, i) << 32) | (uint64_t)lane_u32(lo, i);
}

// ---------------------------------------------------------------- canonical full branch, per rate block
// f9 02 11 | 16 x (a0 + 32 bytes) | 80 = 532 bytes: what the marker bytes of rate block K (bytes
// [136 K, 136 K + 136) of the node, as 34 little-endian dwords) must be.  The hash waves hold exactly
// these dwords in registers when they absorb the block, so checking the form of a node there costs ~10
// VALU operations per block and no memory traffic.
struct BranchMask {
    uint32_t m[4][RATE_DWORDS];
    uint32_t v[4][RATE_DWORDS];
};
constexpr BranchMask make_branch_mask() {
    BranchMask r{};
    for (uint32_t q = 0; q < BRANCH_LEN; ++q) {
        int want = -1;
        if (q == 0) want = 0xf9;
        else if (q == 1) want = 0x02;
        else if (q == 2) want = 0x11;
        else if (q == BRANCH_LEN - 1u) want = 0x80;
        else if ((q - 3u) % 33u == 0u) want = 0xa0;
        if (want >= 0) {
            const uint32_t k = q / RATE, i = (q % RATE) / 4u, sh = 8u * (q % 4u);
            r.m[k][i] |= 0xffu << sh;
            r.v[k][i] |= (uint32_t)want << sh;
        }
    }
    return r;
}
constexpr BranchMask BRANCH_MASK = make_branch_mask();

template <int K, int NDW>
PHANT_DEV uint32_t branch_block_bad_k(const uint32_t (&d)[RATE_DWORDS]) {
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < NDW; ++i) {
        if (BRANCH_MASK.m[K][i] != 0u) bad |= (d[i] ^ BRANCH_MASK.v[K][i]) & BRANCH_MASK.m[K][i];
    }
    return bad;
}

// One rate block of a 532-byte node into the sponge: K = which block (0..3), NDW = its message dwords (34, or 31 for
// the last block: 124 message bytes, then the padding -- two constants, nothing masked per lane, nothing read beyond
// the node's last byte).  Returns nonzero iff the block contradicts the canonical full branch.
template <int K, int NDW>
PHANT_DEV uint32_t absorb_b532_block(Sponge& s, const uint8_t* __restrict__ p) {
    uint32_t d[RATE_DWORDS];
    if constexpr (NDW == 34) {
        load_block_wide(d, p);
    } else {
        static_assert(NDW == 31, "last block of a 532-byte node: 124 message bytes");
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const uint4 v = load16u(p + 16 * c);
            d[4 * c] = v.x;
            d[4 * c + 1] = v.y;
            d[4 * c + 2] = v.z;
            d[4 * c + 3] = v.w;
        }
        const U32x3 t = *reinterpret_cast<const U32x3*>(p + 112);
        d[28] = t.x;
        d[29] = t.y;
        d[30] = t.z;
        d[31] = 0x00000001u;  // pad 0x01 right behind the 124 message bytes
        d[32] = 0u;
        d[33] = 0x80000000u;  // ... 0x80 in the last byte of the rate
    }
    const uint32_t bad = branch_block_bad_k<K, NDW>(d);
    xor_block(s, d);
    return bad;
}

// Keccak-256 of a node that is exactly 532 bytes long, for every lane of the wave (wave-uniform: all active lanes
// have such a node; inactive lanes hash whatever `ptr` points at -- the launcher gives them a readable one).  Returns
// nonzero iff the node is NOT the canonical full branch.
// LADDER: the wave's issue priority falls as it gets on (2, 1, 1, 0 over the four blocks: below the memory-bound kernels' 3
// throughout).  VALU issue on a SIMD is arbitrated by priority, then age -- left alone, the oldest of four co-resident
// hash waves takes ~60 % of the slots, finishes first, and the youngest ends up running its last permutations alone at
// single-wave speed.  With the ladder a wave that is behind outranks the ones ahead: they advance block by block
// together and finish together (profiles/EXPERIMENTS.md: ladders measured).
template <bool LADDER>
PHANT_DEV uint32_t hash_b532(Sponge& s, const uint8_t* __restrict__ p) {
    sponge_zero(s);
    if (LADDER) __builtin_amdgcn_s_setprio(2);
    uint32_t bad = absorb_b532_block<0, 34>(s, p);
    keccak_f1600(s);
    if (LADDER) __builtin_amdgcn_s_setprio(1);
    bad |= absorb_b532_block<1, 34>(s, p + RATE);
    keccak_f1600(s);
    if (LADDER) __builtin_amdgcn_s_setprio(1);
    bad |= absorb_b532_block<2, 34>(s, p + 2u * RATE);
    keccak_f1600(s);
    if (LADDER) __builtin_amdgcn_s_setprio(0);
    bad |= absorb_b532_block<3, 31>(s, p + 3u * RATE);
    keccak_f1600(s);
    return bad;
}

// The same with every rate block requested a permutation AHEAD, into registers: the 34 dwords of block k + 1 are in flight while
// block k is permuted (the permutation does not touch them), so a wave never waits for memory between two permutations -- and the
// waves of a SIMD, which advance block by block together, never all wait at once.  Costs 34 VGPRs held across the permutation
// (~150 instead of ~115: three hash waves per SIMD instead of four; two already issue at the full VALU rate).
PHANT_DEV void load_b532_block(uint32_t (&d)[RATE_DWORDS], const uint8_t* __restrict__ p, const bool last) {
    if (!last) {
        load_block_wide(d, p);
    } else {  // 124 message bytes, then the padding: nothing read beyond the node's last byte
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const uint4 v = load16u(p + 16 * c);
            d[4 * c] = v.x;
            d[4 * c + 1] = v.y;
            d[4 * c + 2] = v.z;
            d[4 * c + 3] = v.w;
        }
        const U32x3 t = *reinterpret_cast<const U32x3*>(p + 112);
        d[28] = t.x;
        d[29] = t.y;
        d[30] = t.z;
        d[31] = 0x00000001u;
        d[32] = 0u;
        d[33] = 0x80000000u;
    }
}
PHANT_DEV uint32_t hash_b532_ahead(Sponge& s, const uint8_t* __restrict__ p) {
    sponge_zero(s);
    uint32_t d0[RATE_DWORDS], d1[RATE_DWORDS];
    load_b532_block(d0, p, false);
    load_b532_block(d1, p + RATE, false);
    uint32_t bad = branch_block_bad_k<0, 34>(d0);
    xor_block(s, d0);
    keccak_f1600(s);
    load_b532_block(d0, p + 2u * RATE, false);
    bad |= branch_block_bad_k<1, 34>(d1);
    xor_block(s, d1);
    keccak_f1600(s);
    load_b532_block(d1, p + 3u * RATE, true);
    bad |= branch_block_bad_k<2, 34>(d0);
    xor_block(s, d0);
    keccak_f1600(s);
    bad |= branch_block_bad_k<3, 31>(d1);
    xor_block(s, d1);
    keccak_f1600(s);
    return bad;
}

// Keccak-256 of one node per lane, any lengths (exec-masked loop: the wave runs as many permutations as its longest
// node needs).  `safe_end`: one past the last byte of the node blob.
PHANT_DEV void hash_any(Sponge& s, const uint8_t* __restrict__ p, uint32_t len, const uint8_t* __restrict__ safe_end) {
    sponge_zero(s);
    uint32_t left = len;
    while (left >= RATE) {
        absorb_full_block_wide(s, p);
        keccak_f1600(s);
        p += RATE;
        left -= RATE;
    }
    if (p + RATE <= safe_end) {
        uint32_t d[RATE_DWORDS];
        load_block_wide(d, p);  // the whole window; bytes past the node are masked off
        absorb_loaded_final(s, d, left);
    } else {  // last node of the blob: narrow loads that never leave the message
        const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
        absorb_final_block(s, reinterpret_cast<const uint32_t*>(p - sh), sh, left);
    }
    keccak_f1600(s);
}

// Keccak-256 of one node per lane where every lane's node has the SAME length `len` < 136 (wave-uniform): the
// padding masks are scalars.
PHANT_DEV void short_uniform_fill(Sponge& s, const uint32_t (&d)[RATE_DWORDS], uint32_t len /* wave-uniform */) {
#pragma unroll
    for (int i = 0; i < (int)RATE_DWORDS; ++i) {
        const int m = (int)len - 4 * i;  // message bytes inside this dword (scalar)
        const uint32_t t = 1u << ((m & 3) * 8);
        const uint32_t keep = m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : t - 1u);
        uint32_t pad = (m >= 0 && m < 4) ? t : 0u;
        if (i == (int)RATE_DWORDS - 1) pad ^= 0x80000000u;
        const uint32_t v = (d[i] & keep) ^ pad;
        if (i & 1) s.hi[i >> 1] = v;
        else s.lo[i >> 1] = v;
    }
}
PHANT_DEV void hash_short_uniform(Sponge& s, const uint8_t* __restrict__ p, uint32_t len /* wave-uniform */) {
    sponge_zero(s);
    uint32_t d[RATE_DWORDS];
    load_block_wide(d, p);
    short_uniform_fill(s, d, len);
    keccak_f1600(s);
}

// ---------------------------------------------------------------- a proof's last node, decoded where it is hashed
// What the walk would find out about the last node of a proof -- for BASELINE's proofs the 112-byte account leaf -- by copying
// it into LDS and running the generic decoder over the copy (mpt_walk.hip.h: walk_node) is settled by the lane that hashes the
// node, from the dwords it has loaded for the sponge: one 64-bit word per proof, last[proof].
//   bits [0, 40)  byte offset of the value inside the node blob (PRESENT)
//   bits [40, 48) its length
//   bits [48, 62) key nibbles consumed in front of the node: the node's index in its proof
//   bits [62, 64) LAST_NONE (nothing decoded: the walk decodes the node itself), LAST_PRESENT, LAST_ABSENT
constexpr uint32_t LAST_NONE = 0u, LAST_PRESENT = 1u, LAST_ABSENT = 2u;
constexpr uint32_t LAST_POS_MAX = (1u << 14) - 1u;
PHANT_DEV uint32_t last_code(uint64_t w) { return (uint32_t)(w >> 62); }
PHANT_DEV uint32_t last_pos(uint64_t w) { return (uint32_t)(w >> 48) & LAST_POS_MAX; }
PHANT_DEV uint32_t last_value_len(uint64_t w) { return (uint32_t)(w >> 40) & 0xffu; }
PHANT_DEV uint64_t last_value_off(uint64_t w) { return w & ((1ull << 40) - 1ull); }

// The node of `len` bytes (wave-uniform, below the rate) whose rate-block window is in d, at byte `at` of the blob, for the key
// `key` of which `pos` nibbles (wave-uniform) are consumed.  Decoded are exactly the nodes walk_node settles as a leaf:
//   the list header is canonical and spans the node (its form follows from `len`: a scalar comparison);
//   item 0 is a canonical string of 1..33 bytes (so item 1 starts at byte 36 at the latest: ten dwords to select from);
//   hex-prefix flag 2 or 3, an even flag with a zero pad nibble;
//   item 1 is a canonical string -- not a list -- that ends the list;
//   the path is byte-aligned with the key at `pos`: flag 3 for an odd `pos`, flag 2 for an even one.
// PRESENT iff the path is the rest of the key (walk_node: plen == nn - pos and the bytes equal -- with the path that long its
// bytes start at byte 2 + header of the node and there are key_len - ceil(pos / 2) of them: scalars), ABSENT otherwise.
// Everything else -- extensions, branches, embedded or malformed nodes, a path that is not byte-aligned -- is LAST_NONE.
// No byte of the node at or behind `len` decides anything.
PHANT_DEV uint64_t decode_last_leaf(const uint32_t (&d)[RATE_DWORDS], const uint32_t len, const uint8_t* __restrict__ key,
                                    const uint32_t key_len, const uint32_t pos, const uint64_t at) {
    const uint32_t nn = 2u * key_len;
    if (pos > nn || pos > LAST_POS_MAX) return 0ull;
    uint32_t hp;  // bytes of the list header
    bool ok;
    if (len >= 3u && len <= 56u) {
        hp = 1u;
        ok = (d[0] & 0xffu) == 0xc0u + (len - 1u);
    } else if (len >= 58u && len < RATE) {
        hp = 2u;
        ok = (d[0] & 0xffffu) == (0xf8u | ((len - 2u) << 8));
    } else {
        return 0ull;
    }
    ok = ok && (at >> 39) == 0ull;
    // item 0: the hex-prefix path
    const uint32_t h0 = (d[0] >> (8u * hp)) & 0xffu, n0 = (d[0] >> (8u * hp + 8u)) & 0xffu;
    const bool single0 = h0 < 0x80u;
    const uint32_t l0 = single0 ? 1u : h0 - 0x80u;
    const uint32_t b0 = single0 ? h0 : n0;
    const uint32_t o1 = hp + (single0 ? 1u : 1u + l0);  // where item 1 starts
    ok = ok && l0 >= 1u && l0 <= 33u && (single0 || l0 != 1u || n0 >= 0x80u) && o1 < len;
    const uint32_t odd = pos & 1u;
    ok = ok && (b0 >> 4) == 2u + odd && (odd != 0u || (b0 & 0x0fu) == 0u);
    // item 1: the value.  Its header byte and the byte behind it, out of the dwords that can hold them
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 10u; ++i) {
        const bool here = (o1 >> 2) == i;
        lo = here ? d[i] : lo;
        hi = here ? d[i + 1u] : hi;
    }
    const uint32_t w1 = alignbyte(hi, lo, o1 & 3u);
    const uint32_t h1 = w1 & 0xffu, n1 = (w1 >> 8) & 0xffu;
    uint32_t l1, p1;
    if (h1 < 0x80u) {
        l1 = 1u;
        p1 = o1;
    } else if (h1 <= 0xb7u) {
        l1 = h1 - 0x80u;
        p1 = o1 + 1u;
        ok = ok && (l1 != 1u || n1 >= 0x80u);
    } else {
        l1 = n1;
        p1 = o1 + 2u;
        ok = ok && h1 == 0xb8u && n1 >= 56u;
    }
    ok = ok && p1 + l1 == len;  // (with it the byte behind the header, where it was looked at, is the node's)
    if (!ok) return 0ull;
    // the path against the rest of the key
    const uint32_t plen = 2u * (l0 - 1u) + odd;
    const uint32_t kb = (pos + odd) >> 1, nk = key_len - kb;  // the key bytes behind the nibble an odd path starts with
    bool present = plen == nn - pos && nk <= 32u;
    if (present) {
        uint32_t diff = odd ? ((b0 ^ key[pos >> 1]) & 0x0fu) : 0u;
        // (one address in a register pair and constant offsets from it: left to itself the compiler keeps a scalar base per load,
        // all of them computed in front of the caller's loop and held across its sponges)
        const uint8_t* kp = key + kb;
        PHANT_PIN_VGPR(kp);
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) {
            if (4u * t < nk) {  // (wave-uniform)
                const uint32_t m = nk - 4u * t;  // key bytes left
                const uint32_t nw = hp == 2u ? d[1u + t] : alignbyte(d[t + 1u], d[t], 3u);  // node bytes [hp + 2 + 4 t, + 4)
                uint32_t kw = 0u;
                if (m >= 4u) {
                    kw = load4u(kp + 4u * t);
                } else {
                    for (uint32_t q = 0; q < m; ++q) kw |= (uint32_t)kp[4u * t + q] << (8u * q);
                }
                diff |= (nw ^ kw) & (m >= 4u ? 0xffffffffu : (1u << (8u * m)) - 1u);
            }
        }
        present = diff == 0u;
    }
    const uint64_t code = present ? LAST_PRESENT : LAST_ABSENT;
    const uint64_t value = present ? (at + p1) | ((uint64_t)l1 << 40) : 0ull;
    return (code << 62) | ((uint64_t)pos << 48) | value;
}

// hash_short_uniform for a wave some of whose lanes (`is_last`) hold their proof's last node: those decode it from the loaded
// dwords and store the word at `rec` before the permutation (nothing of it has to outlive the sponge but "a result is there").
PHANT_DEV bool hash_short_uniform_last(Sponge& s, const uint8_t* __restrict__ p, uint32_t len /* wave-uniform */, const bool is_last,
                                       uint64_t* __restrict__ rec, const uint8_t* __restrict__ key, const uint32_t key_len,
                                       const uint32_t pos /* wave-uniform */, const uint64_t at) {
    sponge_zero(s);
    uint32_t d[RATE_DWORDS];
    load_block_wide(d, p);
    bool decoded = false;
    if (is_last) {
        const uint64_t w = decode_last_leaf(d, len, key, key_len, pos, at);
        *rec = w;
        decoded = last_code(w) != LAST_NONE;
    }
    short_uniform_fill(s, d, len);
    keccak_f1600(s);
    return decoded;
}

// ---------------------------------------------------------------- the queue of list chunks
// Wave q hashes chunk q (64 nodes of one list) and exits; the grid covers the queue and the dispatcher keeps every
// SIMD full (the per-proof pipeline sizes its grid for the queue a well-formed witness leaves, and a wave comes back for
// chunk q + the grid's waves where the queue is longer: mpt_verify_v3.hip).  A short last chunk repeats its last node
// (same results stored twice) so that no lane is ever idle-masked.
// The chunk queue is the concatenation of the lists in this order: classes by falling rate-block count -- 8+ blocks, 7, 6,
// 5, [532-byte list], 4 (others), 3, 2, 1 --, inside a class the stripes.
constexpr uint32_t N_QUEUE = N_LIST * STRIPES;  // 72
PHANT_DEV uint32_t queue_class(uint32_t li) {
    const uint32_t o = li / STRIPES;
    return o < 4u ? 7u - o : (o == 4u ? LIST_B532 : 8u - o);
}
PHANT_DEV uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Nodes the generic decoder opens (for BASELINE's proofs: the 112-byte account leaf) are first copied
// into a per-lane LDS slot with 16-byte loads, together with the key: the RLP decoder and the path
// comparison read single bytes one after the other, and from HBM/L2 every one of those ~100 dependent
// reads cost a full cache round trip (the per-CU L1 does not hold 256 lanes' nodes).
constexpr uint32_t WALK_STAGE_BYTES = 192;  // nodes up to this size are staged; longer ones are read in place
constexpr uint32_t WALK_KEY_BYTES = 32;
constexpr uint32_t WALK_SLOT_DW = (WALK_STAGE_BYTES + WALK_KEY_BYTES) / 4 + 1;  // odd stride: no bank pile-up

}  // namespace vh
}  // namespace phant
