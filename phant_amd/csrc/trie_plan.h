// trie_plan.h -- what the trie hasher's launcher (trie_build.hip: forest_device, small_forest) chooses, as plain host C++: its
// constants, the diagnostic knobs resolved once, the min-tree's level sizes, the pass, whether the leaves go ahead of the host's
// sizing, the sizes of the t2 arena's tables and every depth bin's launch.  No HIP call and no device code: the driver asks the
// runtime and launches what this says; tests/native/trie_plan_main.cpp holds every rule to literals.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "arena.h"  // TrieTune

namespace phant {

constexpr uint32_t FAN = 16;   // fan-out of the min-tree: a group of children is one 64-byte line
constexpr int MAX_LEVELS = 8;  // 16^8 boundaries
// absorb.hip.h's RATE / RATE_DWORDS (this header stays free of device code; trie_build.hip asserts that the two agree)
constexpr uint32_t PLAN_RATE = 136, PLAN_RATE_DWORDS = 34;
constexpr uint32_t LEAF_STAGE_DW = PLAN_RATE_DWORDS + 1u;  // 35 (odd): one rate block of LDS per lane (a state-trie leaf is ~112 bytes)

constexpr uint32_t CROWDED_BIN = 4u * 256u * 64u;  // nodes: above it a bin in four-block slots (one wave per SIMD) no longer fits the chip at once
// One wave per workgroup: the LDS slot of a lane holds four rate blocks (a full 17-item branch is 532 bytes).
constexpr uint32_t BRANCH_LANES = 64;
constexpr uint32_t BRANCH_STAGE_BLOCKS = 4;
// bins of at most COOP_MAX_NODES nodes (two waves per SIMD) give a node half a wave (branch_coop_kernel) ...
constexpr uint32_t COOP_MAX_NODES = 4096;  // (512 / 2 048 / 4 096 / 8 192 measured: 10 000 keys 0.288 / 0.267 / 0.247 / 0.250 ms, a million 0.669 / 0.663 / 0.651 / 0.654)
// ... and of up to WAVE_MAX_NODES a whole one (branch_wave_kernel)
constexpr uint32_t WAVE_MAX_NODES = 2048;

constexpr uint32_t SMALL_MAX_KEYS = 4096;   // (what the first kernel's LDS holds)
constexpr uint32_t SMALL_SURE_KEYS = 2048;  // up to here whatever the leaves are; beyond, where the mean value is a rate block or more
constexpr uint32_t SMALL_MAX_WGS = 512;
constexpr uint32_t SMALL_LCP_INTS = (SMALL_MAX_KEYS + 1u + FAN - 1u) / FAN * FAN + 512u;  // level 0 + the levels above it (272 + 32 + 16 at the most) + slack

// Up to this many keys the slot tables and the scratch blob are sized for the worst case (a branch node per key: 1.3 KB per key against
// ~0.45 KB for uniformly spread keys -- 10.6 GB at the limit) so that the leaves need not wait for the host to learn the node count.
constexpr uint64_t LEAVES_AHEAD_MAX_KEYS = 8u << 20;
constexpr uint32_t SIDE_MIN_KEYS = 400000;  // below it the leaves are too few to hide the deepest bins behind (200 000 keys: 0.497 vs 0.491 ms without)
constexpr uint32_t SIDE_LEAF_LDS = 20480;   // bytes of unused dynamic LDS per leaf workgroup meanwhile: TWO of them per CU instead of four (with three,
                                            // 5 or 6 KB, the bins beside them still starved: 146-162 us for a bin of 116 nodes)
constexpr uint32_t FALLBACK_GRID = 1024;    // workgroups of a bin's fallback pass (its count is on the device)

// ---- the knobs (arena.h: TrieTune), resolved once a call ----
struct TrieChoices {
    uint32_t side_min;       // the deepest bins may run beside the leaves from this many keys on
    uint64_t ahead_max;      // the leaves are queued ahead of the host's sizing up to this many keys
    uint32_t side_lds;       // idle dynamic LDS of the bulk leaf kernel while bins may run beside it
    uint32_t fallback_grid;  // workgroups of a bin's fallback pass at the most
    uint32_t coop_max;       // thin bins: up to this many nodes
    int32_t force_blocks;    // != 0: no thin-bin kernels; 1 / 2 / 4: every bin in slots of this many rate blocks
    bool no_coop, no_wave, no_side, join_in_stream;
    int64_t small_max;       // < 0: the library's own rule for the small pass
};
inline TrieChoices resolve_choices(const TrieTune& k) {
    TrieChoices c;
    c.side_min = k.side_min_keys >= 0 ? (uint32_t)std::min<int64_t>(k.side_min_keys, 0xffffffffll) : SIDE_MIN_KEYS;
    c.ahead_max = k.ahead_max_keys >= 0 ? (uint64_t)k.ahead_max_keys : LEAVES_AHEAD_MAX_KEYS;
    // (a leaf workgroup's static LDS + this must stay within the 64 KiB a launch gets without opting in)
    c.side_lds = k.side_lds >= 0 ? (uint32_t)std::min<int64_t>(k.side_lds, 65536 - 4 * 256 * (int)LEAF_STAGE_DW) : SIDE_LEAF_LDS;
    c.fallback_grid = k.fallback_grid >= 1 ? (uint32_t)std::min<int64_t>(k.fallback_grid, 1 << 20) : FALLBACK_GRID;
    c.coop_max = k.coop_max >= 0 ? (uint32_t)std::min<int64_t>(k.coop_max, 1 << 20) : COOP_MAX_NODES;
    c.force_blocks = k.slot_blocks;
    c.no_coop = k.no_coop;
    c.no_wave = k.no_wave;  // (A/B: the half-wave kernel for every thin bin)
    c.no_side = k.no_side;
    c.join_in_stream = k.join_in_stream;  // (A/B)
    c.small_max = k.small_max_keys;
    return c;
}

// ---- the min-tree's levels: level 0 = the n + 1 lcp values, every level padded to whole groups, the top level ONE group ----
struct TreeLevels {
    uint32_t size[MAX_LEVELS], off[MAX_LEVELS], n_lvl;  // level k >= 1 at tree + off[k]
    size_t tree_ints;                                   // of the levels above level 0 together
};
inline TreeLevels tree_levels(uint32_t n) {
    auto pad = [](uint64_t v) { return (uint32_t)((v + FAN - 1u) / FAN * FAN); };
    TreeLevels l{};
    l.size[0] = pad((uint64_t)n + 1);
    l.n_lvl = 1;
    while (l.size[l.n_lvl - 1u] > FAN) {
        l.size[l.n_lvl] = pad(l.size[l.n_lvl - 1u] / FAN);
        l.off[l.n_lvl] = (uint32_t)l.tree_ints;
        l.tree_ints += l.size[l.n_lvl];
        ++l.n_lvl;
    }
    return l;
}

// ---- the pass: the two launches of small_head_kernel / small_climb_kernel, or the general one ----
// Measured (profiles/r6_explore/NOTES.md section 3): one-block leaves (a state trie's) -- the two passes level at 2 048 keys, the
// general one ahead beyond (0.19 against 0.30 ms at 4 096); a block's lists (values of 50 .. 700 bytes: several permutations a
// leaf, which a wave's sponge runs at twice a lane's pace) -- ahead up to 3 x 1 000 items, level at 3 x 1 400.
inline bool small_pass(uint32_t n, uint64_t val_bytes, const TreeLevels& l, const TrieChoices& c) {
    const bool fits = n <= SMALL_MAX_KEYS && (size_t)l.size[0] + l.tree_ints + FAN <= SMALL_LCP_INTS;  // (the first kernel's LDS)
    if (c.small_max >= 0) return fits && n <= (uint64_t)c.small_max;
    return fits && (n <= SMALL_SURE_KEYS || val_bytes >= (uint64_t)PLAN_RATE * n);
}
inline uint32_t small_climb_grid(uint32_t n) { return std::max(1u, std::min(SMALL_MAX_WGS, (n + 3u) / 4u)); }

// ---- the t2 arena: slot tables by dense node id (16 x 32 bytes a node) + the scratch blob of the nodes that take the general way ----
inline uint64_t slot_table_bytes(uint64_t nodes) { return nodes * 16 * 32; }
// leaves: list hdr (<=9) + HP (<= 3 + key bytes + 1) + value (<= 9 + len), 4-byte rounded -- 32 a key beside its bytes;
// branches: <= 3 + 16*33 + value (16); extensions <= 48 + key bytes / 2 (255 / 2), 16 of rounding
constexpr uint64_t SCRATCH_PER_KEY = 32, SCRATCH_PER_NODE = 3 + 16 * 33 + 16 + 48 + 255 / 2 + 16, SCRATCH_SLACK = 4096;
inline uint64_t scratch_bound(uint64_t nodes, uint64_t n, uint64_t key_bytes, uint64_t val_bytes) {
    return val_bytes + key_bytes + n * SCRATCH_PER_KEY + nodes * SCRATCH_PER_NODE + SCRATCH_SLACK;
}

// ---- leaves ahead: the tables sized for a node per key (a node has two children at least), the bulk of the leaves queued behind
// order_kernel at once -- else from the node count the mailbox brings, the leaves after it ----
// what the worst-case tables take (the decision has always counted them without the blob's slack)
inline uint64_t ahead_need(uint64_t n, uint64_t key_bytes, uint64_t val_bytes) {
    return slot_table_bytes(n) + scratch_bound(n, n, key_bytes, val_bytes) - SCRATCH_SLACK;
}
// The worst-case tables are ~3 x what the trie will need (1.3 KB against ~0.45 KB per key).  Where that much is not to be had -- torch
// sharing the device, several ctxs or slots -- the call falls back to what it did before the leaves went ahead.  The driver asks the
// runtime for the free bytes only where ask_free_bytes says so; free_known: it did, and got an answer.
inline bool ask_free_bytes(uint64_t n, uint64_t need, uint64_t t2_cap, const TrieChoices& c) { return n <= c.ahead_max && need > t2_cap; }
inline bool leaves_ahead(uint64_t n, uint64_t need, uint64_t t2_cap, bool free_known, uint64_t free_bytes, const TrieChoices& c) {
    if (n > c.ahead_max) return false;
    return !(need > t2_cap && free_known && need > free_bytes + t2_cap);
}

// ---- the helper stream: order_kernel may send the deepest bins there (deep_from, through the mailbox; < 0: it did not) ----
inline bool side_ok(uint32_t n, const TrieChoices& c) { return !c.no_side && n >= c.side_min; }
inline bool bin_on_side(int depth, int deep_from) { return deep_from >= 0 && depth >= deep_from; }

// ---- a bin's launch ----
// cls (TrieStats::by_class): a wave per node, a node per half wave, a lane per node in 1- / 2- / 4-block slots
enum : uint32_t { BIN_WAVE = 0, BIN_HALF_WAVE = 1, BIN_BLOCKS1 = 2, BIN_BLOCKS2 = 3, BIN_BLOCKS4 = 4 };
struct BinLaunch {
    uint32_t cls;
    uint32_t slot_blocks;      // 0 for the thin-bin kernels
    uint32_t grid, block;      // the main launch
    uint32_t fb_grid, fb_block;  // the four-block pass over what did not fit, behind it (fb_grid 0: none)
};
inline BinLaunch plan_bin(uint32_t c, uint64_t children, const TrieChoices& ch) {
    if (c <= ch.coop_max && !ch.no_coop && !ch.force_blocks) {
        // (the sponge's fetches share the CU's LDS pipeline: with one wave on a CU a permutation takes 4.9 us, with four 5.7 --
        // up to two waves per CU the workgroups are single waves, which the dispatcher spreads over the CUs)
        if (c <= WAVE_MAX_NODES && !ch.no_wave) return c <= 512u ? BinLaunch{BIN_WAVE, 0, c, 64, 0, 0} : BinLaunch{BIN_WAVE, 0, (c + 3u) / 4u, 256, 0, 0};
        return c <= 1024u ? BinLaunch{BIN_HALF_WAVE, 0, (c + 1u) / 2u, 64, 0, 0} : BinLaunch{BIN_HALF_WAVE, 0, (c + 7u) / 8u, 256, 0, 0};
    }
    // A bin's slot class (branch_kernel): four blocks unless the bin is crowded (more workgroups than the chip holds at once) and
    // its mean fan-out says that most of its nodes fit less; what does not fit is run through the four-block class behind it.
    uint32_t blocks = BRANCH_STAGE_BLOCKS;
    if (c >= CROWDED_BIN) {
        if (children <= 3ull * c) blocks = 1;       // (<= 3 children of 33 bytes: one rate block)
        else if (children <= 6ull * c) blocks = 2;  // (<= 7: two)
    }
    if (ch.force_blocks == 1 || ch.force_blocks == 2 || ch.force_blocks == 4) blocks = (uint32_t)ch.force_blocks;
    const uint32_t waves = (c + BRANCH_LANES - 1u) / BRANCH_LANES;
    if (blocks == BRANCH_STAGE_BLOCKS) return BinLaunch{BIN_BLOCKS4, blocks, waves, BRANCH_LANES, 0, 0};
    const uint32_t lanes = 256u / blocks;
    return BinLaunch{blocks == 1 ? BIN_BLOCKS1 : BIN_BLOCKS2, blocks, (c + lanes - 1u) / lanes, lanes, std::min(waves, ch.fallback_grid), BRANCH_LANES};
}

}  // namespace phant
