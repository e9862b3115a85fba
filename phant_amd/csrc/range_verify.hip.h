// range_verify.hip.h -- range proofs (phant_mpt_verify_ranges): is a sorted run of leaves exactly what the trie under a trusted root holds
// between an origin and the run's last key, and does anything lie to its right?  Included by mpt_verify_nodeset.hip behind
// poststate.hip.h: it resolves references through that file's record table and builds its tries with the post-state's item list
// (the contract is the comment above phant_mpt_verify_ranges in include/phant_gpu.h).
//
// Per range the item list is  [what the origin's path leaves to its LEFT]  [the caller's leaves]  [what the last key's path leaves to
// its RIGHT], all ranges of a call back to back, every range a trie of its own:
//
//   range_check_kernel      device form only: leaf_first / val_off / node_off as the contract asks (the host reads the verdict before
//                           any kernel indexes with them)
//   range_leaf_rule_kernel  a lane per leaf: the four leaf rules; the least bad leaf of a range by atomicMin (whatever order the lanes run in)
//   range_count_kernel / range_emit_kernel   a lane per leaf and two walker lanes per range (count, exclusive scan, write): the walkers are
//                           post::walk_emit with the rule SideRule below (left / right) -- the left one writes in path order, the right one from
//                           the back, so the concatenation IS the sorted list
//   post_link_kernel        (poststate.hip.h) a list out of order or not prefix-free is that range's mismatch
//   range_leaf_kernel       a lane per leaf item: its parent's depth is max(lcp with the predecessor, lcp with the successor), so the lane
//                           encodes rlp([hex-prefix(remaining nibbles), value]) in an LDS slot of its own, hashes it there and leaves a
//                           READY REFERENCE one nibble below its parent, which attach() copies -- the lane that builds the parent no longer
//                           hashes up to sixteen leaves one after the other
//   post_level_kernel x 64, post_root_kernel   (poststate.hip.h, launch_post_levels) ONE pass over all tries of the call
//   range_finish_kernel     a lane per range: the status in the contract's order, has_more, the computed root, the counts
//
// Soundness: as poststate.hip.h -- a byte of a built node is the caller's (a leaf) or comes from a node reached from the trusted root
// through references resolved by Keccak.  A reference of unknown type that the build would have to merge with nibbles above it is a
// mismatch of its range, never looked up.
//
// With PHANT_RANGE_RULES_ONLY defined only the rules are declared, without any HIP header: tests/native/ranges_main.cpp builds them as
// a program of its own.
#pragma once
#include <stdint.h>

#include "../../include/phant_gpu.h"

#ifdef PHANT_RANGE_RULES_ONLY
#define RANGE_HD inline
#else
#define RANGE_HD __host__ __device__ inline
#endif

namespace phant {
namespace range {

constexpr uint32_t NO_LEAF = 0xffffffffu;
constexpr uint32_t MAX_LEAF_VALUE = 560;  // post::MAX_VALUE (asserted below)

// -1 / 0 / 1: the 32-byte keys a and b in path order
RANGE_HD int cmp_keys(const uint8_t* a, const uint8_t* b) {
    for (uint32_t t = 0; t < 32u; ++t)
        if (a[t] != b[t]) return a[t] < b[t] ? -1 : 1;
    return 0;
}
// The rule a leaf breaks (0: none), in the contract's order.  prev: the key in front of it in its range (null: it is the first);
// origin: non-null only for the first leaf of a range with a proof.
RANGE_HD uint32_t leaf_rule(const uint8_t* key, uint64_t vlen, const uint8_t* prev, const uint8_t* origin) {
    if (vlen == 0u) return PHANT_RANGE_EMPTY_VALUE;
    if (vlen > MAX_LEAF_VALUE) return PHANT_RANGE_VALUE_TOO_LONG;
    if (prev && cmp_keys(key, prev) <= 0) return PHANT_RANGE_BAD_ORDER;
    if (origin && cmp_keys(key, origin) < 0) return PHANT_RANGE_BELOW_ORIGIN;
    return 0;
}
// What a walker emits next to its key's path.  LEFT: the origin's walker (everything in front of the origin).  RIGHT: the last key's
// (everything behind it).  At a branch at depth pos where the key has nibble nib: the slots [0, front_end) in path order and the slots
// [back_begin, back_end) from the back.
struct SideRule {
    bool right;
    RANGE_HD void slots(uint32_t /*pos*/, uint32_t nib, uint32_t& front_end, uint32_t& back_begin, uint32_t& back_end) const {
        front_end = right ? 0u : nib;
        back_begin = right ? nib + 1u : 16u;
        back_end = 16u;
    }
    // a leaf / an extension the walk diverges from: the left walker's when it sorts in front of the origin, the right walker's when it
    // sorts behind the last key; the other case lies inside the range, where the leaves must supply it
    template <class Cmp>
    RANGE_HD bool diverging(bool before, uint32_t /*pos*/, const Cmp& /*cmp*/) const {
        return before != right;
    }
};

}  // namespace range
}  // namespace phant

#ifndef PHANT_RANGE_RULES_ONLY
#include "launch.h"

namespace phant {
namespace range {

static_assert(MAX_LEAF_VALUE == post::MAX_VALUE, "the leaf rule refuses what the build cannot carry");

struct Args {
    RangeArgs r;
    post::Args b;  // the build: the item list, the record table
};

// the range lane x of the count / emit grid works for: per range r the lanes leaf_first[r] + 2r (the left walker), one per leaf, and
// leaf_first[r + 1] + 2r + 1 (the right walker)
PHANT_DEV uint32_t lane0_of(const RangeArgs& a, uint32_t r) { return a.leaf_first[r] + 2u * r; }
PHANT_DEV uint32_t range_of_lane(const RangeArgs& a, uint32_t x) {
    uint32_t lo = 0, hi = a.n_ranges;  // the last r with lane0_of(r) <= x
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (lane0_of(a, mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
PHANT_DEV uint32_t range_of_leaf(const RangeArgs& a, uint32_t j) {
    uint32_t lo = 0, hi = a.n_ranges;  // the last r with leaf_first[r] <= j (empty ranges in front of it share the value: the last wins)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.leaf_first[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}
PHANT_DEV uint32_t rule_at(const RangeArgs& a, uint32_t r, uint32_t j) {
    const uint32_t first = a.leaf_first[r];
    return leaf_rule(a.keys + 32ull * j, a.val_off[j + 1] - a.val_off[j], j > first ? a.keys + 32ull * (j - 1u) : nullptr,
                     j == first && a.has_proof[r] ? a.origins + 32ull * r : nullptr);
}

// ---------------------------------------------------------------- the device form's offsets
// ctl[RANGE_CTL_CHECK] != 0: refused.  Every entry is compared with its neighbour only; nothing is indexed with an entry's value.
__global__ void __launch_bounds__(256) range_check_kernel(const RangeArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (g <= a.n_ranges) {
        const uint32_t v = a.leaf_first[g];
        bad = bad || (g == 0u && v != 0u) || (g == a.n_ranges && v != a.n_leaves) || (g < a.n_ranges && a.leaf_first[g + 1] < v);
    }
    if (g <= a.n_leaves && a.val_off) {  // (null: no leaves, the caller has seen to that)
        const uint64_t v = a.val_off[g];
        bad = bad || (g == 0u && v != 0u) || (g == a.n_leaves && v != a.vals_len) || (g < a.n_leaves && a.val_off[g + 1] < v);
    }
    if (g <= a.n_nodes && a.node_off) {
        const uint64_t v = a.node_off[g];
        bad = bad || (g == 0u && v != 0u) || (g == a.n_nodes && v != a.nodes_len) || (g < a.n_nodes && a.node_off[g + 1] < v);
    }
    if (bad) atomicOr(&a.ctl[RANGE_CTL_CHECK], 1u);
}

// ---------------------------------------------------------------- the leaves' rules
__global__ void __launch_bounds__(256) range_leaf_rule_kernel(const RangeArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n_leaves) return;
    const uint32_t r = range_of_leaf(a, j);
    if (rule_at(a, r, j) != 0u) atomicMin(&a.bad_leaf[r], j);
}

// ---------------------------------------------------------------- count / emit
// lane x of the grid.  WRITE = false: only counts (and notes a walker's failure, and whether the right walker had anything).
PHANT_DEV uint32_t emit_lane(const Args& a, const uint32_t x, const bool write, const uint32_t base, const uint32_t count) {
    const RangeArgs& q = a.r;
    const uint32_t r = range_of_lane(q, x);
    if (q.bad_leaf[r] != NO_LEAF) return 0;  // a range whose leaves break a rule contributes nothing
    const uint32_t first = q.leaf_first[r], m = q.leaf_first[r + 1] - first, at = x - lane0_of(q, r);
    post::Item* const items = post::post_items(a.b.p);
    if (at >= 1u && at <= m) {  // a leaf, with the caller's value
        if (write && count == 1u) {
            const uint32_t j = first + at - 1u;
            post::Item* const it = items + base;
            for (uint32_t t = 0; t < 32u; ++t) it->path[t] = q.keys[32ull * j + t], it->ref[t] = 0u;
            it->src = q.val_off[j];
            it->vlen = (uint32_t)(q.val_off[j + 1] - q.val_off[j]);
            it->key = 1u;  // (the value lies in leaf_vals)
            it->trie = r;
            it->lcp = -1;
            it->nxt = 0;
            it->plen = 64;
            it->kind = post::IK_LEAF_OLD;
            it->reflen = 0;
            it->pad = 0;
        }
        return 1;
    }
    const bool right = at != 0u;
    if (!q.has_proof[r] || (right && m == 0u)) return 0;
    const uint8_t* const key = right ? q.keys + 32ull * (first + m - 1u) : q.origins + 32ull * r;
    post::Emitter e{items, base, base + count, r, key, write};
    if (!write) e.tail = 0x40000000u;
    const uint32_t tail0 = e.tail;
    uint32_t err = 0;
    const bool ok = post::walk_emit(a.b.t, q.nodes, q.roots + 32ull * r, key, e, SideRule{right}, err);
    const uint32_t n = (e.head - base) + (tail0 - e.tail);
    if (write) {
        if (!ok || e.head != e.tail) a.b.p.trie_bad[r] = 1u;  // (the two passes disagree: cannot happen)
        return n;
    }
    q.walk_err[2u * r + (right ? 1u : 0u)] = ok ? 0u : err;
    if (!ok) {
        a.b.p.trie_bad[r] = 1u;  // (nobody builds it: its status is the walk's)
        return 0;
    }
    if (right) q.more[r] = n != 0u ? 1u : 0u;
    return n;
}
__global__ void __launch_bounds__(64) range_count_kernel(const Args a) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, lanes = a.r.n_leaves + 2u * a.r.n_ranges;
    if (x > lanes) return;
    a.b.p.cnt[x] = x < lanes ? emit_lane(a, x, false, 0, 0) : 0u;
}
__global__ void __launch_bounds__(64) range_emit_kernel(const Args a) {
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, lanes = a.r.n_leaves + 2u * a.r.n_ranges;
    if (x == 0) a.b.p.counters[POST_CNT_ITEMS] = post::n_items_of(a.b.p);
    if (x >= lanes || !post::usable(a.b.p)) return;
    const uint32_t base = a.b.p.cnt[x];
    emit_lane(a, x, true, base, a.b.p.cnt[x + 1] - base);
}

// ---------------------------------------------------------------- the leaf pass
// Two size classes, as the trie hasher's leaf pass has them: a node below one rate block (an account, a storage slot: 256 lanes a
// workgroup, 35 dwords of LDS each) and one below four (64 lanes with 137 dwords each); a longer one is left to attach, as before.
// The slot sizes are odd: the lanes' equal offsets fall into different banks.  The lane zeroes the rate blocks its node needs, writes
// the node there and hashes it with the trie hasher's staged sponge (absorb.hip.h: keccak256_staged).
template <uint32_t BLOCKS, uint32_t LANES>
__global__ void __launch_bounds__(LANES) range_leaf_kernel(const Args a) {
    constexpr uint32_t SLOT_DW = BLOCKS * RATE_DWORDS + 1u;
    __shared__ uint32_t s_stage[LANES * SLOT_DW];
    const PoststateArgs& p = a.b.p;
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    if (!post::usable(p)) return;
    const uint32_t total = post::n_items_of(p);
    if (i >= total) return;
    post::Item* const me = post::post_items(p) + i;
    if (me->kind != post::IK_LEAF_OLD || me->plen != 64u || post::trie_skipped(p, me->trie)) return;
    const uint32_t vlen = me->vlen;
    if (vlen == 0u || vlen > MAX_LEAF_VALUE) return;  // (a proof's own leaf may carry anything: attach decides)
    // the depth of the branch this leaf will hang under: the longer of the prefixes shared with its neighbours (-1: alone in its trie)
    int32_t d = me->lcp;
    if (i + 1u < total && me[1].lcp > d) d = me[1].lcp;  // (the next trie's first item has -1)
    const uint32_t n = 63u - (uint32_t)d;  // nibbles left below the branch: path[d + 1 .. 64)
    const uint8_t* const v = (me->key ? p.leaf_vals : p.nodes) + me->src;
    const uint32_t hl = n / 2u + 1u, hpl = hl == 1u ? 1u : 1u + hl;
    const uint32_t sl = vlen == 1u && v[0] < 0x80u ? 1u : hdr_len(vlen) + vlen;
    const uint32_t pl = hpl + sl, node_len = hdr_len(pl) + pl;
    if (node_len >= BLOCKS * RATE || (BLOCKS > 1u && node_len < RATE)) return;  // (another class's)
    uint32_t* const slot = s_stage + threadIdx.x * SLOT_DW;
    const uint32_t clear = (node_len / RATE + 1u) * RATE_DWORDS;
    for (uint32_t k = 0; k < clear; ++k) slot[k] = 0u;
    uint8_t* const enc = reinterpret_cast<uint8_t*>(slot);
    uint32_t w = put_hdr(enc, 0xc0u, pl);
    if (hl != 1u) enc[w++] = (uint8_t)(0x80u + hl);
    const uint32_t from = (uint32_t)(d + 1);
    enc[w++] = (uint8_t)(((2u + (n & 1u)) << 4) | ((n & 1u) ? post::nib_of(me->path, from) : 0u));
    for (uint32_t j = from + (n & 1u); j < 64u; j += 2u) enc[w++] = me->path[j >> 1];  // (j is even: a whole byte of the key)
    w += put_str(enc + w, v, vlen);
    const bool hashed = node_len >= 32u || d < 0;
    if (hashed) {
        Sponge s;
        keccak256_staged(s, slot, node_len);
        for (uint32_t k = 0; k < 4u; ++k) {
            pre::put_word(me->ref, 2u * k, s.lo[k]);
            pre::put_word(me->ref, 2u * k + 1u, s.hi[k]);
        }
        me->reflen = 32;
    } else {
        for (uint32_t t = 0; t < node_len; ++t) me->ref[t] = enc[t];
        me->reflen = (uint8_t)node_len;
    }
    me->kind = post::IK_BUILT;  // a ready reference one nibble below its parent: attach copies it
    me->plen = (uint8_t)from;
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(256) range_finish_kernel(const Args a) {
    const RangeArgs& q = a.r;
    const PoststateArgs& p = a.b.p;
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool failed = false;
    if (r < q.n_ranges && post::usable(p)) {
        uint32_t st = PHANT_RANGE_VALID;
        uint8_t* const out = q.computed_root + 32ull * r;
        const uint32_t bl = q.bad_leaf[r];
        if (bl != NO_LEAF) st = rule_at(q, r, bl);
        else if (q.has_proof[r] && q.walk_err[2u * r]) st = q.walk_err[2u * r];
        else if (q.has_proof[r] && q.walk_err[2u * r + 1u]) st = q.walk_err[2u * r + 1u];
        else if (p.trie_bad[r]) st = PHANT_RANGE_ROOT_MISMATCH;
        else {
            if (p.cnt[lane0_of(q, r + 1u)] == p.cnt[lane0_of(q, r)]) post::put_empty_root(out);  // no item: the empty trie
            else for (uint32_t t = 0; t < 32u; ++t) out[t] = p.post_sroots[32ull * r + t];
            for (uint32_t t = 0; t < 32u; ++t)
                if (out[t] != q.roots[32ull * r + t]) st = PHANT_RANGE_ROOT_MISMATCH;
        }
        failed = st != PHANT_RANGE_VALID;
        if (failed)
            for (uint32_t t = 0; t < 32u; ++t) out[t] = 0u;
        q.status[r] = (uint8_t)st;
        q.has_more[r] = (uint8_t)(!failed && q.has_proof[r] && q.leaf_first[r + 1] > q.leaf_first[r] && q.more[r] ? 1u : 0u);
        q.out_bad_leaf[r] = bl;
    }
    // the counts: one atomic per wave each (the lowest lane that has something to say holds the lowest index)
    const unsigned long long m = __ballot(failed);
    if (m && lane == (uint32_t)__builtin_ctzll(m)) {
        atomicAdd(&q.ctl[RANGE_CTL_FAILED], (uint32_t)__builtin_popcountll(m));
        atomicMax(&q.ctl[RANGE_CTL_FIRST], q.n_ranges - r);
    }
    if (r == 0u) q.ctl[RANGE_CTL_ITEMS] = post::n_items_of(p);
}

}  // namespace range

// leaf rules -> count -> scan -> emit -> link -> leaf pass -> every trie level by level -> roots -> finish.  The record table of `epoch`
// has been filled (launch_nodeset_hash).  The caller has zeroed a.trie_bad, a.walk_err, a.more, a.counters and a.ctl and set a.bad_leaf to
// ff..ff.
hipError_t launch_range_verify(const RangeArgs& q, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch, const uint32_t salt[2], hipStream_t st) {
    const uint32_t lanes = q.n_leaves + 2u * q.n_ranges;
    range::Args a;
    a.r = q;
    PoststateArgs p{};
    p.nodes = q.nodes;
    p.nodes_len = q.nodes_len;
    p.na = q.n_ranges;  // tries 0 .. n_ranges: all of them "storage tries" of pass 0; cnt[na + ns] is the list's length
    p.ns = lanes - q.n_ranges;
    p.post_sroots = q.built_root;
    p.cnt = q.cnt;
    p.scan_scratch = q.scan_scratch;
    p.items_raw = q.items_raw;
    p.cap_items = q.cap_items;
    p.counters = q.counters;
    p.trie_bad = q.trie_bad;
    p.leaf_vals = q.vals;
    a.b.p = p;
    VerifyArgs v{};
    v.nodes = q.nodes;
    v.nodes_len = q.nodes_len;
    a.b.t = nodeset_args(v, 0, cap_nodes, ws, epoch, salt, 0);
    const uint32_t lg = (lanes + 1u + 63u) / 64u, ig = (q.cap_items + 63u) / 64u;
    if (q.n_leaves) hipLaunchKernelGGL(range::range_leaf_rule_kernel, dim3(grid256(q.n_leaves)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(range::range_count_kernel, dim3(lg), dim3(64), 0, st, a);
    hipError_t e = launch_exclusive_scan_u32(p.cnt, lanes + 1u, p.scan_scratch, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(range::range_emit_kernel, dim3(lg), dim3(64), 0, st, a);
    hipLaunchKernelGGL(post::post_link_kernel, dim3(grid256(q.cap_items)), dim3(256), 0, st, p);
    if (q.leaf_pass) {
        hipLaunchKernelGGL((range::range_leaf_kernel<1, 256>), dim3(grid256(q.cap_items)), dim3(256), 0, st, a);
        hipLaunchKernelGGL((range::range_leaf_kernel<4, 64>), dim3(ig), dim3(64), 0, st, a);
    }
    launch_post_levels(a.b, ig, 0, st);
    hipLaunchKernelGGL(range::range_finish_kernel, dim3(grid256(q.n_ranges)), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_range_check(const RangeArgs& q, hipStream_t st) {
    const uint32_t most = q.n_leaves > q.n_nodes ? q.n_leaves : q.n_nodes;
    hipLaunchKernelGGL(range::range_check_kernel, dim3(grid256((most > q.n_ranges ? most : q.n_ranges) + 1u)), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace phant
#endif  // PHANT_RANGE_RULES_ONLY
#undef RANGE_HD
