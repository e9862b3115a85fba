// poststate.hip.h -- the post-state root of a stateless block from its execution witness (phant_exec_witness_poststate), the kernels
// behind the pre-state pipeline.  Included by mpt_verify_nodeset.hip (it resolves references through that file's record table).
//
// No trie is mutated key by key.  Every trie a key of the witness lives in (the storage tries, then the state trie) becomes a
// sorted, prefix-free ITEM LIST, which is hashed bottom-up as mptize would build it:
//
//   post_slot_action_kernel / post_account_action_kernel   a lane per key: what the block does to it (keep the old leaf, a new leaf,
//                          remove it, nothing there), from the proven status and the caller's writes
//   (launch_order_digests orders the hashed keys, grouped by trie)
//   post_emit_kernel       a lane per key in that order, twice (count, exclusive scan, write): it walks its proven path again and
//                          emits, in path order, the fifteen other slots of every branch on it that no neighbouring key of the list
//                          is responsible for (opaque references), the old leaf or the extension's child it diverges from, and its
//                          own leaf.  Two neighbours and the common prefixes with them decide who emits what, so every item is
//                          written once and the concatenation over the keys IS the sorted list: no deduplication, no second sort.
//   post_link_kernel       a lane per item: the common prefix with its predecessor (-1 at a trie's first item)
//   post_level_kernel      once per nibble depth 63 .. 0: the items that share exactly `depth` nibbles are the children of one
//                          branch; the lane of the first builds the node, hashes it and becomes the branch's item.  A child whose
//                          path is longer than depth + 1 is wrapped: a leaf takes the longer path, a node known to be a branch
//                          hangs under an extension, a reference of unknown type is resolved through the record table and merged
//                          (leaf / extension) -- or, if nothing in the set hashes to it, every removed key under the branch that held
//                          it gets PHANT_PROOF_MISSING_SIBLING.  No workgroup waits for another: a level is a launch.
//   post_root_kernel       a lane per trie: the last item standing is the root node (always hashed)
//   post_finish_kernel     MISSING_SIBLING into the statuses, the post storage roots of accounts that do not exist afterwards
//
// phant_exec_witness_advance runs the same kernels with a sink behind node_ref: every hashed node the build constructs leaves the
// lane's private buffer for a device blob, with a descriptor of its position.  Without a sink nothing changes.
//
// Soundness: a byte enters a node built here from (a) a post value of the caller or (b) a node that the emit walk reached from the
// trusted root (or a storage root proven under it) through references resolved by Keccak in the record table, or such a node's
// child reference resolved the same way.  Nodes of the set that nothing reachable refers to are never looked at.
#pragma once
#include "launch.h"
#include "../../include/phant_gpu.h"

namespace phant {
namespace post {

enum : uint32_t { ACT_NONE = 0, ACT_OLD = 1, ACT_NEW = 2, ACT_REMOVE = 3 };
enum : uint32_t { IK_LEAF_OLD = 0, IK_LEAF_SLOT = 1, IK_LEAF_ACC = 2, IK_REF_HASH = 3, IK_REF_BRANCH = 4, IK_REF_EMBED = 5, IK_BUILT = 6 };
enum : uint32_t { F_WRITE = 1u, F_BADKEEP = 2u };
constexpr uint32_t NODE_BUF = 640;   // a branch is at most 532 bytes; a leaf 3 + 34 + 3 + MAX_VALUE
constexpr uint32_t MAX_VALUE = 560;  // the longest old leaf value carried over

struct Args {
    PoststateArgs p;
    ns::Args t;  // the record table of the call's epoch
};

PHANT_DEV uint32_t nib_of(const uint8_t* k, uint32_t i) {
    const uint32_t b = k[i >> 1];
    return (i & 1u) ? (b & 0x0fu) : (b >> 4);
}
PHANT_DEV void nib_put(uint8_t* k, uint32_t i, uint32_t v) {
    const uint32_t b = k[i >> 1];
    k[i >> 1] = (uint8_t)((i & 1u) ? ((b & 0xf0u) | v) : ((b & 0x0fu) | (v << 4)));
}
PHANT_DEV uint32_t common_nibbles(const uint8_t* a, const uint8_t* b, uint32_t n) {
    uint32_t k = 0;
    while (k < n && nib_of(a, k) == nib_of(b, k)) ++k;
    return k;
}
PHANT_DEV void put_empty_root(uint8_t* out) {
    for (uint32_t w = 0; w < 8u; ++w) pre::put_word(out, w, pre::empty_root_word(w));
}
PHANT_DEV bool failed_already(const PoststateArgs& p) { return p.counters[PRE_CNT_FAILED] != 0u; }

// ---------------------------------------------------------------- actions
__global__ void __launch_bounds__(256) post_slot_action_kernel(const PoststateArgs p) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.ns) return;
    const uint32_t acc = p.slot_account[j];
    const uint32_t op = p.op[acc], ast = p.acc_status[acc], st = p.slot_status[j];
    const bool wr = p.slot_write && p.slot_write[j] != 0u && op != PHANT_POST_DELETE;
    uint32_t act = st == PHANT_PROOF_PRESENT ? ACT_OLD : ACT_NONE;
    if (wr) {
        if (ast == PHANT_PROOF_ABSENT && op == PHANT_POST_KEEP) {
            atomicOr(&p.acc_flag[acc], F_BADKEEP);  // a slot under an account that does not exist and is not created
        } else {
            uint32_t any = 0;
            for (uint32_t t = 0; t < 32u; ++t) any |= p.post_slot_vals[32ull * j + t];
            act = any ? ACT_NEW : (st == PHANT_PROOF_PRESENT ? ACT_REMOVE : ACT_NONE);
            atomicOr(&p.acc_flag[acc], F_WRITE);
        }
    }
    p.act[p.na + j] = (uint8_t)act;
    p.seg_of[p.na + j] = acc;
}

__global__ void __launch_bounds__(256) post_account_action_kernel(const PoststateArgs p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.na) return;
    uint32_t st = p.acc_status[i];
    const uint32_t op = p.op[i], fl = p.acc_flag[i];
    if ((fl & F_BADKEEP) && st == PHANT_PROOF_ABSENT) {
        st = PHANT_PROOF_MISMATCH;
        p.acc_status[i] = (uint8_t)st;
        atomicAdd(&p.counters[PRE_CNT_FAILED], 1u);
    }
    const bool present = st == PHANT_PROOF_PRESENT;
    uint32_t act;
    if (op == PHANT_POST_SET) act = ACT_NEW;
    else if (op == PHANT_POST_DELETE) act = present ? ACT_REMOVE : ACT_NONE;
    else act = present ? ((fl & F_WRITE) ? ACT_NEW : ACT_OLD) : ACT_NONE;
    p.act[i] = (uint8_t)act;
    p.seg_of[i] = p.na;  // the state trie: behind every storage trie
    // the storage root an account that has no slot among the keys keeps; a trie with keys overwrites it (post_root_kernel)
    uint8_t* const sr = p.post_sroots + 32ull * i;
    if (p.slot_first[i + 1] > p.slot_first[i]) put_empty_root(sr);
    else for (uint32_t t = 0; t < 32u; ++t) sr[t] = p.pre_sroots[32ull * i + t];
    if (i == 0) put_empty_root(p.state_root);
}

// ---------------------------------------------------------------- nodes
struct Node {
    RlpItem it[17];
    uint32_t cnt;  // 17: branch, 2: leaf / extension, 0: not a node
    uint32_t plen, leaf, odd;
};
PHANT_DEV void decode_node(const uint8_t* nd, uint32_t len, Node& n) {
    n.cnt = 0;
    const GlobalBytes b{nd};
    RlpItem outer;
    if (!rlp_decode(b, 0, len, outer) || outer.total != len || !outer.is_list) return;
    uint32_t cnt = 0, off = 0;
    while (off < outer.len) {
        if (cnt == 17u) return;
        if (!rlp_decode(b, outer.pay + off, outer.len - off, n.it[cnt])) return;
        off += n.it[cnt].total;
        ++cnt;
    }
    if (cnt == 17u) {
        for (uint32_t s = 0; s < 16u; ++s)
            if (ref_kind(n.it[s]) == REF_BAD) return;
        if (n.it[16].is_list) return;
    } else if (cnt == 2u) {
        const RlpItem& i0 = n.it[0];
        if (i0.is_list || i0.len == 0u || i0.len > 33u) return;
        const uint32_t b0 = nd[i0.pay], flag = b0 >> 4;
        if (flag > 3u) return;
        n.leaf = (flag >> 1) & 1u;
        n.odd = flag & 1u;
        if (!n.odd && (b0 & 0x0fu)) return;
        n.plen = 2u * (i0.len - 1u) + n.odd;
        if (n.leaf) {
            if (n.it[1].is_list) return;
        } else {
            const uint32_t k = ref_kind(n.it[1]);
            if (n.plen == 0u || k == REF_BAD || k == REF_EMPTY) return;
        }
    } else {
        return;
    }
    n.cnt = cnt;
}
// nibble j of a leaf's / an extension's hex-prefix path
PHANT_DEV uint32_t hp_nibble(const uint8_t* nd, const Node& n, uint32_t j) {
    const uint32_t pj = j + (n.odd ? 1u : 2u);
    const uint32_t b = nd[n.it[0].pay + (pj >> 1)];
    return (pj & 1u) ? (b & 0x0fu) : (b >> 4);
}
PHANT_DEV void words_of(const uint8_t* h, uint32_t (&w)[8]) {
    for (uint32_t k = 0; k < 8u; ++k) w[k] = pre::get_word(h, k);
}

// ---------------------------------------------------------------- emit
struct Item {
    uint8_t path[32];
    uint8_t ref[32];   // IK_REF_* / IK_BUILT: the reference (32: a hash, less: an embedded node)
    uint64_t src;      // IK_LEAF_OLD: the value's bytes in the node blob
    uint32_t vlen;
    uint32_t key;      // IK_LEAF_SLOT / IK_LEAF_ACC: the slot / the account
    uint32_t trie;
    int32_t lcp;
    uint32_t nxt;
    uint8_t plen, kind, reflen, pad;
};

static_assert(sizeof(Item) == POSTSTATE_ITEM_BYTES, "the host sizes the list by it");
PHANT_DEV Item* post_items(const PoststateArgs& p) { return static_cast<Item*>(p.items_raw); }

struct Emitter {
    Item* items;
    uint32_t head, tail;  // next item in front of the key's own, one past the last free place behind it
    uint32_t trie;
    const uint8_t* key;
    bool write;
    PHANT_DEV Item* place(bool before) {
        if (write && head >= tail) {  // (more than was counted: cannot happen; never written beyond the key's own places)
            if (before) ++head;
            return nullptr;
        }
        if (before) return write ? items + head++ : (++head, nullptr);
        return write ? items + --tail : (--tail, nullptr);
    }
    PHANT_DEV void fill(Item* it, uint32_t depth, uint32_t kind) {
        for (uint32_t t = 0; t < 32u; ++t) it->path[t] = t < (depth + 1u) / 2u ? key[t] : 0u;
        if (depth & 1u) it->path[depth >> 1] &= 0xf0u;
        it->trie = trie;
        it->kind = (uint8_t)kind;
        it->plen = (uint8_t)depth;
        it->reflen = 0;
        it->src = 0;
        it->vlen = 0;
        it->key = 0;
        it->lcp = -1;
        it->nxt = 0;
        it->pad = 0;
    }
};
PHANT_DEV void set_ref(Item* it, const uint8_t* nd, const RlpItem& r) {
    if (ref_kind(r) == REF_HASH) {
        for (uint32_t t = 0; t < 32u; ++t) it->ref[t] = nd[r.pay + t];
        it->reflen = 32;
    } else {  // an embedded node: its whole encoding
        const uint32_t at = r.pay - (r.total - r.len);
        for (uint32_t t = 0; t < 32u; ++t) it->ref[t] = t < r.total ? nd[at + t] : 0u;
        it->reflen = (uint8_t)r.total;
        it->kind = IK_REF_EMBED;
    }
}

// The walk of one key's path from `root` through the record table, shared by the post-state emit (emit_key) and the range walkers
// (range_verify.hip.h).  What is emitted next to the path is the caller's RULE:
//   rule.slots(pos, nib, front_end, back_begin, back_end)   at a branch at depth pos where the key has nibble nib: the slots [0, front_end)
//                          go in front of the key (in path order), the slots [back_begin, back_end) behind it (written from the back)
//   rule.diverging(before, pos, cmp)   the walk leaves the path at a leaf / an extension that sorts in front of (before) or behind the key:
//                          is it this walker's to emit?  cmp(other) compares the node's path with `other`'s nibbles behind pos
// The key's own leaf is never emitted here.  Sets `err` (PHANT_PROOF_MISSING_NODE / PHANT_PROOF_BAD_NODE) and returns false on failure.
template <class Rule>
PHANT_DEV bool walk_emit(const ns::Args& t, const uint8_t* const nodes, const uint8_t* const root, const uint8_t* const key, Emitter& e,
                         const Rule& rule, uint32_t& err) {
    const uint32_t ovf = t.hdr[ns::HDR_OVF + 32u * (t.epoch & 1u)];
    uint32_t want[8];
    words_of(root, want);
    const uint8_t* cur = nullptr;
    uint32_t cur_len = 0, pos = 0;
    bool by_hash = true, at_root = true;
    Node n;
    for (;;) {
        if (by_hash) {
            if (at_root && is_empty_root(want)) break;  // an empty trie: nothing but the key's own leaf
            const ns::Found f = ns::set_find(t, want, ovf);
            if (!f.ok) {
                err = PHANT_PROOF_MISSING_NODE;
                return false;
            }
            cur = nodes + f.off;
            cur_len = f.len_canon & ~ns::CANON_BIT;
        }
        at_root = false;
        decode_node(cur, cur_len, n);
        if (n.cnt == 0u) {
            err = PHANT_PROOF_BAD_NODE;
            return false;
        }
        if (n.cnt == 17u) {
            if (pos >= 64u || n.it[16].len != 0u) {  // (keys are 32 bytes: no branch carries a value)
                err = PHANT_PROOF_BAD_NODE;
                return false;
            }
            const uint32_t nib = nib_of(key, pos);
            uint32_t front_end = 0, back_begin = 16, back_end = 16;
            rule.slots(pos, nib, front_end, back_begin, back_end);
            for (uint32_t s = 0; s < front_end; ++s) {
                if (ref_kind(n.it[s]) == REF_EMPTY) continue;
                Item* it = e.place(true);
                if (it) {
                    e.fill(it, pos + 1u, IK_REF_HASH);
                    nib_put(it->path, pos, s);
                    set_ref(it, cur, n.it[s]);
                }
            }
            // the slots above it: written from the back, the shallowest branch last
            for (uint32_t s = back_end; s-- > back_begin;) {
                if (ref_kind(n.it[s]) == REF_EMPTY) continue;
                Item* it = e.place(false);
                if (it) {
                    e.fill(it, pos + 1u, IK_REF_HASH);
                    nib_put(it->path, pos, s);
                    set_ref(it, cur, n.it[s]);
                }
            }
            const RlpItem& c = n.it[nib];
            pos += 1u;
            const uint32_t ck = ref_kind(c);
            if (ck == REF_EMPTY) break;
            if (ck == REF_HASH) {
                words_of(cur + c.pay, want);
                by_hash = true;
            } else {
                cur += c.pay - (c.total - c.len);  // an embedded child: its bytes inside its parent's
                cur_len = c.total;
                by_hash = false;
            }
            continue;
        }
        // a leaf or an extension at depth pos: every key of the list with these pos nibbles arrives here
        if (pos + n.plen > 64u || (n.leaf && pos + n.plen != 64u)) {
            err = PHANT_PROOF_BAD_NODE;
            return false;
        }
        auto cmp = [&](const uint8_t* other) -> int {  // the node's path against `other`'s nibbles behind pos
            for (uint32_t j = 0; j < n.plen; ++j) {
                const uint32_t x = hp_nibble(cur, n, j), y = nib_of(other, pos + j);
                if (x != y) return x < y ? -1 : 1;
            }
            return 0;
        };
        const int c = cmp(key);
        if (c == 0) {
            if (n.leaf) break;  // the key's own leaf
            pos += n.plen;
            const RlpItem& ch = n.it[1];
            if (ref_kind(ch) == REF_HASH) {
                words_of(cur + ch.pay, want);
                by_hash = true;
            } else {
                cur += ch.pay - (ch.total - ch.len);
                cur_len = ch.total;
                by_hash = false;
            }
            continue;
        }
        // the key leaves the path here: the old leaf / the extension's child stays, emitted by exactly one walker
        const bool before = c < 0;
        if (rule.diverging(before, pos, cmp)) {
            // (in front of the key it is the last item there; behind it, the first: it must precede everything written from the back so
            // far -- nothing of THIS depth or deeper has been, and shallower slots sort behind it, so the next place from the back is right)
            Item* it = e.place(before);
            if (it) {
                e.fill(it, pos, n.leaf ? IK_LEAF_OLD : IK_REF_BRANCH);
                for (uint32_t j = 0; j < n.plen; ++j) nib_put(it->path, pos + j, hp_nibble(cur, n, j));
                it->plen = (uint8_t)(pos + n.plen);
                if (n.leaf) {
                    it->src = (uint64_t)(cur - nodes) + n.it[1].pay;
                    it->vlen = n.it[1].len;
                } else {
                    set_ref(it, cur, n.it[1]);  // (an extension's child is a branch: IK_REF_BRANCH needs no lookup; embedded: decoded)
                }
            }
        }
        break;
    }
    return true;
}

// the post-state's rule: two neighbours of the ordered list and the common prefixes with them decide who emits what
struct NeighbourRule {
    int32_t lp, ln;  // nibbles shared with the predecessor / the successor in the same trie (-1: there is none)
    const uint8_t *kp, *kn;
    PHANT_DEV void slots(uint32_t pos, uint32_t nib, uint32_t& front_end, uint32_t& back_begin, uint32_t& back_end) const {
        // the slots below the key's: this key's unless its predecessor passes through the same branch (which then has emitted
        // the slots between the two as the ones above its own)
        front_end = lp >= (int32_t)pos ? 0u : nib;
        // the slots above it, up to its successor's
        back_begin = nib + 1u;
        back_end = 16u;
        if (ln > (int32_t)pos) back_begin = 16u;
        else if (ln == (int32_t)pos) back_end = nib_of(kn, pos);
    }
    template <class Cmp>
    PHANT_DEV bool diverging(bool before, uint32_t pos, const Cmp& cmp) const {
        if (before) return lp < (int32_t)pos || cmp(kp) > 0;
        return ln < (int32_t)pos;
    }
};

// One key of the ordered list (rank r).  WRITE = false: only counts.  Returns the number of items, or sets `err`.
PHANT_DEV uint32_t emit_key(const Args& a, const uint32_t r, const bool write, const uint32_t base, const uint32_t count, uint32_t& err) {
    const PoststateArgs& p = a.p;
    const uint32_t nk = p.na + p.ns;
    const uint32_t k = p.order[r];
    const uint32_t trie = p.seg_of[k];
    const uint8_t* const key = p.keys + 32ull * k;
    NeighbourRule rule{-1, -1, key, key};
    if (r > 0 && p.seg_of[p.order[r - 1]] == trie) {
        rule.kp = p.keys + 32ull * p.order[r - 1];
        rule.lp = (int32_t)common_nibbles(rule.kp, key, 64);
    }
    if (r + 1 < nk && p.seg_of[p.order[r + 1]] == trie) {
        rule.kn = p.keys + 32ull * p.order[r + 1];
        rule.ln = (int32_t)common_nibbles(rule.kn, key, 64);
    }
    if (rule.lp == 64 || rule.ln == 64) {  // the same key twice: no trie has it twice
        err = PHANT_PROOF_BAD_INPUT;
        return 0;
    }
    Emitter e{post_items(p), base, base + count, trie, key, write};
    if (!write) e.tail = 0x40000000u;
    const uint32_t tail0 = e.tail;
    const uint8_t* root = trie == p.na ? p.parent_root : p.pre_sroots + 32ull * trie;
    if (!walk_emit(a.t, p.nodes, root, key, e, rule, err)) return 0;
    // the key's own leaf
    const uint32_t act = p.act[k];
    if (act == ACT_OLD || act == ACT_NEW) {
        Item* it = e.place(true);
        if (it) {
            e.fill(it, 64u, IK_LEAF_OLD);
            if (act == ACT_OLD) {
                it->src = k < p.na ? p.acc_voff[k] : p.slot_voff[k - p.na];
                it->vlen = k < p.na ? p.acc_vlen[k] : p.slot_vlen[k - p.na];
            } else {
                it->kind = k < p.na ? IK_LEAF_ACC : IK_LEAF_SLOT;
                it->key = k < p.na ? k : k - p.na;
            }
        }
    }
    const uint32_t n_items = (e.head - base) + (tail0 - e.tail);
    if (write && e.head != e.tail) err = PHANT_PROOF_BAD_INPUT;  // (the two passes disagree: cannot happen)
    return n_items;
}

PHANT_DEV uint32_t n_items_of(const PoststateArgs& p) { return p.cnt[p.na + p.ns]; }
// the passes behind the count: nothing failed so far and the list fits (else the host runs the call again with the room it needs)
PHANT_DEV bool usable(const PoststateArgs& p) {
    return !failed_already(p) && p.counters[POST_CNT_EMIT_FAILED] == 0u && n_items_of(p) <= p.cap_items;
}
// (a counter no lane of the same launch reads: which keys fail and how many never depends on the order the lanes run in)
PHANT_DEV void key_failed(const PoststateArgs& p, uint32_t k, uint32_t status, uint32_t counter) {
    if (k < p.na) p.acc_status[k] = (uint8_t)status;
    else p.slot_status[k - p.na] = (uint8_t)status;
    atomicAdd(&p.counters[counter], 1u);
}

// what cannot be built: the whole call's (POST_CNT_INTERNAL) -- or, where the tries of a call stand each for itself (trie_bad: the ranges
// of phant_mpt_verify_ranges), that trie's alone; the kernels behind skip such a trie
PHANT_DEV void cannot_build(const PoststateArgs& p, uint32_t trie) {
    if (p.trie_bad) p.trie_bad[trie] = 1u;
    else atomicAdd(&p.counters[POST_CNT_INTERNAL], 1u);
}
PHANT_DEV bool trie_skipped(const PoststateArgs& p, uint32_t trie) { return p.trie_bad && p.trie_bad[trie] != 0u; }

__global__ void __launch_bounds__(64) post_count_kernel(const Args a) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x, nk = a.p.na + a.p.ns;
    if (r > nk) return;
    uint32_t c = 0;
    if (r < nk && !failed_already(a.p)) {
        uint32_t err = 0;
        c = emit_key(a, r, false, 0, 0, err);
        if (err) {
            key_failed(a.p, a.p.order[r], err, POST_CNT_EMIT_FAILED);
            c = 0;
        }
    }
    a.p.cnt[r] = c;
}
__global__ void __launch_bounds__(64) post_emit_kernel(const Args a) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x, nk = a.p.na + a.p.ns;
    if (r == 0) a.p.counters[POST_CNT_ITEMS] = n_items_of(a.p);
    if (r >= nk || !usable(a.p)) return;
    const uint32_t base = a.p.cnt[r], count = a.p.cnt[r + 1] - base;
    uint32_t err = 0;
    emit_key(a, r, true, base, count, err);
    if (err) atomicAdd(&a.p.counters[POST_CNT_INTERNAL], 1u);
}

__global__ void __launch_bounds__(256) post_link_kernel(const PoststateArgs p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (!usable(p) || i >= n_items_of(p)) return;
    Item* const it = post_items(p) + i;
    int32_t l = -1;
    if (i > 0 && it[-1].trie == it->trie) {
        const uint32_t m = it->plen < it[-1].plen ? it->plen : it[-1].plen;
        l = (int32_t)common_nibbles(it->path, it[-1].path, m);
        // one path inside another: the list is not prefix-free; (per-trie form) or not in path order
        if ((uint32_t)l == m || (p.trie_bad && nib_of(it[-1].path, (uint32_t)l) > nib_of(it->path, (uint32_t)l))) cannot_build(p, it->trie);
    }
    it->lcp = l;
    it->nxt = i + 1u;
}

// ---------------------------------------------------------------- encoding
// (headers, strings and integers: rlp.h's writers)
// rlp([hex-prefix(nibs[0 .. n), leaf), item]) -- mpt.zig:187-193 / :254-261 / :285-314; `item` is RLP already
PHANT_DEV uint32_t put_short_node(uint8_t* out, const uint8_t* nibs, uint32_t n, bool leaf, const uint8_t* item, uint32_t ilen) {
    const uint32_t hl = n / 2u + 1u, hpl = hl == 1u ? 1u : 1u + hl, pl = hpl + ilen;
    uint32_t p = put_hdr(out, 0xc0u, pl);
    if (hl != 1u) out[p++] = (uint8_t)(0x80u + hl);
    const uint32_t flag = (leaf ? 2u : 0u) + (n & 1u);
    out[p++] = (uint8_t)((flag << 4) | ((n & 1u) ? nibs[0] : 0u));
    for (uint32_t j = n & 1u; j < n; j += 2u) out[p++] = (uint8_t)((nibs[j] << 4) | nibs[j + 1]);
    for (uint32_t t = 0; t < ilen; ++t) out[p + t] = item[t];
    return p + ilen;
}
// a node's reference: itself below 32 bytes (mpt.zig:104 / :112), else -- or when `force` (the root, :42) -- its Keccak-256
// -- the single place a built node is hashed, and therefore where phant_exec_witness_advance takes its nodes from: a hashed node
// goes to the sink (`at.p` null: there is none) with the position it was built for.  A lane reserves its room with one atomicAdd on the
// byte cursor and one on the node count; what does not fit is counted and not written (the host runs the call again with the
// counted sizes).  Nothing is emitted for the storage trie of an account that does not exist afterwards (the build still walks
// it; its root is overwritten by post_finish_kernel) nor in a run whose key order the device sort left undecided.
struct NodeAt {
    const PoststateArgs* p;
    uint32_t trie, item, where;  // PoststateNodeDesc
};
PHANT_DEV void sink_put(const NodeAt& at, const uint8_t* node, uint32_t len) {
    const PoststateArgs& p = *at.p;
    if (at.trie < p.na && (p.act[at.trie] == ACT_REMOVE || p.act[at.trie] == ACT_NONE)) return;
    if (p.sink_undecided && *p.sink_undecided != 0u) return;
    const unsigned long long off = atomicAdd(p.sink_bytes, (unsigned long long)len);
    const uint32_t idx = atomicAdd(&p.sink_cnt[POST_SINK_NODES], 1u);
    if (off + len > p.sink_cap_bytes || idx >= p.sink_cap_desc) {
        atomicOr(&p.sink_cnt[POST_SINK_OVERFLOW], 1u);
        return;
    }
    uint8_t* const out = p.sink_blob + off;
    for (uint32_t t = 0; t < len; ++t) out[t] = node[t];
    PoststateNodeDesc& d = p.sink_desc[idx];
    d.off = off;
    d.len = len;
    d.trie = at.trie;
    d.item = at.item;
    d.where = at.where;
}
PHANT_DEV uint32_t node_ref(const uint8_t* node, uint32_t len, bool force, uint8_t* ref, const NodeAt& at) {
    if (len < 32u && !force) {
        for (uint32_t t = 0; t < len; ++t) ref[t] = node[t];
        return len;
    }
    if (at.p) sink_put(at, node, len);
    Sponge s;
    keccak256_global(s, node, len);
    for (uint32_t k = 0; k < 4u; ++k) {
        pre::put_word(ref, 2u * k, s.lo[k]);
        pre::put_word(ref, 2u * k + 1u, s.hi[k]);
    }
    return 32;
}
PHANT_DEV uint32_t put_ref_item(uint8_t* out, const uint8_t* ref, uint32_t rl) {
    uint32_t p = 0;
    if (rl == 32u) out[p++] = 0xa0;
    for (uint32_t t = 0; t < rl; ++t) out[p + t] = ref[t];
    return p + rl;
}

// the removed keys of `trie` under the first `plen` nibbles of `path`: the collapse there cannot be decided
PHANT_DEV void mark_removed_under(const PoststateArgs& p, uint32_t trie, const uint8_t* path, uint32_t plen) {
    const uint32_t nk = p.na + p.ns;
    auto below = [&](uint32_t r) -> bool {  // key of rank r sorts in front of (trie, path)
        const uint32_t k = p.order[r], s = p.seg_of[k];
        if (s != trie) return s < trie;
        const uint8_t* key = p.keys + 32ull * k;
        for (uint32_t j = 0; j < plen; ++j) {
            const uint32_t x = nib_of(key, j), y = nib_of(path, j);
            if (x != y) return x < y;
        }
        return false;
    };
    uint32_t lo = 0, hi = nk;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (below(mid)) lo = mid + 1u;
        else hi = mid;
    }
    uint32_t marked = 0;
    for (uint32_t r = lo; r < nk; ++r) {
        const uint32_t k = p.order[r];
        if (p.seg_of[k] != trie || common_nibbles(p.keys + 32ull * k, path, plen) != plen) break;
        if (p.act[k] == ACT_REMOVE) {
            p.key_bad[k] = 1;
            ++marked;
        }
    }
    if (!marked) atomicAdd(&p.counters[POST_CNT_INTERNAL], 1u);  // (no removal explains it: still no root)
}

// The reference of item `c` as the child of a branch at nibble depth d (d = -1: as the trie's root, always hashed): its node is
// built with the nibbles path[d + 1 .. plen) that the branch does not consume.
PHANT_DEV uint32_t attach(const Args& a, const Item* c, const int32_t d, const bool force, uint8_t* ref) {
    const PoststateArgs& p = a.p;
    alignas(16) uint8_t node[NODE_BUF];
    uint8_t vb[MAX_VALUE + 8];
    uint8_t nibs[64];
    uint32_t n = 0;
    const NodeAt here{p.sink_blob ? &p : nullptr, c->trie, (uint32_t)(c - post_items(p)), (uint32_t)(d + 1) << 1};
    for (uint32_t j = (uint32_t)(d + 1); j < c->plen; ++j) nibs[n++] = (uint8_t)nib_of(c->path, j);
    const uint32_t kind = c->kind;
    if (kind <= IK_LEAF_ACC) {
        uint32_t vl = 0;
        if (kind == IK_LEAF_OLD) {
            if (c->vlen > MAX_VALUE) {
                cannot_build(p, c->trie);
                return 0;
            }
            vl = put_str(vb, (c->key ? p.leaf_vals : p.nodes) + c->src, c->vlen);  // (key != 0: a caller's leaf of a range)
        } else if (kind == IK_LEAF_SLOT) {
            uint8_t v[36];
            const uint32_t l = put_minimal(v, p.post_slot_vals + 32ull * c->key, 32);
            vl = put_str(vb, v, l);
        } else {  // rlp([nonce, balance, storageRoot, codeHash]), types.zig:13-20
            const uint32_t i = c->key;
            const bool set = p.op[i] == PHANT_POST_SET;
            uint8_t body[120];
            uint32_t q = put_uint(body, set ? p.post_nonces[i] : p.pre_nonces[i]);
            q += put_minimal(body + q, (set ? p.post_balances : p.pre_balances) + 32ull * i, 32);
            q += put_str(body + q, p.post_sroots + 32ull * i, 32);
            q += put_str(body + q, (set ? p.post_code_hashes : p.pre_code_hashes) + 32ull * i, 32);
            uint8_t acc[124];
            const uint32_t h = put_hdr(acc, 0xc0u, q);
            for (uint32_t t = 0; t < q; ++t) acc[h + t] = body[t];
            vl = put_str(vb, acc, h + q);
        }
        return node_ref(node, put_short_node(node, nibs, n, true, vb, vl), force, ref, here);
    }
    if (n == 0u) {  // the reference fills the slot as it is (the root: the hash of a branch built here)
        if (force && c->reflen != 32u) {  // (over 32-byte keys a root branch is never small enough to embed)
            cannot_build(p, c->trie);
            return 0;
        }
        for (uint32_t t = 0; t < c->reflen; ++t) ref[t] = c->ref[t];
        return c->reflen;
    }
    if (kind == IK_BUILT || kind == IK_REF_BRANCH) {  // known to be a branch: it hangs under an extension
        const uint32_t il = put_ref_item(vb, c->ref, c->reflen);
        return node_ref(node, put_short_node(node, nibs, n, false, vb, il), force, ref, here);
    }
    if (p.trie_bad) {  // a range: a reference of unknown type that would have to be merged is no proof of anything
        cannot_build(p, c->trie);
        return 0;
    }
    // what the reference points to decides: never guessed
    const uint8_t* nd = c->ref;
    uint32_t nd_len = c->reflen;
    if (kind == IK_REF_HASH) {
        uint32_t want[8];
        words_of(c->ref, want);
        const ns::Found f = ns::set_find(a.t, want, a.t.hdr[ns::HDR_OVF + 32u * (a.t.epoch & 1u)]);
        if (!f.ok) {
            mark_removed_under(p, c->trie, c->path, c->plen - 1u);
            return 0;
        }
        nd = p.nodes + f.off;
        nd_len = f.len_canon & ~ns::CANON_BIT;
    }
    Node m;
    decode_node(nd, nd_len, m);
    if (m.cnt == 17u) {
        const uint32_t il = put_ref_item(vb, c->ref, c->reflen);
        return node_ref(node, put_short_node(node, nibs, n, false, vb, il), force, ref, here);
    }
    if (m.cnt != 2u || n + m.plen > 64u || m.it[1].total > MAX_VALUE) {
        mark_removed_under(p, c->trie, c->path, c->plen - 1u);
        return 0;
    }
    // a leaf takes the longer path; an extension merges with the nibbles above it
    for (uint32_t j = 0; j < m.plen; ++j) nibs[n++] = (uint8_t)hp_nibble(nd, m, j);
    const uint32_t at = m.it[1].pay - (m.it[1].total - m.it[1].len);
    for (uint32_t t = 0; t < m.it[1].total; ++t) vb[t] = nd[at + t];
    return node_ref(node, put_short_node(node, nibs, n, m.leaf != 0u, vb, m.it[1].total), force, ref, here);
}

// ---------------------------------------------------------------- build
__global__ void __launch_bounds__(64) post_level_kernel(const Args a, const int32_t d, const uint32_t state_pass) {
    const PoststateArgs& p = a.p;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (!usable(p)) return;
    const uint32_t total = n_items_of(p);
    if (i >= total) return;
    Item* const me = post_items(p) + i;
    if ((me->trie == p.na) != (state_pass != 0u) || me->lcp >= d || trie_skipped(p, me->trie)) return;
    const uint32_t first = me->nxt;
    if (first >= total || post_items(p)[first].lcp != d) return;
    // the first child of a branch at depth d: the others are the items behind it that share exactly d nibbles with their predecessor
    alignas(16) uint8_t buf[NODE_BUF];
    uint8_t ref[32];
    uint32_t pos = 3, slot = 0, c = i;
    for (;;) {
        const Item* const ch = post_items(p) + c;
        const uint32_t nib = nib_of(ch->path, (uint32_t)d);
        while (slot < nib) {
            buf[pos++] = 0x80;
            ++slot;
        }
        pos += put_ref_item(buf + pos, ref, attach(a, ch, d, false, ref));
        slot = nib + 1u;
        c = c == i ? first : ch->nxt;
        if (c >= total || post_items(p)[c].lcp != d) break;
    }
    while (slot < 17u) {  // the remaining slots and the value (keys are 32 bytes: never one)
        buf[pos++] = 0x80;
        ++slot;
    }
    const uint32_t pl = pos - 3u, hdr = hdr_len(pl);  // (at most 3: a branch is below 64 KiB)
    uint8_t* const node = buf + 3u - hdr;
    (void)put_hdr(node, 0xc0u, pl);
    const NodeAt at{p.sink_blob ? &p : nullptr, me->trie, i, ((uint32_t)(d + 1) << 1) | 1u};
    me->reflen = (uint8_t)node_ref(node, hdr + pl, false, me->ref, at);
    me->kind = IK_BUILT;
    me->plen = (uint8_t)d;
    me->nxt = c;
}

__global__ void __launch_bounds__(64) post_root_kernel(const Args a, const uint32_t state_pass) {
    const PoststateArgs& p = a.p;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (!usable(p)) return;
    const uint32_t total = n_items_of(p);
    if (i >= total) return;
    const Item* const me = post_items(p) + i;
    if ((me->trie == p.na) != (state_pass != 0u) || me->lcp != -1 || trie_skipped(p, me->trie)) return;
    if (me->nxt < total && post_items(p)[me->nxt].lcp != -1) cannot_build(p, me->trie);  // (more than one item left)
    uint8_t ref[32];
    for (uint32_t t = 0; t < 32u; ++t) ref[t] = 0;
    attach(a, me, -1, true, ref);
    uint8_t* const out = state_pass ? p.state_root : p.post_sroots + 32ull * me->trie;
    for (uint32_t t = 0; t < 32u; ++t) out[t] = ref[t];
}

__global__ void __launch_bounds__(256) post_finish_kernel(const PoststateArgs p) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.na + p.ns) return;
    if (p.key_bad[k]) key_failed(p, k, PHANT_PROOF_MISSING_SIBLING, PRE_CNT_FAILED);
    if (k < p.na && (p.act[k] == ACT_REMOVE || p.act[k] == ACT_NONE)) put_empty_root(p.post_sroots + 32ull * k);  // no such account afterwards
}

}  // namespace post

// ---------------------------------------------------------------- host side
hipError_t launch_poststate_actions(const PoststateArgs& p, hipStream_t st) {
    if (p.ns) hipLaunchKernelGGL(post::post_slot_action_kernel, dim3(grid256(p.ns)), dim3(256), 0, st, p);
    if (p.na) hipLaunchKernelGGL(post::post_account_action_kernel, dim3(grid256(p.na)), dim3(256), 0, st, p);
    return hipGetLastError();
}

// every trie of one pass (0: the tries with an index below p.na, 1: the trie p.na), level by level, then the roots: the one build
// behind the post-state calls and phant_mpt_verify_ranges
static void launch_post_levels(const post::Args& a, uint32_t item_groups, uint32_t pass, hipStream_t st) {
    for (int32_t d = 63; d >= 0; --d) hipLaunchKernelGGL(post::post_level_kernel, dim3(item_groups), dim3(64), 0, st, a, d, pass);
    hipLaunchKernelGGL(post::post_root_kernel, dim3(item_groups), dim3(64), 0, st, a, pass);
}

// count -> scan -> emit -> link -> the storage tries level by level -> their roots -> the state trie the same way -> finish
hipError_t launch_poststate_build(const PoststateArgs& p, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch, const uint32_t salt[2],
                                  hipStream_t st) {
    const uint32_t nk = p.na + p.ns;
    if (p.na == 0) return hipGetLastError();
    post::Args a;
    a.p = p;
    VerifyArgs v{};
    v.nodes = p.nodes;
    v.nodes_len = p.nodes_len;
    a.t = nodeset_args(v, 0, cap_nodes, ws, epoch, salt, 0);
    const uint32_t kg = (nk + 1u + 63u) / 64u, ig = (p.cap_items + 63u) / 64u;
    hipLaunchKernelGGL(post::post_count_kernel, dim3(kg), dim3(64), 0, st, a);
    hipError_t e = launch_exclusive_scan_u32(p.cnt, nk + 1u, p.scan_scratch, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(post::post_emit_kernel, dim3(kg), dim3(64), 0, st, a);
    hipLaunchKernelGGL(post::post_link_kernel, dim3(grid256(p.cap_items)), dim3(256), 0, st, p);
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        if (pass == 0u && p.ns == 0u) continue;
        launch_post_levels(a, ig, pass, st);
    }
    hipLaunchKernelGGL(post::post_finish_kernel, dim3(grid256(nk)), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace phant
