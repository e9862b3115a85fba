// trie_prove.hip.h -- witness generation behind the trie hasher (phant_mpt_prove_nodeset): the hashed nodes on the paths of queried
// keys, as a node set.  Included into trie_build.hip's namespace: the kernels read what a build leaves in the t1 arena (dense,
// nd_parent, nd_pd, nd_l, lcp, value_key, leaf_parent, leaf_ps) and the t2 arena (slot_bytes, slot_len) and re-encode the marked
// nodes with the build's own device functions (leaf_plan, branch_plan_node, put_branch, put_extension, put_hp).  Both build passes
// leave the same tables: the small pass numbers a node by its boundary (dense[i] == i), writes lcp[] to global memory as well as to
// LDS and resolves every nd_parent in small_climb_kernel; the min-tree, which it keeps in LDS only, is not read here.
//
//   prove_locate_kernel   a lane per query: binary search of the trie's key range; of the two neighbours the key that shares the
//                         longer nibble prefix c with the query (the exact hit if there is one) walks the same path down to depth
//                         c, so the climb from that key's leaf marks: the leaf if c reaches its path, every ancestor branch of
//                         depth d <= c, and the extension over a branch whenever c >= parent depth + 1 (the walk of DESIGN.md
//                         section 3 enters the extension and stops there unless it agrees with all of it).  Marks are atomicOr
//                         into a word per boundary; a lane stops at a branch that was marked before it came (its marker goes on to
//                         the root) unless it carries PHANT_PROVE_MAY_REMOVE, whose position masks must reach the root.
//   prove_sibling_kernel  a lane per boundary (only when flags were passed): a marked branch of which exactly one occupied
//                         position is outside the mask of the flagged, PRESENT queries gets the node under that position marked
//                         too if it is a 32-byte reference: what a collapse of that branch would have to look at.
//   prove_size_kernel     a lane per key / boundary index: which of its (extension, branch, leaf) are members -- marked AND hashed --
//                         and their bytes; exclusive scan inside the 1 024-index tile, the tile's sums
//   prove_scan_kernel     one workgroup: the tiles' sums scanned, the totals to the pinned mailbox
//   prove_base_kernel     tile bases added: node index and byte offset of every index's first member; trie_first_node
//   prove_emit_kernel     a lane per index with members: the nodes' bytes straight into the caller's blob (byte stores), node_off.
//                         The digest an extension carries is recomputed: its branch is encoded into the build's scratch blob and
//                         hashed there (the build keeps only the extension's own hash, in the parent's slot).
//
// The per-proof form (phant_mpt_prove_batch) runs all of the above with the set emitted into the prover's own arena, then:
//   prove_batch_count_kernel   a lane per query: the climb of the locate pass once more from the kept (key, common prefix), to the
//                              root without an early stop; the members on it counted, their bytes summed; scan inside the tile
//   prove_batch_scan_kernel    one workgroup: the tiles' sums scanned, the totals (64 bits each) to the pinned mailbox
//   prove_batch_place_kernel   the same climb: member `step` of query j (deepest first) lands at node base(j + 1) - 1 - step -- its
//                              set index and its byte offset; proof_first_node
//   prove_batch_gather_kernel  a wave per output node: the node's bytes from the set into the proof blob, 16 bytes a lane
//
// Position (index i, kind) in ascending order IS the output order: tries are runs of indices, so nodes come grouped by trie, every
// position once, and the same inputs give the same bytes.

constexpr uint32_t PV_BRANCH = 1u, PV_EXT = 2u, PV_SIB_BRANCH = 4u, PV_SIB_EXT = 8u, PV_MASK_SHIFT = 8u;  // a boundary's mark word
constexpr uint32_t PV_LEAF = 1u, PV_SIB_LEAF = 2u;                                                       // a key's mark byte
constexpr uint32_t PV_M_EXT = 1u, PV_M_BRANCH = 2u, PV_M_LEAF = 4u;                                      // members of an index
constexpr uint32_t PV_TILE = 1024;
constexpr uint32_t PV_ERR_TRIE = 1u, PV_ERR_SCRATCH = 2u;
// the mailbox words behind the build's own: total nodes, total bytes (two words), error flags
constexpr uint32_t MAILBOX_PROVE = N_COUNTERS + 8u;
// ... and behind those the per-proof form's: total nodes (two words), total bytes (two words)
constexpr uint32_t MAILBOX_PROVE_BATCH = MAILBOX_PROVE + 4u;
static_assert(MAILBOX_PROVE_BATCH + 4u <= Workspaces::MAILBOX_WORDS, "the prover's totals fit the pinned mailbox");
static_assert(MAILBOX_PROVE_BATCH + 4u <= Workspaces::MAILBOX_RECEIPTS, "the builder's and the prover's words end in front of the receipts'");

struct ProveDev {
    const uint8_t* qkeys;
    const uint32_t* qkey_off;
    const uint32_t* q_trie;   // optional
    const uint8_t* q_flags;   // optional
    uint32_t n_queries;
    uint8_t* q_status;        // optional
    uint32_t* nmark;          // n + 1
    uint8_t* lmark;           // n + 1
    uint8_t* members;         // n + 1
    uint32_t* nbase;          // n + 1: index of the first member node of index i
    unsigned long long* bbase;  // n + 1: its byte offset
    uint32_t* tile_cnt;       // tiles + 1
    unsigned long long* tile_bytes;  // tiles + 1
    uint32_t tiles;
    uint32_t* flags;          // 4 words: errors
    uint32_t* mailbox;
    // outputs (device; optional)
    uint8_t* nodes;
    unsigned long long* node_off;
    uint32_t* trie_first_node;
    // the per-proof form keeps what the locate pass found (optional): the key whose leaf query j climbs from (NONE: an empty trie)
    // and the nibbles the two share
    uint32_t* qk;
    uint32_t* qc;
};

// nibble j of query key bytes q
PHANT_DEV uint32_t pv_nib(const uint8_t* q, uint32_t j) {
    const uint32_t b = q[j >> 1];
    return (j & 1u) ? (b & 0x0fu) : (b >> 4);
}
// common nibble prefix of the query (qb bytes at q) and key k; `cmp`: <0 / 0 / >0 as key k is below / equal to / above the query
PHANT_DEV uint32_t pv_common(const TrieDev& t, uint32_t k, const uint8_t* q, uint32_t qb, int32_t& cmp) {
    const uint8_t* a = t.keys + t.key_off[k];
    const uint32_t la = t.key_off[k + 1] - t.key_off[k];
    const uint32_t m = la < qb ? la : qb;
    uint32_t b = 0;
    while (b < m && a[b] == q[b]) ++b;
    if (b == m) {
        cmp = la < qb ? -1 : (la > qb ? 1 : 0);
        return 2u * m;
    }
    cmp = a[b] < q[b] ? -1 : 1;
    return 2u * b + (((a[b] ^ q[b]) & 0xf0u) ? 0u : 1u);
}

__global__ void __launch_bounds__(256) prove_locate_kernel(TrieDev t, ProveDev p) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.n_queries) return;
    uint32_t tr = 0;
    if (p.q_trie) {
        tr = p.q_trie[j];
        if (tr >= t.n_tries) {
            atomicOr(&p.flags[0], PV_ERR_TRIE);
            return;
        }
    }
    uint8_t status = PHANT_PROOF_ABSENT;
    uint32_t kept_k = NONE, kept_c = 0;
    const uint32_t lo = t.n ? t.seg_first[tr] : 0u, hi = t.n ? t.seg_first[tr + 1u] : 0u;
    if (lo < hi) {
        const uint8_t* q = p.qkeys + p.qkey_off[j];
        const uint32_t qb = p.qkey_off[j + 1u] - p.qkey_off[j];
        // the first key of the trie that is not below the query
        uint32_t a = lo, b = hi;
        while (a < b) {
            const uint32_t mid = a + ((b - a) >> 1);
            int32_t cmp;
            (void)pv_common(t, mid, q, qb, cmp);
            if (cmp < 0) a = mid + 1u;
            else b = mid;
        }
        uint32_t k = a, c = 0;
        bool exact = false;
        if (a < hi) {
            int32_t cmp;
            c = pv_common(t, a, q, qb, cmp);
            exact = cmp == 0;
        }
        if (!exact && a > lo) {
            int32_t cmp;
            const uint32_t cl = pv_common(t, a - 1u, q, qb, cmp);
            if (a == hi || cl > c) {
                k = a - 1u;
                c = cl;
            }
        }
        if (exact) status = PHANT_PROOF_PRESENT;
        kept_k = k;
        kept_c = c;
        const bool flagged = exact && p.q_flags && (p.q_flags[j] & PHANT_PROVE_MAY_REMOVE);
        // the climb from key k
        const uint32_t ps = t.leaf_ps[k];
        if (ps != BRANCH_VALUE && c >= ps) p.lmark[k] = (uint8_t)PV_LEAF;  // (every writer of this pass stores the same byte)
        uint32_t node = t.leaf_parent[k];
        uint32_t pos = ps == BRANCH_VALUE ? 16u : 0xffu;  // the position the path enters the node at: the value, or a nibble
        while (node != NONE) {
            const int32_t d = t.lcp[node], pd = t.nd_pd[node];
            uint32_t bits = 0;
            if ((int32_t)c >= d) bits |= PV_BRANCH;
            if (d > pd + 1 && (int32_t)c >= pd + 1) bits |= PV_EXT;
            if (flagged) bits |= (1u << (pos == 16u ? 16u : nib_at(t, k, (uint32_t)d))) << PV_MASK_SHIFT;
            if (bits) {
                const uint32_t old = atomicOr(&p.nmark[node], bits);
                if (!flagged && (bits & PV_BRANCH) && (old & PV_BRANCH)) break;  // its marker goes on to the root
            }
            pos = 0xffu;
            node = t.nd_parent[node];
        }
    }
    if (p.q_status) p.q_status[j] = status;
    if (p.qk) {
        p.qk[j] = kept_k;
        p.qc[j] = kept_c;
    }
}

// key x against the d nibbles that key l starts with followed by nibble s: is x below that string?
PHANT_DEV bool pv_below(const TrieDev& t, uint32_t x, uint32_t l, uint32_t d, uint32_t s) {
    const uint32_t nx = nib_len(t, x);
    for (uint32_t j = 0; j <= d; ++j) {
        if (j >= nx) return true;  // a proper prefix
        const uint32_t a = nib_at(t, x, j), b = j < d ? nib_at(t, l, j) : s;
        if (a != b) return a < b;
    }
    return false;
}

__global__ void __launch_bounds__(256) prove_sibling_kernel(TrieDev t, ProveDev p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0 || i >= t.n) return;
    const uint32_t m = p.nmark[i];
    if (!(m & PV_BRANCH) || (m >> PV_MASK_SHIFT) == 0u) return;
    const uint32_t dn = t.dense[i];
    if (dn == NONE) return;
    uint32_t occ = t.value_key[i] != NONE ? (1u << 16) : 0u;
    for (uint32_t s = 0; s < 16u; ++s)
        if (t.slot_len[(uint64_t)dn * 16u + s]) occ |= 1u << s;
    const uint32_t rest = occ & ~(m >> PV_MASK_SHIFT);
    if (__popc(rest) != 1) return;
    const uint32_t s = (uint32_t)__builtin_ctz(rest);
    if (s == 16u || t.slot_len[(uint64_t)dn * 16u + s] != 32u) return;  // the value, or a child embedded in the branch itself
    // the first key under position s: keys of the interval are sorted, the trie ends at hi
    const uint32_t l = t.nd_l[i], d = (uint32_t)t.lcp[i];
    uint32_t a = l, b = t.seg_first[trie_of(t, l) + 1u];
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (pv_below(t, mid, l, d, s)) a = mid + 1u;
        else b = mid;
    }
    if (a >= t.n) return;
    if (t.leaf_ps[a] != BRANCH_VALUE && t.leaf_parent[a] == i) {
        p.lmark[a] = (uint8_t)(p.lmark[a] | PV_SIB_LEAF);  // (this lane is the only writer of the byte in this pass)
        return;
    }
    uint32_t node = t.leaf_parent[a];
    while (node != NONE && t.nd_parent[node] != i) node = t.nd_parent[node];
    if (node == NONE) return;
    atomicOr(&p.nmark[node], t.lcp[node] > t.nd_pd[node] + 1 ? PV_SIB_EXT : PV_SIB_BRANCH);
}

// the length of the extension over branch plan b (put_extension's arithmetic)
PHANT_DEV uint32_t pv_ext_size(const BranchPlan& b, bool inner_hashed) {
    const uint64_t xpayload = hp_rlp_size(b.ext_len) + (inner_hashed ? 33u : b.total);
    return (uint32_t)(hdr_len(xpayload) + xpayload);
}
// which nodes of index i are members, and their lengths
PHANT_DEV uint32_t pv_members(const TrieDev& t, const ProveDev& p, uint32_t i, uint32_t& xlen, uint32_t& blen, unsigned long long& llen) {
    uint32_t mem = 0;
    xlen = blen = 0;
    llen = 0;
    if (i >= t.n) return 0;
    const uint32_t m = i ? p.nmark[i] : 0u;
    if ((m & (PV_BRANCH | PV_EXT | PV_SIB_BRANCH | PV_SIB_EXT)) && t.dense[i] != NONE) {
        const BranchPlan b = branch_plan_node(t, i, true);
        const bool is_root = t.nd_parent[i] == NONE;
        const bool hashed = b.total >= 32u || (is_root && b.ext_len == 0u);
        if ((m & (PV_BRANCH | PV_SIB_BRANCH)) && hashed) {
            mem |= PV_M_BRANCH;
            blen = b.total;
        }
        if ((m & (PV_EXT | PV_SIB_EXT)) && b.ext_len) {
            const uint32_t x = pv_ext_size(b, hashed);
            if (x >= 32u || is_root) {
                mem |= PV_M_EXT;
                xlen = x;
            }
        }
    }
    if (p.lmark[i]) {
        const LeafPlan lp = leaf_plan(t, i);
        if (lp.live && (lp.total >= 32u || t.leaf_parent[i] == NONE)) {
            mem |= PV_M_LEAF;
            llen = hdr_len(lp.payload) + lp.payload;
        }
    }
    return mem;
}

__global__ void __launch_bounds__(PV_TILE) prove_size_kernel(TrieDev t, ProveDev p) {
    __shared__ uint32_t s_c[2][PV_TILE];
    __shared__ unsigned long long s_b[2][PV_TILE];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * PV_TILE + tid;
    uint32_t xlen, blen;
    unsigned long long llen;
    const uint32_t mem = pv_members(t, p, i, xlen, blen, llen);
    const uint32_t cnt = (uint32_t)__popc(mem);
    const unsigned long long bytes = (unsigned long long)xlen + blen + llen;
    if (i <= t.n) p.members[i] = (uint8_t)mem;
    s_c[0][tid] = cnt;
    s_b[0][tid] = bytes;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t o = 1; o < PV_TILE; o <<= 1) {  // inclusive scan, two buffers
        s_c[cur ^ 1u][tid] = s_c[cur][tid] + (tid >= o ? s_c[cur][tid - o] : 0u);
        s_b[cur ^ 1u][tid] = s_b[cur][tid] + (tid >= o ? s_b[cur][tid - o] : 0ull);
        cur ^= 1u;
        __syncthreads();
    }
    if (i <= t.n) {
        p.nbase[i] = s_c[cur][tid] - cnt;
        p.bbase[i] = s_b[cur][tid] - bytes;
    }
    if (tid == PV_TILE - 1u) {
        p.tile_cnt[blockIdx.x] = s_c[cur][tid];
        p.tile_bytes[blockIdx.x] = s_b[cur][tid];
    }
}

// the tiles' sums -> their exclusive prefix, in place; the totals and the error flags to the mailbox
__global__ void __launch_bounds__(PV_TILE) prove_scan_kernel(ProveDev p) {
    __shared__ uint32_t s_c[2][PV_TILE];
    __shared__ unsigned long long s_b[2][PV_TILE];
    __shared__ uint32_t s_run_c;
    __shared__ unsigned long long s_run_b;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_run_c = 0u;
        s_run_b = 0ull;
    }
    __syncthreads();
    for (uint32_t first = 0; first < p.tiles; first += PV_TILE) {
        const uint32_t q = first + tid;
        const uint32_t cnt = q < p.tiles ? p.tile_cnt[q] : 0u;
        const unsigned long long bytes = q < p.tiles ? p.tile_bytes[q] : 0ull;
        s_c[0][tid] = cnt;
        s_b[0][tid] = bytes;
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t o = 1; o < PV_TILE; o <<= 1) {
            s_c[cur ^ 1u][tid] = s_c[cur][tid] + (tid >= o ? s_c[cur][tid - o] : 0u);
            s_b[cur ^ 1u][tid] = s_b[cur][tid] + (tid >= o ? s_b[cur][tid - o] : 0ull);
            cur ^= 1u;
            __syncthreads();
        }
        if (q < p.tiles) {
            p.tile_cnt[q] = s_run_c + s_c[cur][tid] - cnt;
            p.tile_bytes[q] = s_run_b + s_b[cur][tid] - bytes;
        }
        __syncthreads();
        if (tid == PV_TILE - 1u) {
            s_run_c += s_c[cur][tid];
            s_run_b += s_b[cur][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        p.mailbox[MAILBOX_PROVE] = s_run_c;
        p.mailbox[MAILBOX_PROVE + 1u] = (uint32_t)s_run_b;
        p.mailbox[MAILBOX_PROVE + 2u] = (uint32_t)(s_run_b >> 32);
        p.mailbox[MAILBOX_PROVE + 3u] = p.flags[0];
        __threadfence_system();
    }
}

__global__ void __launch_bounds__(256) prove_base_kernel(TrieDev t, ProveDev p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > t.n) return;
    p.nbase[i] += p.tile_cnt[i / PV_TILE];
    p.bbase[i] += p.tile_bytes[i / PV_TILE];
}
__global__ void __launch_bounds__(256) prove_first_kernel(TrieDev t, ProveDev p) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s <= t.n_tries) p.trie_first_node[s] = p.nbase[t.seg_first[s]];
}

__global__ void __launch_bounds__(64) prove_emit_kernel(TrieDev t, ProveDev p) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i > t.n) return;
    uint32_t j = p.nbase[i];
    unsigned long long at = p.bbase[i];
    if (i == t.n) {
        if (p.node_off) p.node_off[j] = at;  // the end of the last node
        return;
    }
    if (!p.members[i]) return;
    uint32_t xlen, blen;
    unsigned long long llen;
    const uint32_t mem = pv_members(t, p, i, xlen, blen, llen);
    if (mem & (PV_M_EXT | PV_M_BRANCH)) {
        const BranchPlan b = branch_plan_node(t, i, true);
        const bool is_root = t.nd_parent[i] == NONE;
        const bool hashed = b.total >= 32u || (is_root && b.ext_len == 0u);
        if (mem & PV_M_EXT) {
            if (p.node_off) p.node_off[j] = at;
            if (p.nodes) {
                // the branch under it once more, in the build's scratch blob (free since the build ended), for its digest
                const unsigned long long tmp = atomicAdd(t.cursor, (unsigned long long)((b.total + 7u) & ~3u));
                if (tmp + b.total + 8u > t.scratch_cap) {
                    atomicOr(&p.flags[0], PV_ERR_SCRATCH);
                    return;
                }
                uint8_t* const enc = t.scratch + tmp;
                (void)put_branch(enc, t, b.dn, b.payload, b.v, b.vlen);
                Sponge s;
                sponge_zero(s);
                if (hashed) keccak256_global(s, enc, b.total);
                (void)put_extension(p.nodes + at, t, b.l, (uint32_t)(b.pd + 1), (uint32_t)b.d, hashed, s, enc, b.total);
            }
            ++j;
            at += xlen;
        }
        if (mem & PV_M_BRANCH) {
            if (p.node_off) p.node_off[j] = at;
            if (p.nodes) (void)put_branch(p.nodes + at, t, b.dn, b.payload, b.v, b.vlen);
            ++j;
            at += blen;
        }
    }
    if (mem & PV_M_LEAF) {
        const LeafPlan lp = leaf_plan(t, i);
        if (p.node_off) p.node_off[j] = at;
        if (p.nodes) {
            uint8_t* w = put_hdr_to(p.nodes + at, 0xc0u, lp.payload);
            w = put_hp(w, t, i, lp.ps, lp.nl, true);
            (void)put_str_wide(w, lp.v, lp.vlen);
        }
    }
}
__global__ void __launch_bounds__(64) prove_reset_kernel(TrieDev t, ProveDev p) {
    if (threadIdx.x == 0) {
        if (t.cursor) *t.cursor = 0ull;  // (no keys: no build, no arenas)
        p.flags[0] = 0u;
    }
}

// ---- the per-proof form: every query's own ordered list, cut from the emitted set ----
struct ProveBatchDev {
    uint32_t n_queries;
    const uint8_t* set_nodes;               // the node set in the prover's arena
    const unsigned long long* set_off;      // its offsets (set nodes + 1)
    uint32_t* q_cnt;                        // n_queries + 1: the first node of proof j (inside its tile until the place pass adds the tile's base)
    unsigned long long* q_bytes;            // n_queries + 1: its byte offset, likewise
    uint32_t* tile_cnt;                     // tiles + 1
    unsigned long long* tile_bytes;         // tiles + 1
    uint32_t tiles;
    uint32_t* mailbox;
    // the writing passes
    uint32_t total_nodes;
    uint32_t* src;                          // total_nodes: the set index of every output node
    unsigned long long* node_off;           // total_nodes + 1
    uint32_t* proof_first_node;             // n_queries + 1 (optional)
    uint8_t* nodes;
};

// The members on the walk of a query that shares c nibbles with key k, deepest first: visit(set index).  The conditions are the
// locate pass's own marks; members[] says which of the marked are hashed nodes, nbase[] where an index's members (extension, branch,
// leaf, in that order) stand in the set.
template <class Visit>
PHANT_DEV void pv_walk_up(const TrieDev& t, const ProveDev& p, uint32_t k, uint32_t c, Visit&& visit) {
    const uint32_t ps = t.leaf_ps[k];
    if (ps != BRANCH_VALUE && c >= ps) {
        const uint32_t mem = p.members[k];
        if (mem & PV_M_LEAF) visit(p.nbase[k] + (uint32_t)__popc(mem & (PV_M_EXT | PV_M_BRANCH)));
    }
    uint32_t node = t.leaf_parent[k];
    while (node != NONE) {
        const int32_t d = t.lcp[node], pd = t.nd_pd[node];
        const uint32_t mem = p.members[node];
        if ((int32_t)c >= d && (mem & PV_M_BRANCH)) visit(p.nbase[node] + ((mem & PV_M_EXT) ? 1u : 0u));
        if (d > pd + 1 && (int32_t)c >= pd + 1 && (mem & PV_M_EXT)) visit(p.nbase[node]);
        node = t.nd_parent[node];
    }
}

__global__ void __launch_bounds__(PV_TILE) prove_batch_count_kernel(TrieDev t, ProveDev p, ProveBatchDev b) {
    __shared__ uint32_t s_c[2][PV_TILE];
    __shared__ unsigned long long s_b[2][PV_TILE];
    const uint32_t tid = threadIdx.x;
    const unsigned long long j = (unsigned long long)blockIdx.x * PV_TILE + tid;
    uint32_t cnt = 0;
    unsigned long long bytes = 0;
    if (j < b.n_queries) {
        const uint32_t k = p.qk[j];
        if (k != NONE)
            pv_walk_up(t, p, k, p.qc[j], [&](uint32_t s) {
                ++cnt;
                bytes += b.set_off[s + 1u] - b.set_off[s];
            });
    }
    s_c[0][tid] = cnt;
    s_b[0][tid] = bytes;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t o = 1; o < PV_TILE; o <<= 1) {  // inclusive scan, two buffers
        s_c[cur ^ 1u][tid] = s_c[cur][tid] + (tid >= o ? s_c[cur][tid - o] : 0u);
        s_b[cur ^ 1u][tid] = s_b[cur][tid] + (tid >= o ? s_b[cur][tid - o] : 0ull);
        cur ^= 1u;
        __syncthreads();
    }
    if (j <= b.n_queries) {
        b.q_cnt[j] = s_c[cur][tid] - cnt;
        b.q_bytes[j] = s_b[cur][tid] - bytes;
    }
    if (tid == PV_TILE - 1u) {
        b.tile_cnt[blockIdx.x] = s_c[cur][tid];  // (keys of at most 255 bytes: a walk passes fewer than 2^11 nodes, a tile's 1 024 walks fit 32 bits)
        b.tile_bytes[blockIdx.x] = s_b[cur][tid];
    }
}

// the tiles' sums -> their exclusive prefix, in place; the totals to the mailbox.  The node total is kept in 64 bits: the host
// refuses one beyond 2^32 - 1, and nobody reads the (wrapped) prefixes then.
__global__ void __launch_bounds__(PV_TILE) prove_batch_scan_kernel(ProveBatchDev b) {
    __shared__ uint32_t s_c[2][PV_TILE];
    __shared__ unsigned long long s_b[2][PV_TILE];
    __shared__ unsigned long long s_run_c, s_run_b;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_run_c = 0ull;
        s_run_b = 0ull;
    }
    __syncthreads();
    for (uint32_t first = 0; first < b.tiles; first += PV_TILE) {
        const uint32_t q = first + tid;
        const uint32_t cnt = q < b.tiles ? b.tile_cnt[q] : 0u;
        const unsigned long long bytes = q < b.tiles ? b.tile_bytes[q] : 0ull;
        s_c[0][tid] = cnt;
        s_b[0][tid] = bytes;
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t o = 1; o < PV_TILE; o <<= 1) {
            s_c[cur ^ 1u][tid] = s_c[cur][tid] + (tid >= o ? s_c[cur][tid - o] : 0u);
            s_b[cur ^ 1u][tid] = s_b[cur][tid] + (tid >= o ? s_b[cur][tid - o] : 0ull);
            cur ^= 1u;
            __syncthreads();
        }
        if (q < b.tiles) {
            b.tile_cnt[q] = (uint32_t)s_run_c + s_c[cur][tid] - cnt;
            b.tile_bytes[q] = s_run_b + s_b[cur][tid] - bytes;
        }
        __syncthreads();
        if (tid == PV_TILE - 1u) {
            s_run_c += s_c[cur][tid];  // (1 024 tiles' sums, each below 2^21, stay below 2^32)
            s_run_b += s_b[cur][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        b.mailbox[MAILBOX_PROVE_BATCH] = (uint32_t)s_run_c;
        b.mailbox[MAILBOX_PROVE_BATCH + 1u] = (uint32_t)(s_run_c >> 32);
        b.mailbox[MAILBOX_PROVE_BATCH + 2u] = (uint32_t)s_run_b;
        b.mailbox[MAILBOX_PROVE_BATCH + 3u] = (uint32_t)(s_run_b >> 32);
        __threadfence_system();
    }
}

__global__ void __launch_bounds__(256) prove_batch_place_kernel(TrieDev t, ProveDev p, ProveBatchDev b) {
    const unsigned long long j = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (j > b.n_queries) return;
    const uint32_t first = b.q_cnt[j] + b.tile_cnt[j / PV_TILE];
    if (b.proof_first_node) b.proof_first_node[j] = first;
    if (j == b.n_queries) {
        b.node_off[first] = b.q_bytes[j] + b.tile_bytes[j / PV_TILE];  // the end of the last node
        return;
    }
    const uint32_t k = p.qk[j];
    if (k == NONE) return;
    // filled from the proof's end: the climb meets the deepest node first
    uint32_t at = b.q_cnt[j + 1u] + b.tile_cnt[(j + 1u) / PV_TILE];
    unsigned long long end = b.q_bytes[j + 1u] + b.tile_bytes[(j + 1u) / PV_TILE];
    pv_walk_up(t, p, k, p.qc[j], [&](uint32_t s) {
        end -= b.set_off[s + 1u] - b.set_off[s];
        --at;
        b.node_off[at] = end;
        b.src[at] = s;
    });
}

// A wave per output node.  Both ends sit at any byte address: the bytes up to the destination's next 16-byte boundary and the
// last (length - head) % 16 go a byte a lane, what lies between as unaligned 16-byte loads (absorb.hip.h) and aligned 16-byte stores.
__global__ void __launch_bounds__(256) prove_batch_gather_kernel(ProveBatchDev b) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long o = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (o >= b.total_nodes) return;
    const uint32_t s = b.src[o];
    const unsigned long long from = b.set_off[s], len = b.set_off[s + 1u] - from;
    const uint8_t* __restrict__ const src = b.set_nodes + from;
    uint8_t* __restrict__ const dst = b.nodes + b.node_off[o];
    unsigned long long head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const unsigned long long body_end = head + ((len - head) & ~15ull);
    for (unsigned long long at = head + 16u * lane; at < body_end; at += 16u * 64u) {
        const PackedU32x4 v = *reinterpret_cast<const PackedU32x4*>(src + at);
        *reinterpret_cast<uint4*>(dst + at) = make_uint4(v.x, v.y, v.z, v.w);
    }
    if (body_end + lane < len) dst[body_end + lane] = src[body_end + lane];  // (fewer than 16 are left)
}
