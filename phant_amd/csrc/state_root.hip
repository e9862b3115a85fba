// state_root.hip -- the `StateDB.root()` the reference leaves as a TODO
// (src/blockchain/blockchain.zig:83-85), over the AccountState fields of
// src/state/types.zig:13-20.
//
// Secure trie: account key keccak256(addr), value
// rlp([nonce, balance, storageRoot, keccak256(code)]); storage key
// keccak256(be32(slot)), value rlp(minimal-BE(value)); zero-valued slots do not
// exist (src/state/statedb.zig:112-119).
//
// Device-resident since round 2: the caller's arrays are copied to the GPU once and everything between them and the
// root happens there -- the live slots are picked out (flag, prefix sum, compaction), their keys and the addresses
// hashed, the hashed keys ordered (radix_sort.hip: per account for the slots, one run for the accounts), the leaves of
// all storage tries written in that order (RLP of the minimal big-endian value), ONE forest pass over them
// (trie_build.hip) for the storage roots, the account leaves rlp([nonce, balance, storageRoot, codeHash]) written in key
// order, a second pass for the state trie.  The host reads back a handful of counters (how many live slots, how many
// value bytes, "is the order decided": each a stream synchronisation) and, for the state root, 32 bytes.
// Round 1 hashed on the GPU and did the rest on the host: five pageable round trips of digests and leaves, std::sort with
// 32-byte memcmp, byte-wise packing -- 121 ms per 200 000 accounts x 5 slots against 9.8 ms now (tools/bench_state.py).
//
// HBM-bound byte shuffling around the Keccak kernels; nothing here is GEMM-shaped.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <array>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/phant_gpu.h"
#include "launch.h"
#include "rlp.h"
#include "staging.h"
#include "trie_build.h"
#include "witness.h"

namespace phant {
namespace {

#define SR_TRY(call)                                                          \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            err = std::string(#call) + ": " + hipGetErrorString(e_);          \
            return e_ == hipErrorOutOfMemory ? PHANT_E_OOM : PHANT_E_DEVICE;  \
        }                                                                     \
    } while (0)

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// ------------------------------------------------------------------ kernels
// bytes of the minimal big-endian form of a 32-byte value (0 for zero); v is 4-byte aligned.  rlp.h's be_bytes(v, 32) says the same
// byte by byte; this dword form relies on the alignment, which that one must not assume, and stays here.
__device__ __forceinline__ uint32_t be_len32(const uint8_t* v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(v);
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t x = __builtin_bswap32(w[i]);  // most significant byte first
        if (x) return 32u - 4u * i - (uint32_t)(__builtin_clz(x) >> 3);
    }
    return 0u;
}
// length of rlp(the integer in the 32 bytes at v), whose minimal form has vl bytes
__device__ __forceinline__ uint32_t rlp_be32_len(const uint8_t* v, uint32_t vl) { return (uint32_t)str_len(vl, vl == 1u ? v[31] : 0u); }

// live[s] = 1 iff slot s holds a non-zero value (statedb.zig:112-119: zero = absent); live[m] = 0 (the scan's total lands there)
__global__ void __launch_bounds__(256) slot_live_kernel(const uint8_t* __restrict__ slot_vals, uint32_t m, uint32_t* __restrict__ live) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > m) return;
    live[s] = s < m ? (be_len32(slot_vals + 32ull * s) != 0u) : 0u;
}

// pos = exclusive scan of live: live slot s becomes storage leaf pos[s] (before ordering): its key, where it came from, whose it is
__global__ void __launch_bounds__(256) slot_compact_kernel(const uint32_t* __restrict__ pos, const uint8_t* __restrict__ slot_keys,
                                                           const uint32_t* __restrict__ slot_first, uint32_t n_acc, uint32_t m,
                                                           uint8_t* __restrict__ live_keys, uint32_t* __restrict__ live_src,
                                                           uint32_t* __restrict__ seg_of) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= m || pos[s + 1] == pos[s]) return;
    const uint32_t j = pos[s];
    const uint4* k = reinterpret_cast<const uint4*>(slot_keys + 32ull * s);
    uint4* o = reinterpret_cast<uint4*>(live_keys + 32ull * j);
    o[0] = k[0];
    o[1] = k[1];
    live_src[j] = s;
    // the account a with slot_first[a] <= s < slot_first[a + 1]: the last a whose first slot is not behind s
    uint32_t lo = 0, hi = n_acc;  // invariant: slot_first[lo] <= s, answer in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (slot_first[mid] <= s) lo = mid;
        else hi = mid;
    }
    seg_of[j] = lo;
}

// storage trie a owns leaves [acc_first[a], acc_first[a + 1])
__global__ void __launch_bounds__(256) acc_first_kernel(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ slot_first, uint32_t n_acc,
                                                        uint32_t* __restrict__ acc_first) {
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a <= n_acc) acc_first[a] = pos[slot_first[a]];
}

// leaf j of the ordered storage leaves: length of rlp(minimal big-endian value); len[L] = 0
__global__ void __launch_bounds__(256) slot_leaf_len_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ live_src,
                                                            const uint8_t* __restrict__ slot_vals, uint32_t L, uint32_t* __restrict__ len) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j > L) return;
    uint32_t l = 0;
    if (j < L) {
        const uint8_t* v = slot_vals + 32ull * live_src[order[j]];
        const uint32_t vl = be_len32(v);
        l = rlp_be32_len(v, vl);
    }
    len[j] = l;
}

__global__ void __launch_bounds__(256) slot_leaf_write_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ live_src,
                                                              const uint8_t* __restrict__ slot_vals, const uint8_t* __restrict__ hk,
                                                              const uint32_t* __restrict__ off, uint32_t L, uint8_t* __restrict__ skeys,
                                                              uint32_t* __restrict__ skoff, uint8_t* __restrict__ svals,
                                                              uint64_t* __restrict__ svoff) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j > L) return;
    skoff[j] = 32u * j;
    svoff[j] = off[j];
    if (j == L) return;
    const uint32_t src = order[j];
    const uint4* k = reinterpret_cast<const uint4*>(hk + 32ull * src);
    uint4* o = reinterpret_cast<uint4*>(skeys + 32ull * j);
    o[0] = k[0];
    o[1] = k[1];
    const uint8_t* v = slot_vals + 32ull * live_src[src];
    const uint32_t vl = be_len32(v);
    (void)put_str(svals + off[j], v + (32u - vl), vl);
}

// account leaf i (key order): length of rlp([nonce, balance, storageRoot, codeHash]); len[n] = 0
__global__ void __launch_bounds__(256) account_len_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ nonces,
                                                          const uint8_t* __restrict__ balances, uint32_t n, uint32_t* __restrict__ len) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    uint32_t l = 0;
    if (i < n) {
        const uint32_t a = order[i];
        const uint8_t* bv = balances + 32ull * a;
        const uint32_t payload = uint_len(nonces[a]) + rlp_be32_len(bv, be_len32(bv)) + 33u + 33u;
        l = hdr_len(payload) + payload;
    }
    len[i] = l;
}

__global__ void __launch_bounds__(256) account_write_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ nonces,
                                                            const uint8_t* __restrict__ balances, const uint8_t* __restrict__ sroots,
                                                            const uint8_t* __restrict__ hc, const uint8_t* __restrict__ ha,
                                                            const uint32_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ akeys,
                                                            uint32_t* __restrict__ akoff, uint8_t* __restrict__ avals,
                                                            uint64_t* __restrict__ avoff) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    akoff[i] = 32u * i;
    avoff[i] = off[i];
    if (i == n) return;
    const uint32_t a = order[i];
    const uint4* k = reinterpret_cast<const uint4*>(ha + 32ull * a);
    uint4* ko = reinterpret_cast<uint4*>(akeys + 32ull * i);
    ko[0] = k[0];
    ko[1] = k[1];
    const uint8_t* bv = balances + 32ull * a;
    const uint32_t bl = be_len32(bv);
    const uint32_t payload = uint_len(nonces[a]) + rlp_be32_len(bv, bl) + 33u + 33u;
    uint8_t* o = avals + off[i];
    o += put_hdr(o, 0xc0u, payload);
    o += put_uint(o, nonces[a]);
    o += put_str(o, bv + (32u - bl), bl);
    o += put_str(o, sroots + 32ull * a, 32u);
    (void)put_str(o, hc + 32ull * a, 32u);
}

// ------------------------------------------------------------------ host side
// the permutation radix_sort.hip left undecided (64-bit prefixes tie / keys repeat), made on the host instead
int32_t order_on_host(const TrieTune& tune, hipStream_t st, const uint8_t* d_digests, const uint32_t* d_seg_of, uint32_t n, uint32_t* d_order, std::string& err) {
    if (tune.sort_no_fallback) {  // tests: prove which path ordered the batch
        err = "device sort undecided (64-bit key prefixes tie or keys repeat)";
        return PHANT_E_UNSUPPORTED;
    }
    std::vector<uint8_t> dg((size_t)n * 32);
    std::vector<uint32_t> seg(d_seg_of ? n : 0), order(n);
    SR_TRY(hipMemcpyAsync(dg.data(), d_digests, dg.size(), hipMemcpyDeviceToHost, st));
    if (d_seg_of) SR_TRY(hipMemcpyAsync(seg.data(), d_seg_of, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (d_seg_of && seg[x] != seg[y]) return seg[x] < seg[y];
        return std::memcmp(&dg[(size_t)x * 32], &dg[(size_t)y * 32], 32) < 0;
    });
    SR_TRY(hipMemcpyAsync(d_order, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    SR_TRY(hipStreamSynchronize(st));  // (`order` goes out of scope)
    return PHANT_OK;
}

// digests (device) -> their order in device memory by the device sort, WITHOUT waiting for its verdict: the order is used at
// once, *d_flag is read back by the caller together with whatever it reads back next anyway; a set flag (ties in the 64-bit
// prefixes: never, unless someone ground keys for it) means order_on_host and the work since then again.
int32_t order_digests_async(const TrieTune& tune, hipStream_t st, const uint8_t* d_digests, const uint32_t* d_seg_of, uint32_t n, uint32_t n_seg, uint8_t* d_sort_ws,
                            uint32_t** d_order, uint32_t** d_flag, std::string& err) {
    uint32_t prefix_bits = 0;  // (the sort's own choice; a number -- tests -- means that many bits and no repair of ties)
    if (tune.sort_prefix_bits >= 0) prefix_bits = (uint32_t)tune.sort_prefix_bits;
    if (tune.sort_repair_bits >= 0) prefix_bits = (uint32_t)tune.sort_repair_bits | 0x80000000u;  // (tests: few bits, ties repaired)
    SR_TRY(launch_order_digests(d_digests, d_seg_of, n, n_seg, d_sort_ws, d_order, d_flag, prefix_bits, st));
    return PHANT_OK;
}

// the state trie's leaves in device memory (inside ws.io: valid until the next call that lays something out there)
struct DevLeaves {
    uint8_t* keys = nullptr;      // n x 32, ascending
    uint32_t* key_off = nullptr;  // n + 1
    uint8_t* vals = nullptr;
    uint64_t* val_off = nullptr;  // n + 1
    uint64_t val_bytes = 0;
    uint32_t n = 0;
    uint32_t* seg = nullptr;      // {0, n}: the one trie's segment table (room for 17 entries: the sixteen sub-tries')
    uint8_t* root = nullptr;      // 32 bytes for the caller's forest pass
    uint8_t* code_hash = nullptr; // n x 32, in the caller's account order
    TriePairs pairs(uint32_t n_tries = 1) const { return {keys, key_off, 32ull * n, vals, val_off, val_bytes, n, seg, n_tries, root}; }
};

// phant_state_witness: the slot queries the storage forest is proven for while its tables stand (the state trie's pass reuses
// them).  Trie t of that forest is the caller's account t.  The nodes come back in host memory.
struct StateProve {
    std::vector<uint8_t> slot_pre;    // ns x 32 slot preimages
    std::vector<uint32_t> slot_trie;  // ns
    std::vector<uint8_t> slot_flags;  // ns
    std::vector<uint8_t> nodes;
    std::vector<uint64_t> node_off{0};
    // phant_state_proofs: an ordered list per slot query instead (slot_flags is not read): query j = nodes [first[j], first[j + 1])
    bool per_proof = false;
    std::vector<uint32_t> first{0};
};

// the queries' trie keys: 32-byte digests back to back
__global__ void __launch_bounds__(256) query_offsets_kernel(uint32_t nq, uint32_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= nq) off[i] = 32u * i;
}

// dst[32 j ..] = src[32 idx[j] ..]: the code hashes of the touched accounts
__global__ void __launch_bounds__(256) gather32_kernel(const uint8_t* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t cnt,
                                                       uint8_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= 32ull * cnt) return;
    dst[i] = src[32ull * idx[i >> 5] + (i & 31u)];
}

constexpr uint32_t SUBTRIE_CAP_MAX = 256;  // state_subtrie_nodes_host: the longest root node it hands back

// Everything a state call keeps in ws.io, sized and carved by this one list: the counts in front decide which parts there are.
struct StateLayout {
    uint32_t n = 0, m = 0;    // accounts, slots
    uint64_t code_bytes = 0;
    bool host_form = false;   // the caller's arrays are copied in here (else: the device form's flag word)
    uint32_t ns = 0;          // phant_state_witness: slot queries against the storage forest (StateProve)
    bool witness = false;     // ... and the touched accounts' arrays
    uint32_t na = 0;
    size_t subtrie_out = 0;   // state_subtrie_nodes_host: bytes of its output block
    // the caller's arrays (host form)
    uint8_t *addrs = nullptr, *bal = nullptr, *code = nullptr, *skeys_in = nullptr, *svals_in = nullptr;
    uint64_t *nonces = nullptr, *code_off = nullptr;
    uint32_t *slot_first = nullptr, *flag = nullptr;
    // storage: live slots -> hashed keys -> per-account order -> leaves
    uint32_t *acc_first = nullptr, *pos = nullptr, *live_src = nullptr, *seg_of = nullptr, *len = nullptr, *lkoff = nullptr, *scan = nullptr;
    uint8_t *live_keys = nullptr, *hk = nullptr, *sort = nullptr, *lkeys = nullptr, *lvals = nullptr, *sroots = nullptr;
    uint64_t *lvoff = nullptr;
    // the slot queries
    uint8_t *qpre = nullptr, *qkeys = nullptr, *qflags = nullptr;
    uint32_t *qoff = nullptr, *qtrie = nullptr;
    // accounts: hashed addresses, code hashes, leaves
    uint8_t *ha = nullptr, *hc = nullptr, *akeys = nullptr, *avals = nullptr, *root = nullptr;
    uint32_t *alen = nullptr, *akoff = nullptr, *seg = nullptr;
    uint64_t *avoff = nullptr;
    uint8_t *sub_out = nullptr;
    // the touched accounts
    uint8_t *apre = nullptr, *tkeys = nullptr, *aflags = nullptr, *thc = nullptr;
    uint32_t *aoff = nullptr, *held = nullptr;

    template <class A>
    void carve(A& a) {
        const size_t n1 = (size_t)n + 1, m1 = (size_t)m + 1, big = m > n ? m : n;
        if (host_form) {
            addrs = a.template take<uint8_t>(20 * (size_t)n + 16);
            nonces = a.template take<uint64_t>(n);
            bal = a.template take<uint8_t>(32 * (size_t)n);
            code = a.template take<uint8_t>(code_bytes + 16);
            code_off = a.template take<uint64_t>(n1);
            skeys_in = a.template take<uint8_t>(32 * (size_t)m + 16);
            svals_in = a.template take<uint8_t>(32 * (size_t)m + 16);
            slot_first = a.template take<uint32_t>(n1);
        } else {
            flag = a.template take<uint32_t>(1);
        }
        acc_first = a.template take<uint32_t>(n1);
        pos = a.template take<uint32_t>(m1);
        live_keys = a.template take<uint8_t>(32 * (size_t)m + 16);
        live_src = a.template take<uint32_t>(m1);
        seg_of = a.template take<uint32_t>(m1);
        hk = a.template take<uint8_t>(32 * (size_t)m + 16);
        sort = a.template take<uint8_t>(order_workspace_bytes((uint32_t)big));
        len = a.template take<uint32_t>(m1);
        lkeys = a.template take<uint8_t>(32 * (size_t)m + 16);
        lkoff = a.template take<uint32_t>(m1);
        lvals = a.template take<uint8_t>(33 * (size_t)m + 16);
        lvoff = a.template take<uint64_t>(m1);
        sroots = a.template take<uint8_t>(32 * (size_t)n);
        scan = a.template take<uint32_t>(scan_scratch_entries((uint32_t)big + 1u));
        if (ns) {
            qpre = a.template take<uint8_t>(32 * (size_t)ns + 16);
            qkeys = a.template take<uint8_t>(32 * (size_t)ns + 16);
            qoff = a.template take<uint32_t>((size_t)ns + 1);
            qtrie = a.template take<uint32_t>((size_t)ns + 1);
            qflags = a.template take<uint8_t>((size_t)ns + 1);
        }
        ha = a.template take<uint8_t>(32 * (size_t)n);
        hc = a.template take<uint8_t>(32 * (size_t)n);
        alen = a.template take<uint32_t>(n1);
        akeys = a.template take<uint8_t>(32 * (size_t)n + 16);
        akoff = a.template take<uint32_t>(n1);
        avals = a.template take<uint8_t>(112 * (size_t)n + 16);
        avoff = a.template take<uint64_t>(n1);
        seg = a.template take<uint32_t>(17);
        root = a.template take<uint8_t>(32);
        if (subtrie_out) sub_out = a.template take<uint8_t>(subtrie_out);
        if (witness) {
            apre = a.template take<uint8_t>(20 * (size_t)na + 16);
            tkeys = a.template take<uint8_t>(32 * (size_t)na + 16);
            aoff = a.template take<uint32_t>((size_t)na + 1);
            aflags = a.template take<uint8_t>((size_t)na + 1);
            held = a.template take<uint32_t>((size_t)na + 1);
            thc = a.template take<uint8_t>(32 * (size_t)na + 16);
        }
    }
};
// (the stream is synchronised before the arena grows; a call that fits what is there pays nothing)
int32_t lay_out_state(Workspaces& ws, hipStream_t st, StateLayout& lay, std::string& err) {
    if ((uint64_t)lay.n * 112u > 0xffffffffull || (uint64_t)lay.m * 33u > 0xffffffffull) {  // (leaf offsets are scanned as 32-bit counters)
        err = "state root: more than 4 GiB of leaves in one call";
        return PHANT_E_UNSUPPORTED;
    }
    return lay_out_status(lay_out_arena(ws.io, st, [&](auto& a) { lay.carve(a); }), "state root", "io", err);
}

// device-resident inputs -> the state trie's leaves in device memory (everything else in ws.io, as `lay` was laid out there)
int32_t state_leaves_core(Workspaces& ws, hipStream_t st, const StateIn& in, const StateLayout& lay, DevLeaves& out, std::string& err,
                          StateProve* pv = nullptr) {
    const uint32_t n = in.n, m = in.m;
    const size_t n1 = (size_t)n + 1, m1 = (size_t)m + 1;
    const uint8_t* d_addrs = in.addrs;
    const uint64_t* d_nonces = in.nonces;
    const uint8_t* d_bal = in.bal;
    const uint8_t* d_code = in.code;
    const uint64_t* d_code_off = in.code_off;
    const uint8_t* d_skeys_in = in.skeys;
    const uint8_t* d_svals_in = in.svals;
    const uint32_t* d_slot_first = in.slot_first;

    // ---- storage: live slots -> hashed keys -> per-account order -> leaves -> one forest pass ----
    uint32_t *const d_acc_first = lay.acc_first, *const d_pos = lay.pos, *const d_live_src = lay.live_src, *const d_seg_of = lay.seg_of;
    uint32_t *const d_len = lay.len, *const d_lkoff = lay.lkoff, *const d_scan = lay.scan;
    uint8_t *const d_live_keys = lay.live_keys, *const d_hk = lay.hk, *const d_sort = lay.sort, *const d_lkeys = lay.lkeys;
    uint8_t *const d_lvals = lay.lvals, *const d_sroots = lay.sroots;
    uint64_t* const d_lvoff = lay.lvoff;
    // what the host reads back on the way goes through the ctx's pinned mailbox (a copy into pageable memory is ~25 us a piece);
    // the words behind the trie builder's
    SR_TRY(ws.ensure_mailbox());
    volatile uint32_t* const mb = ws.mailbox + 640;
    hipLaunchKernelGGL(slot_live_kernel, dim3(blocks(m1)), dim3(256), 0, st, d_svals_in, m, d_pos);
    SR_TRY(launch_exclusive_scan_u32(d_pos, m + 1u, d_scan, st));
    SR_TRY(hipMemcpyAsync(const_cast<uint32_t*>(mb), d_pos + m, 4, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(acc_first_kernel, dim3(blocks(n1)), dim3(256), 0, st, d_pos, d_slot_first, n, d_acc_first);
    if (m) hipLaunchKernelGGL(slot_compact_kernel, dim3(blocks(m)), dim3(256), 0, st, d_pos, d_skeys_in, d_slot_first, n, m, d_live_keys, d_live_src, d_seg_of);
    SR_TRY(hipStreamSynchronize(st));
    const uint32_t L = mb[0];
    uint64_t leaf_bytes = 0;
    if (L) {
        SR_TRY(launch_keccak256_fixed(d_live_keys, 32, 32, L, d_hk, st));
        uint32_t* d_order = nullptr;
        uint32_t* d_flag = nullptr;
        int32_t rc = order_digests_async(ws.tune, st, d_hk, d_seg_of, L, n, d_sort, &d_order, &d_flag, err);
        if (rc) return rc;
        for (int pass = 0; pass < 2; ++pass) {  // (a second time only behind the host's ordering)
            hipLaunchKernelGGL(slot_leaf_len_kernel, dim3(blocks((uint64_t)L + 1)), dim3(256), 0, st, d_order, d_live_src, d_svals_in, L, d_len);
            SR_TRY(launch_exclusive_scan_u32(d_len, L + 1u, d_scan, st));
            SR_TRY(hipMemcpyAsync(const_cast<uint32_t*>(mb), d_len + L, 4, hipMemcpyDeviceToHost, st));
            SR_TRY(hipMemcpyAsync(const_cast<uint32_t*>(mb + 1), d_flag, 4, hipMemcpyDeviceToHost, st));
            hipLaunchKernelGGL(slot_leaf_write_kernel, dim3(blocks((uint64_t)L + 1)), dim3(256), 0, st, d_order, d_live_src, d_svals_in, d_hk, d_len, L,
                               d_lkeys, d_lkoff, d_lvals, d_lvoff);
            SR_TRY(hipStreamSynchronize(st));
            leaf_bytes = mb[0];
            if (pass || !mb[1]) break;
            if ((rc = order_on_host(ws.tune, st, d_hk, d_seg_of, L, d_order, err)) != PHANT_OK) return rc;
            SR_TRY(hipMemsetAsync(d_flag, 0, 4, st));
        }
    }
    int32_t rc;
    const uint32_t ns = pv ? (uint32_t)pv->slot_trie.size() : 0u;
    const TriePairs storage{d_lkeys, d_lkoff, 32ull * L, d_lvals, d_lvoff, leaf_bytes, L, d_acc_first, n, d_sroots};
    if (ns && L) {  // the same pass with its tables kept, and the touched slots' paths cut from it (no live slot: no storage node)
        SR_TRY(hipMemcpyAsync(lay.qpre, pv->slot_pre.data(), 32 * (size_t)ns, hipMemcpyHostToDevice, st));
        SR_TRY(hipMemcpyAsync(lay.qtrie, pv->slot_trie.data(), 4 * (size_t)ns, hipMemcpyHostToDevice, st));
        if (!pv->per_proof) SR_TRY(hipMemcpyAsync(lay.qflags, pv->slot_flags.data(), ns, hipMemcpyHostToDevice, st));
        SR_TRY(launch_keccak256_fixed(lay.qpre, 32, 32, ns, lay.qkeys, st));
        hipLaunchKernelGGL(query_offsets_kernel, dim3(blocks((uint64_t)ns + 1)), dim3(256), 0, st, ns, lay.qoff);
        rc = prove_collect(ws, st, storage, ProveQueries{lay.qkeys, lay.qoff, lay.qtrie, pv->per_proof ? nullptr : lay.qflags, ns}, pv->nodes, pv->node_off,
                           pv->per_proof ? &pv->first : nullptr, err);
    } else {
        rc = trie_forest_dev(ws, st, storage, err);
    }
    if (rc) return rc;

    // ---- accounts: hashed addresses in order, code hashes, leaves ----
    uint8_t *const d_ha = lay.ha, *const d_hc = lay.hc;
    uint32_t* const d_alen = lay.alen;
    out.keys = lay.akeys;
    out.key_off = lay.akoff;
    out.vals = lay.avals;
    out.val_off = lay.avoff;
    out.n = n;
    out.seg = lay.seg;
    out.root = lay.root;
    SR_TRY(launch_keccak256_fixed(d_addrs, 20, 20, n, d_ha, st));
    SR_TRY(launch_keccak256_var(d_code, d_code_off, n, d_hc, st));
    out.code_hash = d_hc;
    uint32_t* d_aorder = nullptr;
    uint32_t* d_aflag = nullptr;
    rc = order_digests_async(ws.tune, st, d_ha, nullptr, n, 1, d_sort, &d_aorder, &d_aflag, err);
    if (rc) return rc;
    const uint32_t seg[2] = {0u, n};
    SR_TRY(hipMemcpyAsync(out.seg, seg, sizeof seg, hipMemcpyHostToDevice, st));
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(account_len_kernel, dim3(blocks(n1)), dim3(256), 0, st, d_aorder, d_nonces, d_bal, n, d_alen);
        SR_TRY(launch_exclusive_scan_u32(d_alen, n + 1u, d_scan, st));
        SR_TRY(hipMemcpyAsync(const_cast<uint32_t*>(mb), d_alen + n, 4, hipMemcpyDeviceToHost, st));
        SR_TRY(hipMemcpyAsync(const_cast<uint32_t*>(mb + 1), d_aflag, 4, hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(account_write_kernel, dim3(blocks(n1)), dim3(256), 0, st, d_aorder, d_nonces, d_bal, d_sroots, d_hc, d_ha, d_alen, n, out.keys,
                           out.key_off, out.vals, out.val_off);
        SR_TRY(hipStreamSynchronize(st));  // (and `seg` may go)
        out.val_bytes = mb[0];
        if (pass || !mb[1]) break;
        if ((rc = order_on_host(ws.tune, st, d_ha, nullptr, n, d_aorder, err)) != PHANT_OK) return rc;
        SR_TRY(hipMemsetAsync(d_aflag, 0, 4, st));
    }
    SR_TRY(hipGetLastError());
    return PHANT_OK;
}

// the caller's HOST arrays -> copied in once -> state_leaves_core; `lay` comes with the caller's own parts (ns, witness, subtrie_out)
// set.  A copy per array and a synchronisation: a state is rarely small, and its arrays are followed by scratch.
int32_t state_leaves_dev(Workspaces& ws, hipStream_t st, const StateIn& h, StateLayout& lay, DevLeaves& out, std::string& err, StateProve* pv = nullptr) {
    const uint32_t n = h.n;
    for (uint32_t a = 0; a < n; ++a) {
        if (h.slot_first[a + 1] < h.slot_first[a]) {
            err = "slot_first not monotone";
            return PHANT_E_INVALID_ARG;
        }
        if (h.code_off[a + 1] < h.code_off[a]) {
            err = "code_off not monotone";
            return PHANT_E_INVALID_ARG;
        }
    }
    const uint32_t m = h.slot_first[n] - h.slot_first[0];
    const uint64_t code_bytes = h.code_off[n] - h.code_off[0];
    const size_t n1 = (size_t)n + 1;
    lay.n = n, lay.m = m, lay.code_bytes = code_bytes, lay.host_form = true;
    const int32_t rc = lay_out_state(ws, st, lay, err);
    if (rc) return rc;
    SR_TRY(hipMemcpyAsync(lay.addrs, h.addrs, 20 * (size_t)n, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemcpyAsync(lay.nonces, h.nonces, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemcpyAsync(lay.bal, h.bal, 32 * (size_t)n, hipMemcpyHostToDevice, st));
    if (code_bytes) SR_TRY(hipMemcpyAsync(lay.code, h.code + h.code_off[0], code_bytes, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> rel_code(n1);
    std::vector<uint32_t> rel_slot(n1);
    for (size_t i = 0; i < n1; ++i) {
        rel_code[i] = h.code_off[i] - h.code_off[0];
        rel_slot[i] = h.slot_first[i] - h.slot_first[0];
    }
    SR_TRY(hipMemcpyAsync(lay.code_off, rel_code.data(), 8 * n1, hipMemcpyHostToDevice, st));
    SR_TRY(hipMemcpyAsync(lay.slot_first, rel_slot.data(), 4 * n1, hipMemcpyHostToDevice, st));
    if (m) {
        SR_TRY(hipMemcpyAsync(lay.skeys_in, h.skeys + 32ull * h.slot_first[0], 32 * (size_t)m, hipMemcpyHostToDevice, st));
        SR_TRY(hipMemcpyAsync(lay.svals_in, h.svals + 32ull * h.slot_first[0], 32 * (size_t)m, hipMemcpyHostToDevice, st));
    }
    SR_TRY(hipStreamSynchronize(st));  // (the rel_* vectors may go; the core synchronises within microseconds anyway)
    const StateIn in{lay.addrs, lay.nonces, lay.bal, lay.code, lay.code_off, lay.skeys_in, lay.svals_in, lay.slot_first, n, m, code_bytes};
    return state_leaves_core(ws, st, in, lay, out, err, pv);
}

// device form: what only the device can see -- offsets that go backwards or do not span what the caller says
__global__ void __launch_bounds__(256) state_offsets_check_kernel(const uint64_t* __restrict__ code_off, const uint32_t* __restrict__ slot_first,
                                                                  uint32_t n, uint32_t m, uint64_t code_bytes, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n) return;
    bool bad = false;
    if (i == 0) bad = code_off[0] != 0ull || slot_first[0] != 0u || code_off[n] != code_bytes || slot_first[n] != m;
    if (i < n) bad = bad || code_off[i + 1] < code_off[i] || slot_first[i + 1] < slot_first[i];
    if (bad) *flag = 1u;
}

// sixteen sub-tries by the top nibble of the (sorted, 32-byte) keys: seg[x] = first key whose top nibble is >= x, seg[16] = n
__global__ void __launch_bounds__(64) nibble_segments_kernel(const uint8_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ seg) {
    const uint32_t x = threadIdx.x;
    if (x > 16u) return;
    uint32_t lo = 0, hi = n;  // first i with (keys[32 i] >> 4) >= x
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)(keys[32ull * mid] >> 4) < x) lo = mid + 1u;
        else hi = mid;
    }
    seg[x] = x == 16u ? n : lo;
}

}  // namespace

// The leaves of the state trie: keys = keccak256(address), ascending; values = rlp([nonce, balance, storageRoot,
// codeHash]) with the storage roots computed here (one forest pass over all accounts' live slots).
int32_t state_leaves_host(Workspaces& ws, hipStream_t st, const StateIn& in, std::vector<uint8_t>& akeys, std::vector<uint8_t>& avals,
                          std::vector<uint64_t>& avoff, std::string& err) {
    const uint32_t n = in.n;
    akeys.clear();
    avals.clear();
    avoff.assign((size_t)n + 1, 0);
    if (n == 0) return PHANT_OK;
    StateLayout lay;
    DevLeaves l;
    const int32_t rc = state_leaves_dev(ws, st, in, lay, l, err);
    if (rc) return rc;
    akeys.resize((size_t)n * 32);
    avals.resize(l.val_bytes);
    SR_TRY(hipMemcpyAsync(akeys.data(), l.keys, akeys.size(), hipMemcpyDeviceToHost, st));
    if (l.val_bytes) SR_TRY(hipMemcpyAsync(avals.data(), l.vals, l.val_bytes, hipMemcpyDeviceToHost, st));
    SR_TRY(hipMemcpyAsync(avoff.data(), l.val_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    return PHANT_OK;
}

// StateDB.root() over DEVICE-resident struct-of-arrays: nothing of the state crosses the bus, the root stays on the device.
int32_t state_root_dev(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t* d_root, std::string& err) {
    const uint32_t n = in.n;
    if (n == 0) {
        uint8_t root[32];
        const int32_t rc = trie_forest_host(ws, st, HostPairs{}, root, err);
        if (rc) return rc;
        SR_TRY(hipMemcpyAsync(d_root, root, 32, hipMemcpyHostToDevice, st));
        SR_TRY(hipStreamSynchronize(st));
        return PHANT_OK;
    }
    StateLayout lay;
    lay.n = n, lay.m = in.m, lay.code_bytes = in.code_bytes;
    int32_t rc = lay_out_state(ws, st, lay, err);
    if (rc) return rc;
    SR_TRY(hipMemsetAsync(lay.flag, 0, 4, st));
    hipLaunchKernelGGL(state_offsets_check_kernel, dim3(blocks((uint64_t)n + 1)), dim3(256), 0, st, in.code_off, in.slot_first, n, in.m, in.code_bytes, lay.flag);
    uint32_t flag = 0;
    SR_TRY(hipMemcpyAsync(&flag, lay.flag, 4, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    if (flag) {
        err = "state_root_dev: code_off / slot_first not monotone, not starting at 0 or not ending at code_bytes / n_slots";
        return PHANT_E_INVALID_ARG;
    }
    DevLeaves l;
    rc = state_leaves_core(ws, st, in, lay, l, err);
    if (rc) return rc;
    rc = trie_forest_dev(ws, st, l.pairs(), err);
    if (rc) return rc;
    SR_TRY(hipMemcpyAsync(d_root, l.root, 32, hipMemcpyDeviceToDevice, st));
    return PHANT_OK;
}

// One device's share of a SHARDED state root (comm.hip): its accounts -> leaves (device-resident) -> the sixteen sub-tries by
// top nibble as ONE forest pass -> per nibble the sub-trie's root and the RLP of its root node.  Only those (16 x (32 + cap +
// 4) bytes) come back; the leaves never leave the device.  out.len[x] == 0: no account of this share under nibble x.
int32_t state_subtrie_nodes_host(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t* roots, const RootNodes& out, std::string& err) {
    if (out.cap > SUBTRIE_CAP_MAX) {  // (before anything is done or written)
        err = "state_subtrie_nodes: cap > 256";
        return PHANT_E_INVALID_ARG;
    }
    std::memset(out.len, 0, 16 * sizeof(uint32_t));
    if (in.n == 0) return PHANT_OK;
    StateLayout lay;
    lay.subtrie_out = 16u * (36u + (size_t)out.cap) + 64u;  // 16 x (root 32 + length 4 + encoding) bytes and a flag line
    DevLeaves l;
    const int32_t rc = state_leaves_dev(ws, st, in, lay, l, err);
    if (rc) return rc;
    hipLaunchKernelGGL(nibble_segments_kernel, dim3(1), dim3(64), 0, st, l.keys, in.n, l.seg);
    return trie_forest_nodes_dev(ws, st, l.pairs(16), lay.sub_out, roots, out, err);
}

int32_t state_root_host(Workspaces& ws, hipStream_t st, const StateIn& in, uint8_t out[32], std::string& err) {
    if (in.n == 0) return trie_forest_host(ws, st, HostPairs{}, out, err);
    StateLayout lay;
    DevLeaves l;
    int32_t rc = state_leaves_dev(ws, st, in, lay, l, err);
    if (rc) return rc;
    rc = trie_forest_dev(ws, st, l.pairs(), err);
    if (rc) return rc;
    SR_TRY(hipMemcpyAsync(out, l.root, 32, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    return PHANT_OK;
}

// The touched keys of phant_state_witness / phant_state_proofs (host view; 20-byte address | 52-byte address ++ slot), grouped as
// exec_witness_parse_json groups them: accounts in order of first appearance, slots under their account in order of first
// appearance, duplicates collapsed with their flags ORed.
struct TouchedKeys {
    std::vector<std::array<uint8_t, 20>> addr;
    std::vector<std::vector<std::array<uint8_t, 32>>> slots;
    std::vector<std::vector<uint8_t>> slot_flags;
    std::vector<uint8_t> flags;
};
static int32_t group_touched_keys(const ProveQueries& touched, const char* call, TouchedKeys& tk, std::string& err) {
    const uint32_t n_wkeys = touched.n_queries;
    const uint8_t *const wkeys = touched.qkeys, *const wkey_flags = touched.q_flags;
    const uint32_t* const wkey_off = touched.qkey_off;
    std::vector<std::array<uint8_t, 20>>& t_addr = tk.addr;
    std::vector<std::vector<std::array<uint8_t, 32>>>& t_slots = tk.slots;
    std::vector<std::vector<uint8_t>>& t_slot_flags = tk.slot_flags;
    std::vector<uint8_t>& t_flags = tk.flags;
    std::unordered_map<std::string, uint32_t> touched_of;
    std::unordered_map<std::string, uint32_t> slot_of;  // address ++ slot -> its index under the account
    for (uint32_t k = 0; k < n_wkeys; ++k) {
        if (wkey_off[k + 1] < wkey_off[k]) {
            err = std::string(call) + ": wkey_off not monotone";
            return PHANT_E_INVALID_ARG;
        }
        const uint32_t len = wkey_off[k + 1] - wkey_off[k];
        if (len != 20 && len != 52) {
            err = std::string(call) + ": key " + std::to_string(k) + " is " + std::to_string(len) +
                  " bytes: a key is a 20-byte address or a 52-byte address ++ slot";
            return PHANT_E_INVALID_ARG;
        }
        const uint8_t* p = wkeys + wkey_off[k];
        const uint8_t fl = wkey_flags ? (uint8_t)(wkey_flags[k] & PHANT_PROVE_MAY_REMOVE) : (uint8_t)0;
        const auto ins = touched_of.emplace(std::string(reinterpret_cast<const char*>(p), 20), (uint32_t)t_addr.size());
        const uint32_t a = ins.first->second;
        if (ins.second) {
            std::array<uint8_t, 20> x;
            std::memcpy(x.data(), p, 20);
            t_addr.push_back(x);
            t_slots.emplace_back();
            t_slot_flags.emplace_back();
            t_flags.push_back(0);
        }
        if (len == 20) {
            t_flags[a] |= fl;
            continue;
        }
        const auto si = slot_of.emplace(std::string(reinterpret_cast<const char*>(p), 52), (uint32_t)t_slots[a].size());
        if (si.second) {
            std::array<uint8_t, 32> sl;
            std::memcpy(sl.data(), p + 20, 32);
            t_slots[a].push_back(sl);
            t_slot_flags[a].push_back(0);
        }
        t_slot_flags[a][si.first->second] |= fl;
    }
    return PHANT_OK;
}

// Which touched accounts the state holds: index_of_touched[a] = the state's row of touched account a, or NOT_HELD; held_idx = the rows
// of those it holds, in touched order.  Their touched slots become pv's queries against that account's storage trie.
constexpr uint32_t NOT_HELD = 0xffffffffu;
struct HeldAccounts {
    std::vector<uint32_t> index_of_touched, held_idx;
};
static HeldAccounts held_accounts(const StateIn& in, const TouchedKeys& tk, StateProve& pv) {
    std::unordered_map<std::string, uint32_t> index_of;
    index_of.reserve((size_t)in.n * 2);
    for (uint32_t i = 0; i < in.n; ++i) index_of.emplace(std::string(reinterpret_cast<const char*>(in.addrs + 20ull * i), 20), i);
    HeldAccounts h;
    h.index_of_touched.assign(tk.addr.size(), NOT_HELD);
    for (size_t a = 0; a < tk.addr.size(); ++a) {
        const auto it = index_of.find(std::string(reinterpret_cast<const char*>(tk.addr[a].data()), 20));
        if (it == index_of.end()) continue;
        h.index_of_touched[a] = it->second;
        h.held_idx.push_back(it->second);
        for (size_t j = 0; j < tk.slots[a].size(); ++j) {
            pv.slot_pre.insert(pv.slot_pre.end(), tk.slots[a][j].begin(), tk.slots[a][j].end());
            pv.slot_trie.push_back(it->second);
            pv.slot_flags.push_back(tk.slot_flags[a][j]);
        }
    }
    return h;
}

// The device steps in front of the state trie's proving pass: the touched addresses in (with their flags when the form reads any),
// hashed to the queries' keys (lay.tkeys, offsets lay.aoff), and the held accounts' code hashes -- with `sr` their storage roots as
// well, through the same 32 x na bytes -- on their way back: those copies ride on the pass's synchronisations.
static int32_t stage_touched_addresses(hipStream_t st, const StateLayout& lay, const DevLeaves& l, const TouchedKeys& tk, bool with_flags,
                                       const std::vector<uint32_t>& held_idx, std::vector<uint8_t>& hc, std::vector<uint8_t>* sr, std::string& err) {
    static_assert(sizeof(std::array<uint8_t, 20>) == 20, "tk.addr is the addresses back to back");
    const uint32_t na = (uint32_t)tk.addr.size(), nh = (uint32_t)held_idx.size();
    if (na) {
        SR_TRY(hipMemcpyAsync(lay.apre, tk.addr.data(), 20 * (size_t)na, hipMemcpyHostToDevice, st));
        if (with_flags) SR_TRY(hipMemcpyAsync(lay.aflags, tk.flags.data(), na, hipMemcpyHostToDevice, st));
        SR_TRY(launch_keccak256_fixed(lay.apre, 20, 20, na, lay.tkeys, st));
    }
    hipLaunchKernelGGL(query_offsets_kernel, dim3(blocks((uint64_t)na + 1)), dim3(256), 0, st, na, lay.aoff);
    hc.resize(32 * (size_t)nh);
    if (sr) sr->resize(32 * (size_t)nh);
    if (!nh) return PHANT_OK;
    SR_TRY(hipMemcpyAsync(lay.held, held_idx.data(), 4 * (size_t)nh, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gather32_kernel, dim3(blocks(32ull * nh)), dim3(256), 0, st, l.code_hash, lay.held, nh, lay.thc);
    SR_TRY(hipMemcpyAsync(hc.data(), lay.thc, hc.size(), hipMemcpyDeviceToHost, st));
    if (sr) {
        hipLaunchKernelGGL(gather32_kernel, dim3(blocks(32ull * nh)), dim3(256), 0, st, lay.sroots, lay.held, nh, lay.thc);
        SR_TRY(hipMemcpyAsync(sr->data(), lay.thc, sr->size(), hipMemcpyDeviceToHost, st));
    }
    return PHANT_OK;
}

// phant_state_witness: the state pass with both of its forests proven -- the touched slots against the storage forest while its
// tables stand, the touched addresses against the state trie behind it -- and the result laid out as the parser lays out a
// document: accounts and slots in order of first appearance, "state" = the state-trie nodes, then the storage nodes.
int32_t state_witness_host(Workspaces& ws, hipStream_t st, const StateIn& in, const ProveQueries& touched, ExecWitness& w, uint8_t root_out[32],
                           std::string& err) {
    w = ExecWitness();
    w.node_off.push_back(0);
    w.code_off.push_back(0);
    // ---- the keys, grouped as exec_witness_parse_json groups them ----
    TouchedKeys tk;
    if (const int32_t bad = group_touched_keys(touched, "state_witness", tk, err)) return bad;
    exec_witness_layout_keys(w, tk.addr, tk.slots);
    if (in.n == 0) return trie_forest_host(ws, st, HostPairs{}, root_out, err);  // (every key absent under the empty root)
    // ---- the device passes: the storage forest with the held accounts' touched slots, then the state trie with the touched
    // addresses' paths, exclusion proofs included ----
    StateProve pv;
    const HeldAccounts held = held_accounts(in, tk, pv);
    const uint32_t na = (uint32_t)tk.addr.size();
    StateLayout lay;
    lay.ns = (uint32_t)pv.slot_trie.size(), lay.witness = true, lay.na = na;
    DevLeaves l;
    int32_t rc = state_leaves_dev(ws, st, in, lay, l, err, &pv);
    if (rc) return rc;
    std::vector<uint8_t> nodes, hc;
    if ((rc = stage_touched_addresses(st, lay, l, tk, true, held.held_idx, hc, nullptr, err)) != PHANT_OK) return rc;
    rc = prove_collect(ws, st, l.pairs(), ProveQueries{lay.tkeys, lay.aoff, nullptr, lay.aflags, na}, nodes, w.node_off, nullptr, err);
    if (rc) return rc;
    SR_TRY(hipMemcpyAsync(root_out, l.root, 32, hipMemcpyDeviceToHost, st));
    SR_TRY(hipStreamSynchronize(st));
    // "state": the state-trie nodes, then the storage nodes
    const uint64_t b0 = nodes.size();
    w.nodes.resize(b0 + pv.nodes.size());
    if (b0) std::memcpy(w.nodes.data(), nodes.data(), b0);
    if (!pv.nodes.empty()) std::memcpy(w.nodes.data() + b0, pv.nodes.data(), pv.nodes.size());
    for (size_t i = 1; i < pv.node_off.size(); ++i) w.node_off.push_back(b0 + pv.node_off[i]);
    // "codes": every distinct non-empty code of a touched account the state holds, once, by the hash the pass computed
    std::unordered_set<std::string> seen_code;
    for (size_t h = 0; h < held.held_idx.size(); ++h) {
        const uint32_t i = held.held_idx[h];
        const uint64_t len = in.code_off[i + 1] - in.code_off[i];
        if (!len || !seen_code.emplace(reinterpret_cast<const char*>(hc.data() + 32 * h), 32).second) continue;
        const size_t c0 = w.codes.size();
        w.codes.resize(c0 + len);
        std::memcpy(w.codes.data() + c0, in.code + in.code_off[i], len);
        w.code_off.push_back((uint64_t)w.codes.size());
    }
    return PHANT_OK;
}

// phant_state_proofs: the same pass with both forests proven in the per-proof form and the result laid out as witness_parse_json
// lays out an EIP-1186 document: per touched account its account proof, then its storage proofs; the declarations are the state's
// own.
int32_t state_proofs_host(Workspaces& ws, hipStream_t st, const StateIn& in, const ProveQueries& touched, Witness& w, uint8_t root_out[32],
                          std::string& err) {
    static const uint8_t EMPTY_ROOT[32] = {0x56, 0xe8, 0x1f, 0x17, 0x1b, 0xcc, 0x55, 0xa6, 0xff, 0x83, 0x45, 0xe6, 0x92, 0xc0, 0xf8, 0x6e,
                                           0x5b, 0x48, 0xe0, 0x1b, 0x99, 0x6c, 0xad, 0xc0, 0x01, 0x62, 0x2f, 0xb5, 0xe3, 0x63, 0xb4, 0x21};
    static const uint8_t EMPTY_CODE[32] = {0xc5, 0xd2, 0x46, 0x01, 0x86, 0xf7, 0x23, 0x3c, 0x92, 0x7e, 0x7d, 0xb2, 0xdc, 0xc7, 0x03, 0xc0,
                                           0xe5, 0x00, 0xb6, 0x53, 0xca, 0x82, 0x27, 0x3b, 0x7b, 0xfa, 0xd8, 0x04, 0x5d, 0x85, 0xa4, 0x70};
    w = Witness();
    w.node_off.push_back(0);
    w.proof_first_node.push_back(0);
    w.preimage_off.push_back(0);
    TouchedKeys tk;
    if (const int32_t bad = group_touched_keys(ProveQueries{touched.qkeys, touched.qkey_off, nullptr, nullptr, touched.n_queries}, "state_proofs", tk, err))
        return bad;
    const uint32_t na = (uint32_t)tk.addr.size();
    StateProve pv;
    pv.per_proof = true;
    const HeldAccounts held = held_accounts(in, tk, pv);
    const std::vector<uint32_t>& index_of_touched = held.index_of_touched;
    // ---- the device passes: storage forest, then the state trie ----
    std::vector<uint8_t> anodes, hc, sr;
    std::vector<uint64_t> anode_off{0};
    std::vector<uint32_t> afirst((size_t)na + 1, 0);
    bool storage_proven = false;
    if (in.n == 0) {
        const int32_t rc = trie_forest_host(ws, st, HostPairs{}, root_out, err);  // (every key absent under the empty root: zero-node proofs)
        if (rc) return rc;
    } else {
        StateLayout lay;
        lay.ns = (uint32_t)pv.slot_trie.size(), lay.witness = true, lay.na = na;
        DevLeaves l;
        int32_t rc = state_leaves_dev(ws, st, in, lay, l, err, &pv);
        if (rc) return rc;
        storage_proven = pv.first.size() == pv.slot_trie.size() + 1;  // (no live slot in the whole state: no forest pass, every storage root empty)
        if ((rc = stage_touched_addresses(st, lay, l, tk, false, held.held_idx, hc, &sr, err)) != PHANT_OK) return rc;
        rc = prove_collect(ws, st, l.pairs(), ProveQueries{lay.tkeys, lay.aoff, nullptr, nullptr, na}, anodes, anode_off, &afirst, err);
        if (rc) return rc;
        SR_TRY(hipMemcpyAsync(root_out, l.root, 32, hipMemcpyDeviceToHost, st));
        SR_TRY(hipStreamSynchronize(st));
    }
    // ---- the document: account proof, then its storage proofs ----
    w.roots.assign(root_out, root_out + 32);
    auto add_proof = [&](uint32_t root, uint32_t account, const uint8_t* pre, size_t pre_len, const std::vector<uint8_t>& nodes,
                         const std::vector<uint64_t>& off, uint32_t k0, uint32_t k1) {
        w.root_idx.push_back(root);
        w.account_of.push_back(account);
        w.preimages.insert(w.preimages.end(), pre, pre + pre_len);
        w.preimage_off.push_back((uint32_t)w.preimages.size());
        for (uint32_t k = k0; k < k1; ++k) {
            w.nodes.insert(w.nodes.end(), nodes.begin() + (ptrdiff_t)off[k], nodes.begin() + (ptrdiff_t)off[k + 1]);
            w.node_off.push_back((uint64_t)w.nodes.size());
        }
        w.proof_first_node.push_back((uint32_t)(w.node_off.size() - 1));
    };
    uint32_t h = 0, sq = 0;  // the next held account, the next storage query
    for (uint32_t a = 0; a < na; ++a) {
        const uint32_t i = index_of_touched[a];
        const bool held = i != NOT_HELD;
        WitnessAccount acc{};
        std::memcpy(acc.address, tk.addr[a].data(), 20);
        std::memcpy(acc.storage_hash, held ? sr.data() + 32 * (size_t)h : EMPTY_ROOT, 32);
        std::memcpy(acc.code_hash, held ? hc.data() + 32 * (size_t)h : EMPTY_CODE, 32);
        if (held) {
            std::memcpy(acc.balance, in.bal + 32ull * i, 32);
            acc.nonce = in.nonces[i];
        }
        acc.has_storage_hash = acc.has_code_hash = acc.has_balance = acc.has_nonce = 1;
        acc.proof = (uint32_t)w.root_idx.size();
        add_proof(0u, a, acc.address, 20, anodes, anode_off, afirst[a], afirst[a + 1]);
        w.accounts.push_back(acc);
        w.roots.insert(w.roots.end(), acc.storage_hash, acc.storage_hash + 32);
        // the values of this account's touched slots, from the state's own arrays
        std::unordered_map<std::string, const uint8_t*> value_of;
        if (held && !tk.slots[a].empty())
            for (uint32_t s = in.slot_first[i]; s < in.slot_first[i + 1]; ++s)
                value_of.emplace(std::string(reinterpret_cast<const char*>(in.skeys + 32ull * s), 32), in.svals + 32ull * s);
        for (const std::array<uint8_t, 32>& sl : tk.slots[a]) {
            WitnessSlot slot{};
            slot.proof = (uint32_t)w.root_idx.size();
            slot.account = a;
            slot.has_value = 1;
            const auto it = value_of.find(std::string(reinterpret_cast<const char*>(sl.data()), 32));
            if (it != value_of.end()) std::memcpy(slot.value, it->second, 32);
            const bool proven = held && storage_proven;
            add_proof(1u + a, a, sl.data(), 32, pv.nodes, pv.node_off, proven ? pv.first[sq] : 0u, proven ? pv.first[sq + 1] : 0u);
            if (held) ++sq;
            w.slots.push_back(slot);
        }
        if (held) ++h;
    }
    return PHANT_OK;
}

}  // namespace phant
