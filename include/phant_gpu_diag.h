/*
 * phant_gpu_diag.h -- measurement and diagnostics entry points of libphant_gpu.
 *
 * NOT part of the drop-in boundary (include/phant_gpu.h): nothing a consensus client calls is declared here.  These are
 * what bench.py, tools/ and tests/ use to time the library, to read back what a launch did, and to switch between
 * measured alternatives of one kernel.  The library itself reads NO environment variable: every switch is per ctx and is
 * set through this header.
 */
#ifndef PHANT_GPU_DIAG_H
#define PHANT_GPU_DIAG_H

#include "phant_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device time of the last *_dev call -- every kernel it launched, first to last -- measured with HIP events recorded on
 * the ctx stream around the launches (bench.py uses this for `roofline.achieved`).  Enable with phant_timing(ctx, 1). */
PHANT_API int32_t phant_timing(phant_ctx *ctx, int32_t enable);
PHANT_API int32_t phant_last_kernel_ms(phant_ctx *ctx, float *ms);

/* After a verify call (per-proof or node-set form) on this ctx: hashed[c] = number of nodes of (c+1) rate blocks (c = 7: 8
 * or more) that were actually hashed, i.e. distinct nodes; synchronises the ctx stream. */
PHANT_API int32_t phant_verify_stats(phant_ctx *ctx, uint32_t hashed[8]);
/* After a two-tier verify call on this ctx: out[0] = proofs the walk could not settle from the pipeline's tables and
 * verified from scratch, out[1] = nodes decoded by walks that had to decode more than one node (both 0 for a witness
 * of full-branch paths ending in a leaf); synchronises the ctx stream. */
PHANT_API int32_t phant_verify_path_stats(phant_ctx *ctx, uint32_t out[2]);
/* The two tiers of the last verify call on this ctx: out[0] = trie levels deduplicated (0: every shipped node hashed in
 * place), out[1] = nodes hashed from the class lists (representatives, nodes without a group, copies that differed) and
 * out[2] = their Keccak-f, out[3] = nodes hashed in place by the deep tier and out[4] = their Keccak-f. */
PHANT_API int32_t phant_verify_tier_stats(phant_ctx *ctx, uint32_t out[5]);
/* 0 = the last verify launch hashed every shipped node in place (small batches), 1 = two tiers */
PHANT_API int32_t phant_verify_form(phant_ctx *ctx, uint32_t *form);
/* With PHANT_DIAG_VERIFY_SERIAL set on the ctx (the pipeline's tiers then run one after the other on the ctx stream): device
 * time of each stage of the last two-tier verify launch, alone on the chip -- ms[0..4] = propose_kernel, hash_deep_kernel,
 * dedup_kernel, hash_list_kernel, walk_kernel.  Synchronises the ctx stream. */
#define PHANT_VERIFY_KERNEL_STAGES 5
PHANT_API int32_t phant_verify_kernel_ms(phant_ctx *ctx, float ms[PHANT_VERIFY_KERNEL_STAGES]);
/* What the chip can overlap at best on THIS witness (arguments of phant_mpt_verify_batch_dev).  One complete verification
 * first; then, `reps` times each on the ctx's streams, out_ms[0] = only the hashing that launch did (the deep tier and
 * everything listed, next to each other: the integer-VALU side), out_ms[1] = only a coalesced read of the node bytes (the
 * memory side, a clean stream), out_ms[2] = both next to each other.  A verify launch cannot be shorter than out_ms[2]; how
 * far it is above it is what its own kernels' shape costs.  bench.py: roofline.bound_experiment.  Synchronises. */
PHANT_API int32_t phant_verify_bound_experiment(phant_ctx *ctx, const uint8_t *d_roots, uint32_t n_roots,
                                                const uint32_t *d_root_idx, const uint8_t *d_keys, uint32_t key_len,
                                                const uint8_t *d_nodes, uint64_t nodes_len, const uint64_t *d_node_off,
                                                uint32_t total_nodes, const uint32_t *d_proof_first_node, uint32_t n,
                                                uint8_t *d_status, uint32_t reps, float out_ms[3]);
/* The Keccak-f[1600] rate of the device when it does nothing else -- waves_per_simd (1..8) waves per SIMD, every lane `perms`
 * permutations of a register-resident state with the product's round function, timed with events on the ctx stream
 * (synchronises it).  *perms_per_s = permutations per second over the whole chip: the VALU ceiling every hash kernel of this
 * library is measured against (bench.py: roofline.valu.peak). */
PHANT_API int32_t phant_keccak_rate(phant_ctx *ctx, uint32_t waves_per_simd, uint32_t perms, double *perms_per_s);

/* What the trie hasher's last call on this ctx did (phant_mpt_root*, phant_index_root*, phant_block_roots, the forests of the
 * state root and of the prover ...): the choices its launcher made from the node counts of the depth bins, the key count and free
 * memory, so that a test that forces one of them can tell that the call took it.  Host integers the launcher has anyway; only
 * out[10] and out[15] are read from the device, when this is called.  Synchronises the ctx stream.
 *   out[0]  the pass: 0 = none (no call yet, no keys), 1 = the two-launch pass for small tries, 2 = the general pass
 * the rest is about the general pass (0, deep_from -1, after the small one):
 *   out[1]  1 = the leaves were queued ahead of the host's sizing, with worst-case tables
 *   out[2]  (int32_t) the depth from which the bins ran on the helper stream beside the leaves, -1 = no helper stream
 *   out[3]  non-empty depth bins                    out[4]  nodes of the largest
 *   out[5 .. 9]  bins launched a wave per node, a node per half wave, a lane per node in slots of 1, 2, 4 rate blocks
 *   out[10] nodes that did not fit their bin's slot class and went through its fallback list (all bins)
 *   out[11] 1 = the kernel for leaves of 136 .. 543 bytes ran
 *   out[12] branch nodes                            out[13] keys
 *   out[14] of the bins of out[5 .. 9], those launched on the helper stream
 *   out[15] bytes of the scratch blob taken by the nodes that fit no LDS slot (4-byte rounded; branches: with their extension's
 *           room; leaves of 544 bytes and more in the general pass), both passes, saturating */
#define PHANT_TRIE_STATS 16
PHANT_API int32_t phant_trie_stats(phant_ctx *ctx, uint32_t out[PHANT_TRIE_STATS]);

/* A/B of the node-set pipeline's hash kernel (tools/probe_nodeset*.py): form = how a wave hashes 532-byte nodes (0 plain,
 * 1 its issue priority falls block by block -- the default --, 2 every rate block requested a permutation ahead into
 * registers); order = 0: class lists by falling rate-block count (default), 1: rising; hash_lds_bytes = idle dynamic LDS per
 * hash workgroup (default 40 KiB); resident_wgs = the hash grid's cap, its waves striding over the chunk queue (default 0 = a
 * wave per chunk).  What was measured: profiles/r6_explore/NOTES.md. */
PHANT_API int32_t phant_nodeset_tune(phant_ctx *ctx, int32_t form, uint32_t order, uint32_t hash_lds_bytes,
                                     uint32_t resident_wgs);

/* What the last node-set launch on this ctx's own workspace did (phant_mpt_verify_nodeset*, the execution-witness calls; not the
 * streaming slots): the path its launcher took and what its kernels counted, so that a test that forces a path can tell that the call
 * took it.  All zeros if there was none.  Host integers the launcher has anyway, and the header words phant_verify_stats reads.
 * Synchronises the ctx stream.
 *   out[0]      the path: 0 = none, 1 = a wave per node in single-wave workgroups, 2 = a wave per node in four-wave workgroups,
 *               3 = class lists
 *   out[1 .. 9] nodes per list: the lists of 1, 2, ... 7, 8-or-more rate blocks, then the list of the nodes of exactly 532 bytes
 *               (which phant_verify_stats counts with the four-block class, and this call does not)
 *   out[10]     nodes that went to the overflow list (the record table did not take them: copies of a node already there)
 *   out[11]     workgroups of the hash grid             out[12]  nodes offered
 *   out[13]     the launch's epoch on the workspace */
#define PHANT_NODESET_STATS 14
PHANT_API int32_t phant_nodeset_stats(phant_ctx *ctx, uint32_t out[PHANT_NODESET_STATS]);

/* One primitive of the secp256k1 arithmetic (phant_amd/csrc/secp256k1.hip.h) per lane, host arrays in and out, so that a carry
 * bug shows at the primitive and not as a wrong address 3 000 multiplications later.  Numbers are 32 big-endian bytes.
 *   op 0 field mul, 1 field sqr, 2 field inverse (0 -> 0), 4 scalar mul, 5 scalar inverse: rows of 32 bytes in a (and b for
 *        0 and 4; b is ignored otherwise), 32 out.  The field ops take ANY 256-bit operands, the scalar ops too.
 *   op 3 field square root: 32 in, 33 out: x^((p+1)/4), then 1 if that is a root of x, else 0.
 *   op 6 point double, 7 point add (the general formula), 8 point add (the formula for an affine second operand): rows of 65
 *        bytes, x || y || flag (flag != 0: the point at infinity, x and y ignored; else x, y < p on the curve), 65 out. */
#define PHANT_DIAG_SECP_OPS 9
PHANT_API int32_t phant_diag_secp_op(phant_ctx *ctx, uint32_t op, const uint8_t *a, const uint8_t *b, uint32_t n, uint8_t *out);

/* The three primitives of phant_amd/csrc/radix_sort.hip that headers, receipts, transactions, access lists, the post-state, the
 * transactions' pre-state and the state root share, each alone on inputs of the caller's choice: host arrays in and out, on the ctx
 * stream, synchronised on return.  Every device buffer is carved at exactly the size phant_amd/csrc/launch.h documents for it, with
 * 256 bytes of 0xEE behind it that are read back after the run: a touched guard is PHANT_E_DEVICE, and phant_last_error names the
 * buffer.  A null pointer where n > 0 needs an array and a null ctx are PHANT_E_INVALID_ARG; a refused call writes nothing.
 *   phant_diag_scan_u32       the exclusive prefix sum of counters[0 .. n), in place, modulo 2^32.
 *   phant_diag_sort_pairs     the stable sort of n (64-bit key, 32-bit value) pairs by the low `bits` (0 .. 64; more: INVALID_ARG)
 *                             key bits, rounded up to whole bytes; keys come back whole.  bits == 0 or n == 0: the input unchanged.
 *   phant_diag_order_digests  order_out[0 .. n): the 32-byte digests in ascending order of (seg_of[i], digest i); seg_of may be null
 *                             (one segment), a seg_of[i] >= n_seg is INVALID_ARG.  prefix_bits: 0 = the product's choice (32 bits,
 *                             ties repaired), k = sorted on k key bits (rounded up to bytes) and ties left alone, k | 0x80000000 =
 *                             ties repaired.  *flag_out != 0: the device did not decide the order (a run of more than 16 equal
 *                             prefixes, a digest twice in a segment, ties left alone) -- order_out is then what the callers throw away. */
PHANT_API int32_t phant_diag_scan_u32(phant_ctx *ctx, uint32_t *counters, uint32_t n);
PHANT_API int32_t phant_diag_sort_pairs(phant_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint32_t n, uint32_t bits,
                                        uint64_t *keys_out, uint32_t *vals_out);
PHANT_API int32_t phant_diag_order_digests(phant_ctx *ctx, const uint8_t *digests, const uint32_t *seg_of, uint32_t n, uint32_t n_seg,
                                           uint32_t prefix_bits, uint32_t *order_out, uint32_t *flag_out);

/* Per-ctx switches of measured alternatives and test hooks (phant_diag_set(ctx, knob, value)).  The library's defaults are what
 * the measurements in profiles/ chose; nothing here changes a result, only how it is computed. */
enum {
    PHANT_DIAG_VERIFY_SERIAL = 1,     /* != 0: the verify pipeline's tiers one after the other on the ctx stream, events around each
                                         stage (phant_verify_kernel_ms) */
    PHANT_DIAG_VERIFY_HASH_LDS_KB,    /* idle dynamic LDS (KiB, 0..47) of the deep tier's workgroups while the shallow tier runs beside them */
    PHANT_DIAG_VERIFY_NO_COOP,        /* != 0: small batches never take the node-per-half-wave / node-per-wave hash kernels */
    PHANT_DIAG_VERIFY_NO_WAVE,        /* != 0: ... the half-wave kernel instead of the wave-per-node one */
    PHANT_DIAG_VERIFY_COOP_MAX,       /* ... up to this many nodes */
    PHANT_DIAG_STREAM_WGS,            /* phant_verify_bound_experiment: workgroups of the read stream (0 = 2 048) */
    PHANT_DIAG_STREAM_MB,             /* ... != 0: the region (MB) its index wraps in (a stream out of L2 / Infinity Cache) */
    PHANT_DIAG_TRIE_NO_SIDE,          /* trie hasher: != 0: no depth bins on the helper stream beside the leaves */
    PHANT_DIAG_TRIE_SIDE_MIN_KEYS,    /* ... from this many keys on (-1: the default) */
    PHANT_DIAG_TRIE_AHEAD_MAX_KEYS,   /* the leaves are queued ahead of the host's sizing up to this many keys (-1: the default) */
    PHANT_DIAG_TRIE_SIDE_LDS,         /* idle dynamic LDS (bytes) of the bulk leaf kernel while bins run beside it (-1: the default) */
    PHANT_DIAG_TRIE_FALLBACK_GRID,    /* workgroups of a bin's fallback pass (-1: the default) */
    PHANT_DIAG_TRIE_SLOT_BLOCKS,      /* != 0: every bin in slots of this many rate blocks (1, 2, 4) */
    PHANT_DIAG_TRIE_NO_COOP,          /* != 0: thin bins through the lane-per-node kernels */
    PHANT_DIAG_TRIE_COOP_MAX,         /* ... up to this many nodes (-1: the default) */
    PHANT_DIAG_TRIE_NO_WAVE,          /* != 0: the half-wave kernel for every thin bin */
    PHANT_DIAG_TRIE_JOIN_IN_STREAM,   /* != 0: the helper stream joined by an event in the main stream */
    PHANT_DIAG_SORT_NO_FALLBACK,      /* state root: != 0: an undecided device sort is an error, not a host sort (tests) */
    PHANT_DIAG_SORT_PREFIX_BITS,      /* state root: the device sort on this many key bits, ties left undecided (-1: its own choice) */
    PHANT_DIAG_SORT_REPAIR_BITS,      /* ... ties repaired (-1: its own choice) */
    PHANT_DIAG_NODESET_WAVE_MAX,      /* node-set witnesses of up to this many nodes are hashed a node per wave (default 3 500; 0: never) */
    PHANT_DIAG_TRIE_SMALL_MAX_KEYS,   /* trie hasher: up to this many keys a call takes the two-launch pass for small tries (-1: the default, 0: never) */
    PHANT_DIAG_CODE_HASH_FORM,        /* phant_exec_witness_prestate: the codes hashed 0 = a half wave per code (the default), 1 = a lane per code */
    PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS,/* phant_exec_witness_poststate: != 0: a slot's 32 bytes ARE its storage-trie key, not hashed (tests: tries
                                          with chosen keys -- 63 shared nibbles, nodes small enough to embed; the accounts stay hashed).
                                          A TEST HOOK ONLY: it changes what the entry point computes (the root is no state root any
                                          more), so a client never sets it; it holds for the context it was set on until set back to 0 */
    PHANT_DIAG_ADVANCE_ESTIMATE_BYTES, /* phant_exec_witness_advance: > 0: the room estimated for the emitted nodes is this many bytes (and a
                                          node descriptor per 64 of them), so that a test reaches the run with the counted sizes; 0: the
                                          call's own estimate.  A TEST HOOK ONLY: the result does not depend on it */
    PHANT_DIAG_VERIFY_LIST_WGS,        /* two-tier verify: > 0: the grid that hashes the listed shallow nodes is at most this many workgroups
                                          (of four waves), so that a test with a few hundred proofs reaches a queue longer than the grid,
                                          whose waves then stride over it; 0: sized from the batch.  A TEST HOOK ONLY: the result does not
                                          depend on it */
    PHANT_DIAG_RANGES_NO_LEAF_PASS,    /* phant_mpt_verify_ranges: != 0: no leaf pass -- every leaf is encoded and hashed by the lane that builds
                                          its parent branch, as in the post-state build (the A/B of DESIGN.md section 7p) */
    PHANT_DIAG_RANGES_ITEMS_PER_RANGE, /* phant_mpt_verify_ranges: >= 0: the room estimated for the items outside the leaves, per range, so
                                          that a test whose ranges' walks leave more than that reaches the run with the counted size
                                          (0: room for the leaves and 64 items); -1: the call's own estimate.  A TEST HOOK
                                          ONLY: the result does not depend on it */
    PHANT_DIAG_LOGFILTER_SETS,         /* phant_block_log_filters: how a filter's set is compared: 0 = sets of up to
                                          PHANT_LOGFILTER_LINEAR_MAX entries entry by entry, larger ones through the keyed table (the
                                          default); 1 = every non-empty set through the table; 2 = every set entry by entry.  The
                                          result does not depend on it */
    PHANT_DIAG_FEEHIST_BLOCK_MAX       /* phant_block_fee_history: the most rows a block may have: 0 = PHANT_FEEHIST_BLOCK_MAX (the
                                          product's value); 1 .. PHANT_FEEHIST_BLOCK_MAX - 1 = that many, so that a test reaches the
                                          boundary with a few hundred rows.  A TEST HOOK ONLY: the cap is never raised */
};
/* phant_block_log_filters: the largest set that is compared entry by entry (tools/bench_log_filters.py measures both forms) */
#define PHANT_LOGFILTER_LINEAR_MAX 16u
PHANT_API int32_t phant_diag_set(phant_ctx *ctx, uint32_t knob, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* PHANT_GPU_DIAG_H */
