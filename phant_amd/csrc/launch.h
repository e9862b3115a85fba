// launch.h -- host-callable launchers of the HIP kernels (internal; the public
// surface is include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"

namespace phant {

hipError_t launch_keccak256_var(const uint8_t* d_blob, const uint64_t* d_off, uint32_t n,
                                uint8_t* d_out, hipStream_t st);
hipError_t launch_keccak256_fixed(const uint8_t* d_blob, uint32_t msg_len, uint64_t stride,
                                  uint32_t n, uint8_t* d_out, hipStream_t st);
// SHA-256 of the same messages (sha256.hip.h): d_out n x 32 bytes, 16-byte aligned
hipError_t launch_sha256_var(const uint8_t* d_blob, const uint64_t* d_off, uint32_t n,
                             uint8_t* d_out, hipStream_t st);

// log filters over a chain segment (filters.hip.h; phant_block_log_filters[_dev], phant_log_filters_bloom[_dev]): the structs as they came,
// checked by filters_check.h's check_match_args / check_bloom_args, n_filters != 0; salt: the ctx's key of the keyed table; linear_max: the
// largest set compared entry by entry.  PHANT_OK, or the code with the reason in err
struct Workspaces;
int32_t block_log_filters(Workspaces& ws, hipStream_t st, const phant_logmatch_in& in, const phant_log_filters& filters, phant_logmatch_out& out, bool device_form,
                          const uint32_t salt[2], uint32_t linear_max, std::string& err);
int32_t log_filters_bloom(Workspaces& ws, hipStream_t st, const uint8_t* blooms, uint32_t n_blooms, const phant_log_filters& filters, uint64_t* may,
                          uint32_t* may_count, bool device_form, std::string& err);

// fee history over a chain segment (fee_history.hip.h; phant_block_fee_history[_dev]): the structs as they came, checked by
// feehist_check.h's check_args and check_percentiles, n_blocks != 0; block_max: the cap on a block's rows.  PHANT_OK, or the code with
// the reason in err
int32_t block_fee_history(Workspaces& ws, hipStream_t st, const phant_fee_history_in& in, phant_fee_history_out& out, bool device_form, uint32_t block_max,
                          std::string& err);

// diagnostics: blocks x 256 lanes run `perms` Keccak-f each on a register-resident state; d_out: blocks x 256 words
hipError_t launch_keccak_rate(uint32_t* d_out, uint32_t blocks, uint32_t perms, hipStream_t st);

// bulk_keccak.hip: blooms n_receipts x 256 bytes (4-byte aligned, zeroed by the launcher); addresses n x 20 bytes
// (4-byte aligned)
hipError_t launch_logs_bloom(const uint8_t* d_items, const uint64_t* d_item_off, const uint32_t* d_item_receipt,
                             uint32_t n_items, uint32_t n_receipts, uint8_t* d_blooms, hipStream_t st);
hipError_t launch_sender_addresses(const uint8_t* d_pubkeys, uint64_t stride, uint32_t n, uint8_t* d_out,
                                   hipStream_t st);

// secp256k1 (secp256k1.hip.h): the table of G's multiples (256 x 64 bytes), a lane per signature (rows of 32 / 1 bytes in, 64 /
// 20 / 1 bytes out; d_pre_status, d_pubkeys, d_addresses, d_status may be null), and one arithmetic primitive per lane
constexpr size_t SECP_GTABLE_BYTES = 256 * 64;
hipError_t launch_secp_gtable(uint32_t* d_gtable, hipStream_t st);
hipError_t launch_ecrecover(const uint8_t* d_hashes, const uint8_t* d_r, const uint8_t* d_s, const uint8_t* d_recid,
                            const uint8_t* d_pre_status, uint32_t n, uint32_t flags, const uint32_t* d_gtable,
                            uint8_t* d_pubkeys, uint8_t* d_addresses, uint8_t* d_status, hipStream_t st);
hipError_t launch_secp_op(uint32_t op, const uint8_t* d_a, const uint8_t* d_b, uint32_t n, uint8_t* d_out, hipStream_t st);

// index-form witnesses: decode the nodes' hex digits out of the JSON text on the device (d_err: 2 dwords, [0] != 0
// when some digit was not hex, [1] = the first such node), and compact the proven values for the host
hipError_t launch_hex_decode(const uint8_t* d_json, const uint64_t* d_node_src, const uint64_t* d_node_off,
                             uint32_t total_nodes, uint8_t* d_nodes, uint32_t* d_err, hipStream_t st);
hipError_t launch_gather_values(const uint8_t* d_nodes, const uint64_t* d_value_off, const uint32_t* d_value_len,
                                uint32_t n, uint32_t cap, uint8_t* d_out, hipStream_t st);

struct VerifyArgs {
    const uint8_t* roots;
    uint32_t n_roots;
    const uint32_t* root_idx;  // may be null
    const uint8_t* keys;
    uint32_t key_len;
    const uint8_t* nodes;
    uint64_t nodes_len;
    const uint64_t* node_off;
    const uint32_t* proof_first_node;
    uint32_t n;
    uint8_t* status;
    uint64_t* value_off;  // may be null
    uint32_t* value_len;  // may be null
    uint32_t* fail_count = nullptr;  // may be null: n_roots counters of proofs that are not PRESENT/ABSENT,
                                     // produced by the pipeline's last kernel (phant_mpt_verify_verdict_dev)
    uint32_t total_nodes = 0;        // node_off has total_nodes + 1 entries: a proof whose node range reaches
                                     // beyond it is BAD_INPUT before node_off is touched (set by the launchers'
                                     // caller, capi.hip::run_verify)
};
// Two-tier pipeline (mpt_verify_v3.hip): the trie levels that repeat across proofs are deduplicated (propose ->
// dedup -> class-sorted hashing of the distinct nodes), the deeper ones hashed in place next to that, then walk.
// ws = verify_workspace_bytes().  dedup_levels: how many levels from the root are deduplicated; < 0 = chosen from the
// batch size, 0 = hash every shipped node.  `side` (may be null): helper stream + events owned by the ctx; with
// it the deep tier runs NEXT TO the shallow tier (VALU-bound hashing beside a memory stream), without it in front.
struct FlatSide {
    hipStream_t stream;       // non-blocking helper stream owned by the ctx: the deep tier
    hipEvent_t fork, join;    // timing-disabled events
    // diagnostics (phant_verify_bound_experiment): a second helper stream for the clean read stream
    hipStream_t stream2 = nullptr;
    hipEvent_t join2 = nullptr;
};
size_t verify_workspace_bytes(uint32_t total_nodes);
// The deep tier's occupancy cap and the diagnostics switches (per ctx; set through include/phant_gpu_diag.h, never from the
// environment).
struct VerifyTune {
    // An otherwise unused dynamic LDS allocation per workgroup of the deep tier caps how many of them a CU holds
    // (160 KiB / (8 KiB + it)) WHILE the shallow tier's memory-bound kernels run next to it: 40 KiB -> 3 workgroups = 3 hash
    // waves per SIMD = 360 of its 512 VGPRs, which leaves dedup_kernel (48) three waves per SIMD (measured on BASELINE
    // config 3, round 3: one launch 0.262 ms uncapped, 0.234 at 40 KiB, 0.237 at 52 KiB).  Alone, the deep tier runs uncapped.
    uint32_t hash_lds = 40u * 1024u;
    bool serial = false;  // diagnostics: the tiers one after the other on the ctx stream (clean per-kernel durations in a trace)
    uint32_t* last_shallow = nullptr; // diagnostics: where the launcher notes the tier split it chose (phant_verify_tier_stats)
    hipEvent_t* kernel_ev = nullptr;  // diagnostics, with `serial`: VERIFY_KERNEL_STAGES + 1 events recorded around the stages of a
                                      // two-tier launch (phant_verify_kernel_ms)
    uint32_t coop_max = 2048;      // S = 0 form: batches of up to this many nodes take the node-per-half-wave hash kernel
    bool no_coop = false;
    bool no_wave = false;  // (A/B: small S = 0 launches through the half-wave kernel, not the wave-per-node one)
    uint32_t* last_form = nullptr; // diagnostics: 0 = S = 0 (every shipped node hashed in place), 1 = two tiers
    uint32_t list_wgs_cap = 0;     // tests: != 0: the list role's grid is at most this many workgroups (its waves then stride over the queue)
    // diagnostics (phant_verify_bound_experiment), on a workspace a complete launch over the same witness has just left: 1 = only
    // the hashing of that launch (deep tier + everything listed, next to each other), 2 = only a coalesced read of the witness's
    // bytes (a clean stream with next to no VALU), 3 = both next to each other -- what the chip can overlap at best
    uint32_t diag = 0;
    uint32_t* diag_sink = nullptr;  // device words the read stream leaves its checksum in (so that the loads are not dead)
    uint32_t diag_stream_wgs = 0;   // the read stream's workgroups (0 = 2 048) and, != 0, the region in MB its index wraps in
    uint32_t diag_stream_mb = 0;
};
// stages of a two-tier launch, in the order of phant_verify_kernel_ms: propose_kernel, hash_deep_kernel, dedup_kernel,
// hash_list_kernel, walk_kernel
constexpr int VERIFY_KERNEL_STAGES = 5;
hipError_t launch_mpt_verify(const VerifyArgs& a, uint32_t total_nodes, uint8_t* ws, int32_t dedup_levels,
                             hipStream_t st, const FlatSide* side, const VerifyTune& tune);
// nodes hashed per rate-block class by the last launch, from a host copy of the workspace's first
// VERIFY_HEADER_WORDS words
constexpr uint32_t VERIFY_HEADER_WORDS = 2048;
void verify_stats_from_header(const uint32_t* hdr, uint32_t hashed[8]);
// out[0] = nodes hashed from the class lists, [1] = their Keccak-f (class c = c + 1 permutations), [2] = nodes hashed in
// place by the deep role, [3] = their Keccak-f
void verify_tier_stats_from_header(const uint32_t* hdr, uint32_t out[4]);
// out[0] = proofs the walk could not settle from the tables (verified from scratch by their lane), out[1] = nodes
// decoded by walks that had to decode more than one
void verify_paths_from_header(const uint32_t* hdr, uint32_t out[2]);
// node-SET witnesses (every node shipped once, any order; references resolved by hash): mpt_verify_nodeset.hip.
// The workspace is sized for a CAPACITY in nodes (verify_nodeset_capacity(total_nodes), verify_nodeset_workspace_bytes(capacity)),
// zeroed when it is allocated and never cleared afterwards: every launch on it names the same capacity (the layout follows from it)
// and carries an `epoch` greater than every earlier launch's on the same memory (the owner counts; a failed launch -> zero it again).
// salt: the key of the record table's slot function (per ctx, random).  a.fail_count (may be null): the per-root verdict.
struct NodesetTune {
    uint32_t form = 1;      // how a wave hashes 532-byte nodes: 0 plain, 1 its issue priority falls block by block (hash_b532<true>),
                            // 2 every rate block requested a permutation ahead, into registers (hash_b532_ahead: 3 waves per SIMD)
    uint32_t order = 0;     // chunk queue: 0 = lists by falling rate-block count, 1 = rising (A/B)
    uint32_t hash_lds = 40u * 1024u;  // idle dynamic LDS per hash workgroup (not an occupancy cap at this size: four workgroups a CU
                                      // either way): measured, one launch of BASELINE's node set 189 us without, 183 / 180 / 177 at
                                      // 8 / 32 / 40 KiB -- the dispatcher hands out workgroups with LDS more slowly, the waves of a
                                      // SIMD start apart and do not all wait for their rate blocks at once (profiles/r6_explore/NOTES.md)
    uint32_t wave_max = 3500;   // sets of up to this many nodes: a WAVE per node (set_hash_wave_kernel), no class lists (0: never).  Measured,
                                // one launch, wave per node against the lists: 309 nodes 44 / 65 us, 876: 54 / 93, 1 448: 61 / 78, 3 200: 77 / 82,
                                // 5 137: 87-90 / 81, 9 800: 120 / 79
    uint32_t resident_wgs = 0;  // 0 = a wave per chunk.  Otherwise the hash grid is capped at this many workgroups and its waves stride
                                // over the chunk queue (A/B: one generation of waves, every wave a four-permutation chunk and then
                                // maybe a one-permutation one -- measured SLOWER, 199 against 190 us: the lockstep it creates costs
                                // more than the thin second generation it avoids)
    uint32_t* last = nullptr;   // diagnostics (phant_nodeset_stats): where launch_nodeset_hash notes what it chose -- [0] the path (1 = a wave
                                // per node in single-wave workgroups, 2 = in four-wave workgroups, 3 = class lists), [1] the workgroups
                                // of the hash grid, [2] the nodes offered
};
uint32_t verify_nodeset_capacity(uint32_t total_nodes);
size_t verify_nodeset_workspace_bytes(uint32_t cap_nodes);
hipError_t launch_mpt_verify_nodeset(const VerifyArgs& a, uint32_t total_nodes, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch,
                                     const uint32_t salt[2], hipStream_t st, const NodesetTune& tune);
// nodes hashed per rate-block class by the launch of `epoch`, from a host copy of the workspace's first VERIFY_HEADER_WORDS
// words; *overflow (may be null): nodes that went through the second table
void verify_nodeset_stats_from_header(const uint32_t* hdr, uint32_t epoch, uint32_t hashed[8], uint32_t* overflow);
// the same counts list by list, not folded into classes: lists[0 .. 7] = the rate-block classes without the 532-byte nodes, lists[8] =
// the nodes of exactly 532 bytes
void verify_nodeset_lists_from_header(const uint32_t* hdr, uint32_t epoch, uint32_t lists[9]);
// prestate.hip.h (included by mpt_verify_nodeset.hip): the pre-state of an execution witness between and behind the two walks of
// the node-set pipeline (phant_exec_witness_prestate).  Every pointer is device memory of the call.
struct PrestateArgs {
    const uint8_t* nodes;
    uint32_t na, ns, nc;
    uint8_t* acc_status;          // na: the account walk's statuses, decoded in place
    const uint64_t* acc_voff;
    const uint32_t* acc_vlen;
    uint64_t* nonces;             // na
    uint8_t* balances;            // na x 32, big-endian
    uint8_t* storage_roots;       // na x 32: the storage walk's root table
    uint8_t* code_hashes;         // na x 32
    uint32_t* code_index;         // na
    uint8_t* slot_status;         // ns: the storage walk's statuses, decoded in place
    const uint64_t* slot_voff;
    const uint32_t* slot_vlen;
    const uint32_t* slot_account; // ns
    uint8_t* slot_vals;           // ns x 32, big-endian
    uint32_t* counters;           // PRE_CNT_*: zeroed by the caller
    const uint8_t* codes;
    const uint64_t* code_off;     // nc + 1
    uint32_t* code_dig;           // nc x 8 words
    uint32_t* code_slot;          // nc: the table slot a code's digest lives in
    uint32_t* table;              // mask + 1: 1 + the lowest code index with the slot's digest, 0 = free (zeroed by the caller)
    uint32_t* table_used;         // mask + 1: an account matched the slot's digest (zeroed by the caller)
    uint32_t mask;
    uint32_t salt0, salt1;
};
enum : uint32_t { PRE_CNT_FAILED = 0, PRE_CNT_MISSING_CODE = 1, PRE_CNT_UNUSED_CODES = 2 };  // PrestateArgs::counters
hipError_t launch_prestate_accounts(const PrestateArgs& a, hipStream_t st);  // account_decode_kernel
hipError_t launch_prestate_slots(const PrestateArgs& a, hipStream_t st);     // slot_decode_kernel
// code_hash_kernel (form 0: a half wave per code) or code_hash_lane_kernel (form 1: a lane per code); table / table_used zeroed
hipError_t launch_code_hash(const PrestateArgs& a, uint32_t form, hipStream_t st);
hipError_t launch_code_match(const PrestateArgs& a, hipStream_t st);         // code_match_kernel + code_unused_kernel
uint32_t code_table_slots(uint32_t n_codes);
// The node-set launch in its two phases: the HASH phase (classify + set_hash_kernel, or set_hash_wave_kernel for a small set) fills the
// record table of `epoch`; the WALK phase (set_walk_kernel) may then run any number of times against that table, with keys, roots and
// outputs of its own.  a.n == 0 in the hash phase: only the clearing (nothing will walk).  launch_mpt_verify_nodeset = both, once.
hipError_t launch_nodeset_hash(const VerifyArgs& a, uint32_t total_nodes, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch,
                               const uint32_t salt[2], hipStream_t st, const NodesetTune& tune);
hipError_t launch_nodeset_walk(const VerifyArgs& a, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch, const uint32_t salt[2],
                               hipStream_t st);
// poststate.hip.h (included by mpt_verify_nodeset.hip): the post-state root behind the pre-state kernels
// (phant_exec_witness_poststate).  Every pointer is device memory of the call; keys 0 .. na are the accounts, na .. na + ns the slots.
// a node the post-state build emitted: its bytes in the sink's blob and the position it was built for -- the trie (an account's
// index, n_accounts = the state trie), the item of the call's list that carries it, the branch depth d + 1 it was built at (0: the
// trie's root) and whether it is that branch itself (1) or the child attached to it (0).  No two nodes of a call share all four.
struct PoststateNodeDesc {
    uint64_t off;
    uint32_t len, trie, item, where;  // where = (d + 1) << 1 | branch
};
struct PoststateArgs {
    const uint8_t* nodes;
    uint64_t nodes_len;
    uint32_t na, ns;
    const uint8_t* keys;            // (na + ns) x 32: the hashed keys
    const uint8_t* parent_root;     // 32
    uint8_t* acc_status;            // as the pre-state kernels left them; failures of this phase are added
    uint8_t* slot_status;
    const uint64_t* acc_voff;
    const uint32_t* acc_vlen;
    const uint64_t* slot_voff;
    const uint32_t* slot_vlen;
    const uint64_t* pre_nonces;
    const uint8_t* pre_balances;
    const uint8_t* pre_sroots;      // na x 32: the proven storage roots (the roots the storage tries are walked from)
    const uint8_t* pre_code_hashes;
    const uint32_t* slot_account;   // ns
    const uint32_t* slot_first;     // na + 1
    const uint8_t* op;              // na: PHANT_POST_*
    const uint64_t* post_nonces;
    const uint8_t* post_balances;
    const uint8_t* post_code_hashes;
    const uint8_t* slot_write;      // ns, may be null
    const uint8_t* post_slot_vals;  // ns x 32
    uint8_t* post_sroots;           // na x 32, out
    uint8_t* state_root;            // 32, out
    uint32_t* acc_flag;             // na, zeroed by the caller
    uint8_t* act;                   // na + ns
    uint32_t* seg_of;               // na + ns: the trie a key lives in (a slot: its account; an account: na)
    const uint32_t* order;          // na + ns: the keys by (trie, hashed key)
    uint8_t* key_bad;               // na + ns, zeroed by the caller
    uint32_t* cnt;                  // na + ns + 1 (16-byte aligned): items per key, then their offsets
    uint32_t* scan_scratch;         // scan_scratch_entries(na + ns + 1)
    void* items_raw;                // cap_items x POSTSTATE_ITEM_BYTES
    uint32_t cap_items;
    uint32_t* counters;             // the pre-state's PRE_CNT_*, then POST_CNT_*: zeroed by the caller
    // phant_exec_witness_advance: where the lanes leave every hashed node they build (all null / zero: phant_exec_witness_poststate)
    uint8_t* sink_blob;             // sink_cap_bytes: the nodes back to back, in the order the lanes reserved their room
    PoststateNodeDesc* sink_desc;   // sink_cap_desc: which position of which trie each of them is
    unsigned long long* sink_bytes; // bytes reserved so far (beyond sink_cap_bytes: counted, not written); zeroed by the caller
    uint32_t* sink_cnt;             // POST_SINK_*: zeroed by the caller
    const uint32_t* sink_undecided; // may be null: the device sort's flag -- != 0: this run's key order is not one, it will be discarded
    uint64_t sink_cap_bytes;
    uint32_t sink_cap_desc;
    // phant_mpt_verify_ranges (range_verify.hip.h; both null: the post-state calls): every trie of the call stands for itself
    uint32_t* trie_bad;             // per trie, zeroed by the caller: != 0: this trie cannot be built (nothing else of the call is affected)
    const uint8_t* leaf_vals;       // where the value of an IK_LEAF_OLD item with key != 0 lies (src is an offset in here, not in nodes)
};
constexpr size_t POSTSTATE_ITEM_BYTES = 96;
enum : uint32_t { POST_SINK_NODES = 0, POST_SINK_OVERFLOW = 1 };  // PoststateArgs::sink_cnt
// the list's length (may exceed cap_items: run again), what cannot happen, keys whose emit walk failed (counted apart from PRE_CNT_FAILED,
// which the lanes of that launch read)
enum : uint32_t { POST_CNT_ITEMS = 3, POST_CNT_INTERNAL = 4, POST_CNT_EMIT_FAILED = 5 };
hipError_t launch_poststate_actions(const PoststateArgs& p, hipStream_t st);
hipError_t launch_poststate_build(const PoststateArgs& p, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch, const uint32_t salt[2],
                                  hipStream_t st);
// range_verify.hip.h (included by mpt_verify_nodeset.hip): range proofs (phant_mpt_verify_ranges) on the record table of the call's
// epoch.  Every pointer is device memory of the call; the inputs as include/phant_gpu.h describes them.
struct RangeArgs {
    uint32_t n_ranges, n_leaves, n_nodes;
    const uint8_t* roots;         // n_ranges x 32
    const uint8_t* origins;       // n_ranges x 32
    const uint32_t* leaf_first;   // n_ranges + 1
    const uint8_t* has_proof;     // n_ranges
    const uint8_t* keys;          // n_leaves x 32
    const uint8_t* vals;
    const uint64_t* val_off;      // n_leaves + 1
    uint64_t vals_len;
    const uint8_t* nodes;
    const uint64_t* node_off;     // n_nodes + 1
    uint64_t nodes_len;
    // the call's workspace
    uint32_t* ctl;                // RANGE_CTL_*: zeroed by the caller
    uint32_t* counters;           // 8: the build's PRE_CNT_* / POST_CNT_*, zeroed by the caller
    uint32_t* bad_leaf;           // n_ranges: the least leaf that breaks a rule (the caller fills it with ff..ff)
    uint32_t* walk_err;           // 2 x n_ranges: what the origin's / the last key's walk failed with, zeroed by the caller
    uint32_t* more;               // n_ranges: the right walker emitted something, zeroed by the caller
    uint32_t* trie_bad;           // n_ranges, zeroed by the caller
    uint8_t* built_root;          // n_ranges x 32
    uint32_t* cnt;                // n_leaves + 2 n_ranges + 1 (16-byte aligned): items per lane, then their offsets
    uint32_t* scan_scratch;       // scan_scratch_entries(n_leaves + 2 n_ranges + 1)
    void* items_raw;              // cap_items x POSTSTATE_ITEM_BYTES
    uint32_t cap_items;
    uint32_t leaf_pass;           // 0: the leaves go through the branch lanes' attach (PHANT_DIAG_RANGES_NO_LEAF_PASS)
    // out
    uint8_t* status;              // n_ranges
    uint8_t* has_more;            // n_ranges
    uint8_t* computed_root;       // n_ranges x 32
    uint32_t* out_bad_leaf;       // n_ranges
};
// [CHECK] != 0: the device form's offsets are refused; [FAILED] ranges that are not VALID, [FIRST] n_ranges - the least of them (0: none),
// [ITEMS] the item list's length (beyond cap_items nothing was built: run again with that room)
enum : uint32_t { RANGE_CTL_CHECK = 0, RANGE_CTL_FAILED = 1, RANGE_CTL_FIRST = 2, RANGE_CTL_ITEMS = 3, RANGE_CTL_WORDS = 4 };
hipError_t launch_range_check(const RangeArgs& a, hipStream_t st);  // range_check_kernel
hipError_t launch_range_verify(const RangeArgs& a, uint32_t cap_nodes, uint8_t* ws, uint32_t epoch, const uint32_t salt[2], hipStream_t st);
hipError_t launch_mpt_verdict(const uint8_t* d_status, const uint32_t* d_root_idx, uint32_t n,
                              uint32_t n_roots, uint32_t* d_fail_count, hipStream_t st);

// radix_sort.hip: the order of n 32-byte digests (ascending; grouped by d_seg_of[i] < n_seg when given) as a permutation in
// device memory inside `ws` (order_workspace_bytes(n)); *d_flag_out != 0 afterwards: not decided, order it another way
size_t order_workspace_bytes(uint32_t n);
hipError_t launch_order_digests(const uint8_t* d_digests, const uint32_t* d_seg_of, uint32_t n, uint32_t n_seg, uint8_t* ws,
                                uint32_t** d_order_out, uint32_t** d_flag_out, uint32_t prefix_bits, hipStream_t st);

// radix_sort.hip: the stable sort of n (64-bit key, 32-bit value) pairs by the low `bits` key bits (rounded up to whole bytes; three
// launches per byte).  The pairs end up in *keys_out / *vals_out, which are the given buffers or their alternates; hist:
// sort_hist_entries(n) counters, digit_totals: 512 counters the caller has zeroed.
size_t sort_hist_entries(uint32_t n);
hipError_t launch_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt, uint32_t n, uint32_t bits, uint32_t* hist,
                             uint32_t* digit_totals, uint64_t** keys_out, uint32_t** vals_out, hipStream_t st);
// `bits` for keys that are pre-state rows: they run from 0 to n_accounts (n_accounts: no row)
inline uint32_t sort_key_bits(uint32_t n_accounts) {
    uint32_t bits = 1;
    while (bits < 32u && (n_accounts >> bits)) ++bits;
    return bits;
}

// exclusive prefix sum of d[0 .. n) in place; d 16-byte aligned, scratch = scan_scratch_entries(n) counters of device memory
size_t scan_scratch_entries(uint32_t n);
hipError_t launch_exclusive_scan_u32(uint32_t* d, uint32_t n, uint32_t* scratch, hipStream_t st);

}  // namespace phant
