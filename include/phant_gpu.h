/*
 * phant_gpu.h -- C-ABI of libphant_gpu: the MI355X (gfx950) implementation of
 * phant's Keccak-256 / Merkle-Patricia-Trie hot path.
 *
 * This is the drop-in boundary.  phant (Zig) has no FFI on this path today:
 * `mptize` and `keccak256` are plain Zig functions.  A maintainer keeps their
 * Zig signatures and forwards to the entry points below through `@cImport`
 * exactly as src/blockchain/vm.zig:1-3 does for evmone and
 * src/crypto/ecdsa.zig:2,15 for libsecp256k1 (binding shown in
 * INTEGRATION.md).  Conventions follow those existing C boundaries:
 *   - plain C, `extern "C"`, pointers + sizes only;
 *   - every call returns int32_t: 0 = PHANT_OK, < 0 = PHANT_E_*; nothing
 *     aborts or throws across the boundary.  A malformed *proof* is not an
 *     error, it is a per-proof status byte;
 *   - all buffers are caller-owned and only borrowed for the duration of the
 *     call (for *_dev entry points: until the ctx stream has run the work --
 *     phant_stream_sync);
 *   - a ctx is externally synchronised (one thread at a time), independent
 *     ctxs may be used concurrently (cf. the single shared *Blockchain in
 *     src/main.zig:143-149);
 *   - there is NO CPU fallback: without a usable gfx950 device
 *     phant_ctx_create fails with PHANT_E_NO_DEVICE.
 *
 * Two families of entry points:
 *   host form   `phant_xxx(ctx, host pointers...)`  synchronous; stages H2D,
 *               runs the kernels, copies results back.  This is what the Zig
 *               shim calls.
 *   device form `phant_xxx_dev(ctx, device pointers...)`  asynchronous on the
 *               ctx stream, inputs and outputs already resident in HBM (what
 *               bench.py times, and what a caller that keeps witnesses on the
 *               GPU uses).  Device loads are dword-granular: of a byte buffer
 *               (`d_blob`, `d_nodes`, `d_keys`) the kernels may read every
 *               4-byte-aligned dword that holds one of its bytes, so a buffer
 *               must not end inside a dword that the device cannot read --
 *               true of anything hipMalloc'd (or a sub-range of it); nothing
 *               beyond that dword is ever touched.
 */
#ifndef PHANT_GPU_H
#define PHANT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PHANT_API __attribute__((visibility("default")))
#else
#define PHANT_API
#endif

#define PHANT_OK 0
#define PHANT_E_INVALID_ARG (-1)
#define PHANT_E_OOM (-2)
#define PHANT_E_DEVICE (-3)     /* a HIP call failed; see phant_last_error */
#define PHANT_E_NO_DEVICE (-4)  /* no gfx950 device / device index out of range */
#define PHANT_E_UNSORTED (-5)   /* mptize precondition, src/mpt/mpt.zig:39 */
#define PHANT_E_UNSUPPORTED (-6)

/* Per-proof status written by phant_mpt_verify_batch*.  Values < 16 other
 * than 0 mean "the proof is valid". */
#define PHANT_PROOF_INVALID_EMPTY 0 /* proof has no nodes */
#define PHANT_PROOF_PRESENT 1       /* key is in the trie; value_off/len set */
#define PHANT_PROOF_ABSENT 2        /* proof shows the key is NOT in the trie */
#define PHANT_PROOF_BAD_HASH 16     /* a node does not hash to its reference */
#define PHANT_PROOF_BAD_RLP 17      /* a node is not canonical RLP */
#define PHANT_PROOF_BAD_NODE 18     /* canonical RLP but not an MPT node */
#define PHANT_PROOF_EXTRA_NODES 19  /* walk finished with nodes left over */
#define PHANT_PROOF_MISSING_NODE 20 /* walk needs a node the proof lacks */
#define PHANT_PROOF_BAD_INPUT 21    /* node_off / proof_first_node inconsistent */
#define PHANT_PROOF_MISMATCH 22     /* phant_witness_verify only: the proof is valid, but what it proves
                                       contradicts what the witness declares (storageHash, codeHash, nonce,
                                       balance, slot value), or its root is not anchored because the
                                       account proof above it failed */
#define PHANT_PROOF_BAD_VALUE 23    /* phant_exec_witness_prestate only: the proof is valid, but the value it proves is not a
                                       canonical account body rlp([nonce, balance, storageRoot, codeHash]) / slot value
                                       rlp(minimal non-zero integer of 1..32 bytes) */

typedef struct phant_ctx phant_ctx;

#define PHANT_CTX_OWN_STREAM 1u   /* flags: ignore `stream`, create a private non-blocking stream */
/* flags: how many trie levels, counted from the root, the verify pipeline deduplicates across the proofs of a
 * batch (byte-compares copies instead of hashing them); deeper nodes are hashed in place.  Default (field 0):
 * chosen from the batch -- none for batches of less than 72 MB of nodes (the chip hashes those whole in a few rounds
 * of waves), otherwise the levels with fewer groups than proofs; PHANT_CTX_DEDUP_LEVELS(0): every shipped node is
 * hashed, whatever the batch.  A sizing hint of the one pipeline: correctness does not depend on it. */
#define PHANT_CTX_DEDUP_LEVELS_SHIFT 8
#define PHANT_CTX_DEDUP_LEVELS_MASK 0x1f00u
#define PHANT_CTX_DEDUP_LEVELS(n) ((((uint32_t)(n) + 1u) << PHANT_CTX_DEDUP_LEVELS_SHIFT) & PHANT_CTX_DEDUP_LEVELS_MASK)

typedef struct phant_opts {
    uint32_t struct_size; /* = sizeof(phant_opts) */
    int32_t device;       /* HIP device ordinal */
    void *stream;         /* hipStream_t to run on; NULL = the device's default stream */
    uint32_t flags;       /* PHANT_CTX_* */
} phant_opts;

PHANT_API const char *phant_version(void);
PHANT_API int32_t phant_device_count(void);
PHANT_API int32_t phant_ctx_create(const phant_opts *opts, phant_ctx **out);
PHANT_API void phant_ctx_destroy(phant_ctx *ctx);
/* message for the last failing call on this ctx ("" if none); ctx-owned */
PHANT_API const char *phant_last_error(const phant_ctx *ctx);
/* rebind the ctx to another hipStream_t (e.g. torch's current stream; NULL =
 * the default stream) */
PHANT_API int32_t phant_set_stream(phant_ctx *ctx, void *stream);
PHANT_API int32_t phant_stream_sync(phant_ctx *ctx);

/* ------------------------------------------------------------------ Keccak
 * Replaces src/crypto/hasher.zig:4-8   `keccak256(data: []const u8) Hash32`
 *      and src/crypto/hasher.zig:10-17 `keccak256WithPrefix(prefix, data)`.
 * Keccak-256 = Keccak[c=512], pad 0x01..0x80, rate 136 (NOT SHA3-256). */
PHANT_API int32_t phant_keccak256(phant_ctx *ctx, const uint8_t *data, uint64_t len,
                                  uint8_t out[32]);
PHANT_API int32_t phant_keccak256_with_prefix(phant_ctx *ctx, const uint8_t *prefix,
                                              uint64_t prefix_len, const uint8_t *data,
                                              uint64_t len, uint8_t out[32]);
/* n messages; message i = blob[off[i] .. off[i+1]); out = n x 32 bytes.
 * The batched form of hasher.zig:4-8 (one call per node at mpt.zig:207,245,277
 * becomes one call per level / per witness). */
PHANT_API int32_t phant_keccak256_batch(phant_ctx *ctx, const uint8_t *blob, const uint64_t *off,
                                        uint32_t n, uint8_t *out);
PHANT_API int32_t phant_keccak256_batch_dev(phant_ctx *ctx, const uint8_t *d_blob,
                                            const uint64_t *d_off, uint32_t n, uint8_t *d_out);
/* SHA-256 (FIPS 180-4) under the same contract: n messages, message i = blob[off[i] .. off[i+1]), out = n x 32 bytes; n == 0 is
 * PHANT_OK; the host form refuses offsets that go backwards (PHANT_E_INVALID_ARG), the device form wants d_out 16-byte aligned.  The
 * execution layer's second hash function: EIP-7685 commits a block's requests with it (phant_block_requests below computes
 * requests_hash for a chain segment), and a client that receives `executionRequests` with engine_newPayloadV4 hashes them with this
 * before it can check blockHash.  A lane per message. */
PHANT_API int32_t phant_sha256_batch(phant_ctx *ctx, const uint8_t *blob, const uint64_t *off, uint32_t n, uint8_t *out);
PHANT_API int32_t phant_sha256_batch_dev(phant_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_off, uint32_t n, uint8_t *d_out);
/* n messages of msg_len bytes each at d_blob + i*stride (BASELINE config 2:
 * msg_len = stride = 136). */
PHANT_API int32_t phant_keccak256_fixed_dev(phant_ctx *ctx, const uint8_t *d_blob,
                                            uint32_t msg_len, uint64_t stride, uint32_t n,
                                            uint8_t *d_out);

/* ------------------------------------------------- other bulk Keccak users
 * the per-item keccak256 calls next to the trie path, batched.
 *
 * Logs bloom -- replaces src/types/receipt.zig:37-48 `calculateLogsBloom(logs) LogsBloom` (and its
 * `addToBloom`, :50-63) for all receipts of a block at once.  The bloom items of the block are flattened:
 * item k = items[item_off[k] .. item_off[k+1]) is a log's 20-byte address or one of its 32-byte topics
 * (any length is accepted) and belongs to receipt item_receipt[k]; blooms = n_receipts x 256 bytes out, each
 * the OR over its items of the three bits addToBloom sets (bit index 0x7ff - (big-endian u16 at hash[2i] &
 * 0x7ff), i = 0..2, counted from the most significant bit of byte 0).  An item whose receipt index is
 * >= n_receipts is ignored.  Device form: d_blooms 4-byte aligned; zeroed by the call. */
PHANT_API int32_t phant_logs_bloom(phant_ctx *ctx, const uint8_t *items, const uint64_t *item_off,
                                   const uint32_t *item_receipt, uint32_t n_items, uint32_t n_receipts,
                                   uint8_t *blooms);
PHANT_API int32_t phant_logs_bloom_dev(phant_ctx *ctx, const uint8_t *d_items, const uint64_t *d_item_off,
                                       const uint32_t *d_item_receipt, uint32_t n_items,
                                       uint32_t n_receipts, uint8_t *d_blooms);
/* Sender addresses -- the hashing half of src/signer/signer.zig:77-78 `keccak256(pubkey[1..])[12..]` for a
 * block's recovered public keys: key i = 64 bytes at pubkeys + i * stride (stride >= 64; pass pk + 1 and
 * stride 65 for 0x04-tagged keys), out20 = n x 20 bytes.  (For keys recovered elsewhere; phant_ecrecover_batch
 * below recovers and hashes in one launch.)  Device form: d_out20 4-byte aligned.
 *
 * Transaction hashes (src/types/transaction.zig:183-187,223-228,256-261 = keccak256 of the EIP-2718 bytes) and
 * code hashes (src/blockchain/vm.zig:284-298; keccak256("") is its `empty_hash`) are phant_keccak256_batch
 * over the respective byte strings. */
PHANT_API int32_t phant_sender_addresses(phant_ctx *ctx, const uint8_t *pubkeys, uint64_t stride,
                                         uint32_t n, uint8_t *out20);
PHANT_API int32_t phant_sender_addresses_dev(phant_ctx *ctx, const uint8_t *d_pubkeys, uint64_t stride,
                                             uint32_t n, uint8_t *d_out20);

/* ------------------------------------------------- a block's receipts
 * What src/blockchain/blockchain.zig:76-90 `runBlock` compares with the header once a block has executed, from the receipts'
 * FIELDS in one call and one synchronisation: every receipt's bloom (receipt.zig:37-63), its encoding
 *     [tx_type, when != 0] ++ rlp([status, cumulative_gas_used, bloom, [ [address, [topics...], data] ... ]])
 * (receipt.zig:13-35; EIP-658: status 1 encodes as 0x01, 0 as 0x80; EIP-2718: the type byte in front -- the reference's
 * Receipt.encode has no prefix yet, tx_type 0 reproduces it), the receipts root (calculateMPTRoot over the encodings, key
 * rlp(index) as phant_index_root_rlp) and the block's logs bloom (the OR of all rows).  Nothing is encoded on the host.
 *
 * Input, struct-of-arrays: receipt i has tx_type[i] (0 = legacy, 1 .. 0x7f), status[i] (0 / 1), cum_gas[i] and the logs
 * [log_first[i], log_first[i+1]); log l has address[20 l .. 20 l + 20), the topics [topic_first[l], topic_first[l+1]) of 32
 * bytes each (any count) and the data bytes [data_off[l], data_off[l+1]).  log_first runs from 0 to n_logs, topic_first from
 * 0 to n_topics, data_off from 0 to data_bytes.  An array whose count is zero may be NULL.
 *
 * Lists that ride along (optional): n_lists lists of already encoded items as in phant_block_roots (list l = lists[l][list_off
 * [l][0] .. list_off[l][list_n[l]])), hashed in the SAME forest pass; receipts_at (<= n_lists) is the receipts' place among
 * them.  roots_out = (n_lists + 1) x 32 bytes in that order: transactions, receipts and withdrawals give transactions_root,
 * receipts_root and withdrawals_root from one call.  An empty list (or n_receipts == 0) gives mpt.zig:10 empty_mpt_root; no
 * receipts give a zero bloom.
 *
 * Output, any pointer may be NULL (not wanted): receipts_root[32]; logs_bloom[256]; blooms = n_receipts x 256; roots_out;
 * encoded / encoded_off = the encodings back to back in index order and their n_receipts + 1 offsets.  encoded_len is always
 * written; if it exceeds encoded_cap, or n_receipts + 1 exceeds encoded_off_cap, the call still returns PHANT_OK and neither
 * buffer is touched (a NULL buffer has no capacity to exceed): call again with the reported size.
 *
 * PHANT_E_INVALID_ARG: a wrong struct_size, a NULL array with a non-zero count, status > 1, tx_type > 0x7f, receipts_at >
 * n_lists, offsets that go backwards or do not run from 0 to the stated totals.  PHANT_E_UNSUPPORTED: a receipt longer than
 * 2^32 - 1 bytes, or more than 4 GiB of trie values in one call.  The host form checks before anything is copied.
 *
 * Device form: every array (and every list, with list_off[l] running from 0 to list_bytes[l]) is device memory, cum_gas /
 * data_off / list_off[l] / encoded_off 8-byte and log_first / topic_first 4-byte aligned (kernels read and write them as
 * words; the other outputs are copied as bytes and need no alignment); `lists`, `list_off`, `list_n`, `list_bytes` and both
 * structs themselves are host memory.  The caller's
 * offsets and flags are checked on the device before any kernel indexes with them.  Outputs stay in device memory; the call
 * synchronises the ctx stream on the way (encoded_len is valid when it returns), the copies into the output buffers are in
 * stream order behind it. */
typedef struct phant_receipts_in {
    uint32_t struct_size; /* = sizeof(phant_receipts_in) */
    uint32_t n_receipts;
    uint32_t n_logs;
    uint32_t n_topics;
    uint64_t data_bytes;
    const uint8_t *tx_type;      /* n_receipts */
    const uint8_t *status;       /* n_receipts */
    const uint64_t *cum_gas;     /* n_receipts */
    const uint32_t *log_first;   /* n_receipts + 1 */
    const uint8_t *address;      /* n_logs x 20 */
    const uint32_t *topic_first; /* n_logs + 1 */
    const uint64_t *data_off;    /* n_logs + 1 */
    const uint8_t *topics;       /* n_topics x 32 */
    const uint8_t *data;         /* data_bytes */
    const uint8_t *const *lists;     /* n_lists */
    const uint64_t *const *list_off; /* n_lists, list_n[l] + 1 entries each */
    const uint32_t *list_n;          /* n_lists */
    const uint64_t *list_bytes;      /* n_lists; device form only */
    uint32_t n_lists;
    uint32_t receipts_at;
} phant_receipts_in;
typedef struct phant_receipts_out {
    uint32_t struct_size;     /* = sizeof(phant_receipts_out) */
    uint32_t encoded_off_cap; /* entries of encoded_off */
    uint64_t encoded_cap;     /* bytes of encoded */
    uint8_t *receipts_root;
    uint8_t *logs_bloom;
    uint8_t *blooms;
    uint8_t *encoded;
    uint64_t *encoded_off;
    uint8_t *roots_out;
    /* result */
    uint64_t encoded_len;
} phant_receipts_out;
PHANT_API int32_t phant_block_receipts(phant_ctx *ctx, const phant_receipts_in *in, phant_receipts_out *out);
PHANT_API int32_t phant_block_receipts_dev(phant_ctx *ctx, const phant_receipts_in *in, phant_receipts_out *out);

/* ------------------------------------------------- block headers: encode, hash, validate chain segments
 * src/blockchain/blockchain.zig:100-145 `validateBlockHeader` for n headers in one call: every header's fork-aware RLP
 * encoding (src/types/block.zig:51-69), its hash, and for every header but a segment's first the checks of the header
 * against the one before it.  Nothing is encoded or hashed on the host.
 *
 * Input, struct-of-arrays in the field order of block.zig:15-36; header i has parent_hash[32 i ..), fee_recipient[20 i ..),
 * logs_bloom[256 i ..), nonce[8 i ..), base_fee[32 i ..) (big-endian u256), the uint64_t fields, extra_data[extra_off[i] ..
 * extra_off[i+1]) (extra_off runs from 0, never backwards) and n_fields[i] = how many list items it encodes: 15, 16 (+ base
 * fee), 17 (+ withdrawals root), 19 (+ blob gas used, excess blob gas), 20 (+ parent beacon root) or 21 (+ requests hash).
 * An array that no header of the call encodes may be NULL, and so may extra_data when every header's is empty.
 * seg_first (NULL: one segment): n_segs + 1 strictly increasing indices from 0 to n; the first header of a segment is its
 * ANCHOR (the reference's prev_block): it is hashed, no rule is applied to it.  expected_hash (NULL: none): n x 32.
 *
 * Encoding: one RLP list of the first n_fields items; hashes, address, bloom, prev_randao and nonce as strings of their
 * full width, the integers and base_fee minimal big-endian (zero is 0x80), extra_data by RLP's string rules, any length.
 *
 * flags[i], bit k = the k-th check of validateBlockHeader failed (p = the header before; integers are exact, nothing wraps):
 * the lowest set bit is the error the reference returns, and all failed checks are reported. */
#define PHANT_HDR_GAS_LIMIT_TOO_HIGH 0x0001u /* gas_limit >= p.gas_limit + p.gas_limit / 1024 */
#define PHANT_HDR_GAS_LIMIT_TOO_LOW 0x0002u  /* gas_limit <= p.gas_limit - p.gas_limit / 1024 */
#define PHANT_HDR_GAS_LIMIT_MINIMUM 0x0004u  /* gas_limit < 5000 */
#define PHANT_HDR_GAS_LIMIT_EXCEEDED 0x0008u /* gas_used > gas_limit */
#define PHANT_HDR_BASE_FEE 0x0010u           /* base_fee is not the EIP-1559 value that follows from p (see below) */
#define PHANT_HDR_TIMESTAMP 0x0020u          /* timestamp <= p.timestamp */
#define PHANT_HDR_NUMBER 0x0040u             /* number != p.number + 1 */
#define PHANT_HDR_EXTRA_DATA 0x0080u         /* more than 32 bytes of extra_data */
#define PHANT_HDR_DIFFICULTY 0x0100u         /* difficulty != 0 */
#define PHANT_HDR_NONCE 0x0200u              /* nonce is not eight zero bytes */
#define PHANT_HDR_UNCLE_HASH 0x0400u         /* uncle_hash != keccak256(0xc0) */
#define PHANT_HDR_PARENT_HASH 0x0800u        /* parent_hash != hash(p) */
#define PHANT_HDR_EXPECTED_HASH 0x1000u      /* expected_hash given and != hash(header): the one bit an anchor can have */
/* Expected base fee, t = p.gas_limit / 2, all divisions floor: p.gas_used == t: p.base_fee; above: p.base_fee +
 * max(p.base_fee (p.gas_used - t) / t / 8, 1); below: p.base_fee - p.base_fee (t - p.gas_used) / t / 8.  Where the reference
 * would panic -- t == 0 with p.gas_used != 0, or exactly one of the two headers without a base fee (n_fields 15) -- the bit
 * is set; two headers without one skip the rule; an expected value beyond 2^256 - 1 equals no field: the bit is set.
 *
 * Output, any pointer may be NULL: hashes = n x 32; flags = n words; enc / enc_off = the encodings back to back in index
 * order and their n + 1 offsets.  first_bad (the least i with flags[i] != 0, n if none) and enc_len are always written; if
 * enc_len exceeds enc_cap the call still returns PHANT_OK, neither enc nor enc_off is touched (a NULL enc has no capacity to
 * exceed) and the other outputs arrive: call again with the reported size.
 *
 * A bad header is a flag, never an error.  PHANT_E_INVALID_ARG: a wrong struct_size, a NULL array that a header needs, an
 * n_fields outside the six values, extra_off or seg_first as not described above.  PHANT_E_UNSUPPORTED: 700 n + the
 * extra data's bytes, the call's bound on its encodings, is 4 GiB or more.  n == 0 is PHANT_OK with first_bad = 0.  The host
 * form checks before anything is copied.
 *
 * Device form: every array is device memory, the uint64_t arrays and enc_off 8-byte, extra_off / seg_first / flags 4-byte
 * aligned; both structs are host memory.  n_fields, extra_off and seg_first are checked on the device before any kernel
 * indexes with them.  Outputs stay in device memory; the call synchronises the ctx stream on the way (enc_len and first_bad
 * are valid when it returns), the copies into hashes are in stream order behind it. */
typedef struct phant_headers_in {
    uint32_t struct_size; /* = sizeof(phant_headers_in) */
    uint32_t n;
    uint32_t n_segs;      /* with seg_first */
    uint32_t reserved;    /* 0 */
    const uint8_t *parent_hash;        /* n x 32 */
    const uint8_t *uncle_hash;         /* n x 32 */
    const uint8_t *fee_recipient;      /* n x 20 */
    const uint8_t *state_root;         /* n x 32 */
    const uint8_t *transactions_root;  /* n x 32 */
    const uint8_t *receipts_root;      /* n x 32 */
    const uint8_t *logs_bloom;         /* n x 256 */
    const uint64_t *difficulty;        /* n */
    const uint64_t *number;            /* n */
    const uint64_t *gas_limit;         /* n */
    const uint64_t *gas_used;          /* n */
    const uint64_t *timestamp;         /* n */
    const uint8_t *extra_data;
    const uint32_t *extra_off;         /* n + 1 */
    const uint8_t *prev_randao;        /* n x 32 */
    const uint8_t *nonce;              /* n x 8 */
    const uint8_t *base_fee;           /* n x 32, big-endian; n_fields >= 16 */
    const uint8_t *withdrawals_root;   /* n x 32; n_fields >= 17 */
    const uint64_t *blob_gas_used;     /* n; n_fields >= 19 */
    const uint64_t *excess_blob_gas;   /* n; n_fields >= 19 */
    const uint8_t *parent_beacon_root; /* n x 32; n_fields >= 20 */
    const uint8_t *requests_hash;      /* n x 32; n_fields == 21 */
    const uint8_t *n_fields;           /* n */
    const uint32_t *seg_first;         /* n_segs + 1, or NULL */
    const uint8_t *expected_hash;      /* n x 32, or NULL */
} phant_headers_in;
typedef struct phant_headers_out {
    uint32_t struct_size; /* = sizeof(phant_headers_out) */
    uint32_t first_bad;   /* result */
    uint64_t enc_cap;     /* bytes of enc */
    uint8_t *hashes;
    uint32_t *flags;
    uint8_t *enc;
    uint64_t *enc_off;
    uint64_t enc_len;     /* result */
} phant_headers_out;
PHANT_API int32_t phant_header_chain(phant_ctx *ctx, const phant_headers_in *in, phant_headers_out *out);
PHANT_API int32_t phant_header_chain_dev(phant_ctx *ctx, const phant_headers_in *in, phant_headers_out *out);
/* Host only, strict: header i = blob[off[i] .. off[i+1]), or with PHANT_HEADERS_FROM_BLOCKS the first item of the block
 * encoding there.  Writes the caller's arrays behind fields_out (ALL of them non-NULL and sized for n; extra_data sized by
 * the input bytes; seg_first / expected_hash are not touched) and sets fields_out->n, so that fields_out can go straight into
 * phant_header_chain.
 * Strict: canonical RLP, one of the six field counts, exact widths, minimal integers that fit their field, nothing behind
 * the item -- so encode(decode(x)) == x.  status[i] != 0: refused; its n_fields is 0 (which phant_header_chain refuses) and
 * its other fields are zero.  Returns PHANT_E_INVALID_ARG for NULL arguments, offsets that go backwards or unknown flags. */
#define PHANT_HEADERS_FROM_BLOCKS 1u
PHANT_API int32_t phant_headers_decode_rlp(const uint8_t *blob, const uint64_t *off, uint32_t n, uint32_t flags,
                                           phant_headers_in *fields_out, uint8_t *status);

/* ------------------------------------------------- sender recovery (secp256k1)
 * src/signer/signer.zig:40-79 `get_sender` / src/crypto/ecdsa.zig:19-21 `erecover` for a block's transactions in one
 * launch: one lane per signature does SEC 1 section 4.1.6 and hashes the key it found.  Status byte per item: */
#define PHANT_SIG_OK 0
#define PHANT_SIG_BAD_RANGE 1     /* r or s is 0 or >= n */
#define PHANT_SIG_HIGH_S 2        /* PHANT_RECOVER_LOW_S: s > n / 2 */
#define PHANT_SIG_BAD_RECID 3     /* recid > 3, or r + n (recid & 2) is no field element */
#define PHANT_SIG_NOT_ON_CURVE 4  /* no curve point has that x */
#define PHANT_SIG_INFINITY 5      /* the recovered key is the point at infinity */
#define PHANT_SIG_BAD_TX 6        /* phant_tx_senders: undecodable, non-canonical or unknown transaction type */
#define PHANT_SIG_BAD_V 7         /* phant_tx_senders: v is neither 27 / 28 nor 35 + 2 chain_id + {0, 1}; y_parity > 1 */
#define PHANT_RECOVER_LOW_S 1u    /* src/crypto/ecdsa.zig:28-36 validateSignatureFields: reject s > n / 2 */
/* hashes, r, s: n x 32 bytes, big-endian; recid: n bytes.  The checks run in this order, so a tuple that is wrong in two
 * ways has ONE status: recid > 3 -> BAD_RECID; r == 0, r >= n, s == 0 or s >= n -> BAD_RANGE; with PHANT_RECOVER_LOW_S,
 * s > n / 2 -> HIGH_S; x = r + (recid & 2 ? n : 0), x >= p -> BAD_RECID; x on no curve point -> NOT_ON_CURVE; y's parity =
 * recid & 1; Q = (-z / r) G + (s / r) R; Q at infinity -> INFINITY; else OK.  pubkeys64 (n x 64 bytes, x || y big-endian),
 * addresses20 (n x 20 bytes) and status (n bytes) may each be NULL, not all three; a failed item's outputs are zeroed.
 * n == 0 is PHANT_OK.  NULL inputs with n > 0 or unknown flag bits: PHANT_E_INVALID_ARG.  Device form: every array is
 * device memory (no alignment asked), nothing is synchronised; the first call on a context also computes the context's
 * table of multiples of G (one 16 KiB allocation and one launch). */
PHANT_API int32_t phant_ecrecover_batch(phant_ctx *ctx, const uint8_t *hashes, const uint8_t *r, const uint8_t *s,
                                        const uint8_t *recid, uint32_t n, uint32_t flags, uint8_t *pubkeys64,
                                        uint8_t *addresses20, uint8_t *status);
PHANT_API int32_t phant_ecrecover_batch_dev(phant_ctx *ctx, const uint8_t *d_hashes, const uint8_t *d_r,
                                            const uint8_t *d_s, const uint8_t *d_recid, uint32_t n, uint32_t flags,
                                            uint8_t *d_pubkeys64, uint8_t *d_addresses20, uint8_t *d_status);
/* `get_sender` for raw transactions: transaction i = txs[tx_off[i] .. tx_off[i+1]), a legacy RLP list, 0x01 || rlp or
 * 0x02 || rlp.  One call, one synchronisation: the host decodes each transaction strictly (canonical RLP, the field count
 * of its type, integers without leading zeros and within their width, `to` empty or 20 bytes, a well-formed access list;
 * anything else, or another type byte: BAD_TX) and builds its signing preimage by putting the item bytes, verbatim and
 * without v / r / s, under a new list header (EIP-155: followed by chain_id, 0, 0); the device hashes the preimages and
 * recovers with PHANT_RECOVER_LOW_S.  Legacy v: 27 / 28 -> the pre-EIP-155 preimage; 35 + 2 chain_id + {0, 1} -> the
 * EIP-155 preimage; anything else BAD_V (signer.zig:52-59).  Typed: recid = y_parity, > 1 -> BAD_V.
 * ONE DEVIATION from the reference: signer.zig:87 hashes every legacy transaction with the EIP-155 preimage whenever
 * the signer's chain id is non-zero, also for v = 27 / 28; this call hashes what was signed.
 * addresses20 (n x 20) or status (n) may be NULL, not both; a failed item's address is zeroed. */
PHANT_API int32_t phant_tx_senders(phant_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n,
                                   uint64_t chain_id, uint8_t *addresses20, uint8_t *status);

/* ------------------------------------------------- a block's transactions: decode, hash, pre-execution checks
 * Everything src/blockchain/blockchain.zig `applyBody` needs of a transaction before it touches state, for n raw transactions in
 * one call: the decoded fields (src/types/transaction.zig:152-273), Tx.hash, the signing hash and the sender
 * (src/signer/signer.zig:40-188), `calculateIntrinsicCost` (blockchain.zig:355-381) and the state-free rules of
 * `checkTransaction` / `validateTransaction` (:237-260, :345-353).  The raw bytes are uploaded once and read by kernels only;
 * nothing is decoded, spliced or hashed on the host.
 *
 * Input: transaction i = txs[tx_off[i] .. tx_off[i+1]) (n + 1 offsets from 0, never backwards; device form: up to tx_bytes), a
 * legacy RLP list, 0x01 || rlp or 0x02 || rlp, decoded exactly as strictly as phant_tx_senders decodes; chain_id; base_fee
 * (32 bytes big-endian, HOST memory in both forms; NULL skips the two fee rules); block_gas_limit, read with
 * PHANT_TXS_HAVE_GAS_LIMIT.  PHANT_TXS_NO_RECOVERY skips the secp256k1 launch: sender and sig_status must then be NULL.
 *
 * Output, struct-of-arrays of n rows, any pointer may be NULL.  Integers of 32 bytes are big-endian.
 *   tx_hash (32)       keccak256 of the raw bytes; always defined (a zero-length transaction: the hash of the empty string)
 *   sig_hash (32)      what was signed: the items in front of v under a list header of their own (EIP-155: + chain_id, 0, 0)
 *   sender (20), sig_status (1)   value for value what phant_tx_senders writes for the same input (PHANT_SIG_*; types 0 - 2, the only
 *                      ones either call decodes -- phant_block_transactions_ex below goes further)
 *   sig (65)           r || s || recid
 *   type (1), chain_id, nonce, gas_limit (uint64_t)   chain_id of a legacy transaction: (v - 35) >> 1, 0 for v = 27 / 28
 *   gas_price (32)     getGasPrice(): max_fee_per_gas for type 2
 *   priority_fee (32)  max_priority_fee_per_gas; the gas price for types 0 and 1
 *   value (32), to (20; zero for a creation, which is a flag bit)
 *   data_off (uint64_t, into txs), data_len (uint32_t); al_off / al_len: the access list's payload span in txs (0, 0 for a
 *   legacy transaction); al_addresses, al_keys (uint32_t): its tuples and its storage keys
 *   intrinsic_gas (uint64_t) = 21000 + 4 (zero data bytes) + 16 (non-zero data bytes) + 2400 al_addresses + 1900 al_keys, for a
 *                      creation + 32000 + 2 ceil(data_len / 32)   (src/blockchain/params.zig:7-15)
 *   effective_gas_price (32)  type 2: min(priority_fee, gas_price - base_fee) + base_fee, else gas_price; zero when base_fee is NULL
 *                      or a fee rule fails
 *   upfront_cost (32) = gas_limit x gas_price + value, what blockchain.zig:268-274 compares with the sender's balance
 *   flags (uint32_t)   below; every failed rule is reported, and the lowest set error bit is the error the reference returns first
 * A transaction that does not decode (PHANT_TX_UNDECODABLE) has zero rows except tx_hash, flags and sig_status (PHANT_SIG_BAD_TX);
 * none of the other rules is evaluated for it.  With PHANT_TX_BAD_V the fields and rules are there, sig_hash, sig and sender are zero.
 * first_bad (always written): the least i whose flags carry an error bit, n if none. */
#define PHANT_TXS_HAVE_GAS_LIMIT 1u
#define PHANT_TXS_NO_RECOVERY 2u
#define PHANT_TX_UNDECODABLE 0x001u        /* what phant_tx_senders calls PHANT_SIG_BAD_TX */
#define PHANT_TX_BAD_V 0x002u              /* as PHANT_SIG_BAD_V */
#define PHANT_TX_SIGNATURE 0x004u          /* the recovery failed; sig_status says how */
#define PHANT_TX_CHAIN_ID 0x008u           /* a typed transaction whose chain_id field is not the call's.  AN ADDITION: the reference never
                                            * checks it (signer.zig:149,176 sign with the transaction's own id) */
#define PHANT_TX_PRIORITY_ABOVE_MAX 0x010u /* InvalidMaxFeePerGas: type 2, max_fee_per_gas < max_priority_fee_per_gas */
#define PHANT_TX_FEE_BELOW_BASE 0x020u     /* MaxFeePerGasLowerThanBaseFee / GasPriceLowerThanBaseFee */
#define PHANT_TX_GAS_ABOVE_BLOCK 0x040u    /* gas_limit > block_gas_limit: the state-free part of InsufficientGas; the running
                                            * gas_available needs execution and stays with the caller */
#define PHANT_TX_INTRINSIC_GAS 0x080u      /* intrinsic_gas > gas_limit */
#define PHANT_TX_NONCE_MAX 0x100u          /* nonce == 2^64 - 1 (EIP-2681).  A DEVIATION: the reference's constant (2 << 64) - 1 at
                                            * blockchain.zig:348 can never trigger for a u64 */
#define PHANT_TX_INITCODE_SIZE 0x200u      /* a creation with more than 2 x 0x6000 bytes of data */
#define PHANT_TX_COST_OVERFLOW 0x400u      /* upfront_cost exceeds 2^256 - 1; its row is zero */
#define PHANT_TX_IS_CREATE 0x800u          /* no error: `to` is empty */
/* A bad transaction is a flag, never an error.  PHANT_E_INVALID_ARG: a wrong struct_size, NULL txs / tx_off with n > 0, offsets
 * that go backwards or do not run from 0 (device form: to tx_bytes), unknown flag bits, sender or sig_status together with
 * PHANT_TXS_NO_RECOVERY.  PHANT_E_UNSUPPORTED: a single transaction of 2^32 bytes or more.  n == 0 is PHANT_OK with first_bad =
 * 0.  The host form checks before anything is copied: one staged upload, the launches, one synchronisation.
 *
 * Device form: txs, tx_off and every output are device memory, the uint64_t arrays 8-byte, the uint32_t arrays 4-byte aligned,
 * byte arrays not at all; both structs and base_fee are host memory.  tx_off is checked on the device before any kernel
 * indexes with it.  The call synchronises the ctx stream (first_bad is valid when it returns). */
typedef struct phant_txs_in {
    uint32_t struct_size; /* = sizeof(phant_txs_in) */
    uint32_t n;
    uint32_t flags;       /* PHANT_TXS_* */
    uint32_t reserved;    /* 0 */
    const uint8_t *txs;
    const uint64_t *tx_off;  /* n + 1 */
    uint64_t tx_bytes;       /* device form: tx_off[n] as the caller states it */
    uint64_t chain_id;
    const uint8_t *base_fee; /* 32 bytes, host memory, or NULL */
    uint64_t block_gas_limit;
} phant_txs_in;
typedef struct phant_txs_out {
    uint32_t struct_size; /* = sizeof(phant_txs_out) */
    uint32_t first_bad;   /* result */
    uint8_t *tx_hash;
    uint8_t *sig_hash;
    uint8_t *sender;
    uint8_t *sig_status;
    uint8_t *sig;
    uint8_t *type;
    uint64_t *chain_id;
    uint64_t *nonce;
    uint64_t *gas_limit;
    uint8_t *gas_price;
    uint8_t *priority_fee;
    uint8_t *value;
    uint8_t *to;
    uint64_t *data_off;
    uint32_t *data_len;
    uint64_t *al_off;
    uint32_t *al_len;
    uint32_t *al_addresses;
    uint32_t *al_keys;
    uint64_t *intrinsic_gas;
    uint8_t *effective_gas_price;
    uint8_t *upfront_cost;
    uint32_t *flags;
} phant_txs_out;
PHANT_API int32_t phant_block_transactions(phant_ctx *ctx, const phant_txs_in *in, phant_txs_out *out);
PHANT_API int32_t phant_block_transactions_dev(phant_ctx *ctx, const phant_txs_in *in, phant_txs_out *out);

/* ------------------------------------------------- a block's transactions, the forks after London: blob (type 3) and set-code (type 4)
 * phant_block_transactions_ex is phant_block_transactions with a fork: which typed transactions decode, and which rules hold.
 *   PHANT_TXS_FORK_LONDON   types 0 - 2: answer for answer phant_block_transactions (which is this call with that fork)
 *   PHANT_TXS_FORK_CANCUN   + type 3 (EIP-4844)
 *   PHANT_TXS_FORK_PRAGUE   + type 4 (EIP-7702), + the EIP-7623 floor for every type
 * A type the fork does not enable is PHANT_TX_UNDECODABLE.  None of this is in the reference (its transaction.zig stops at
 * FeeMarketTx): the EIPs are the specification, written out here.  sender / sig_status equal phant_tx_senders' value for value
 * for types 0 - 2 only: that call (and the host decode behind it) does not know types 3 and 4.
 *
 * Type 3 = 0x03 || rlp([chain_id, nonce, max_priority_fee_per_gas, max_fee_per_gas, gas_limit, to, value, data, access_list,
 * max_fee_per_blob_gas, blob_versioned_hashes, y_parity, r, s]): 14 items, max_fee_per_blob_gas of at most 32 bytes, the hashes a
 * list of strings of exactly 32 bytes (anything else: undecodable).  Signing hash: keccak256(0x03 || rlp(the first 11 items)).
 * Type 4 = 0x04 || rlp([chain_id, nonce, max_priority_fee_per_gas, max_fee_per_gas, gas_limit, to, value, data, access_list,
 * authorization_list, y_parity, r, s]): 13 items, authorization_list = [[chain_id, address, nonce, y_parity, r, s], ...] with
 * chain_id <= 32 bytes, address exactly 20, nonce <= 8, y_parity <= 1, r and s <= 32, canonical integers, exactly six items in
 * a tuple and nothing else inside it; any violation makes the TRANSACTION undecodable.  Signing hash: keccak256(0x04 ||
 * rlp(the first 10 items)).  Both: the strictness of types 1 and 2; `to` empty or 20 bytes (empty: PHANT_TX_NO_TO and
 * PHANT_TX_IS_CREATE, not a decode failure); the fee rules, effective_gas_price and PHANT_TX_CHAIN_ID of type 2.
 *
 * Rules.  Type 4: intrinsic_gas gains 25000 per tuple.  Type 3: upfront_cost = gas_limit x max_fee_per_gas + value + blobs x
 * 131072 x max_fee_per_blob_gas; beyond 2^256 - 1: PHANT_TX_COST_OVERFLOW and a zero row, as for the other types.  PRAGUE, every
 * type: floor_gas = 21000 + 10 x (zero bytes + 4 x non-zero bytes of the calldata), PHANT_TX_FLOOR_GAS when gas_limit <
 * floor_gas (PHANT_TX_INTRINSIC_GAS is what it was).  blob_base_fee (32 bytes big-endian, HOST memory in both forms; NULL skips
 * the rule): PHANT_TX_BLOB_FEE_BELOW_BASE when a type-3 transaction's max_fee_per_blob_gas is below it; the caller computes it
 * from the parent header's excess_blob_gas (EIP-4844 fake_exponential).  blob_gas_used is a RESULT, which the caller compares with
 * the header's field and the fork's maximum.
 *
 * Authorization tuples: row j of the per-authorization outputs is tuple j - auth_first[i] of transaction i, auth_first (n + 1
 * entries) being the exclusive prefix sums of the tuples per decodable type-4 transaction.  auth_hash = keccak256(0x05 ||
 * rlp([chain_id, address, nonce])), auth_sig = r || s || y_parity as decoded; authority = the recovered signer (low s enforced:
 * PHANT_RECOVER_LOW_S), zero unless auth_status is PHANT_SIG_OK.  auth_status is, in this order: PHANT_AUTH_CHAIN_ID (the tuple's
 * chain id is neither 0 nor the call's), PHANT_AUTH_NONCE_MAX (its nonce is 2^64 - 1), PHANT_SIG_BAD_V (y_parity > 1) -- none of
 * which reaches the curve arithmetic -- or the recovery's PHANT_SIG_*.  A tuple whose status is not PHANT_SIG_OK is skipped by the
 * caller, as EIP-7702 says: it does NOT flag its transaction.  auth_cap = the rows the per-authorization arrays hold: n_auth and
 * auth_first are always complete, rows from auth_cap on are not written, and the call still returns PHANT_OK.  A tuple takes at
 * least 27 bytes (a list header of 1, then 1 + 21 + 1 + 1 + 1 + 1), so n_auth <= (bytes of the type-4 transactions) / 27.
 * PHANT_TXS_NO_RECOVERY also skips the authorities' recovery: authority and auth_status must then be NULL.
 *
 * Refusals as for phant_block_transactions (PHANT_E_INVALID_ARG, nothing touched), and: a wrong outer struct_size, fork >
 * PHANT_TXS_FORK_PRAGUE, reserved != 0.  Device form: as phant_block_transactions_dev; blob_off, floor_gas and auth_nonce 8-byte,
 * blobs and auth_first 4-byte aligned.  A PRAGUE call that may hold a tuple (device form: every one; host form: one with a
 * transaction that begins with 0x04) synchronises once more in its middle to learn how many there are. */
#define PHANT_TXS_FORK_LONDON 0u
#define PHANT_TXS_FORK_CANCUN 1u
#define PHANT_TXS_FORK_PRAGUE 2u
#define PHANT_AUTH_CHAIN_ID 8u  /* auth_status, beside PHANT_SIG_* */
#define PHANT_AUTH_NONCE_MAX 9u
#define PHANT_TX_NO_TO 0x01000u               /* type 3 or 4 with an empty `to` (PHANT_TX_IS_CREATE is set as well) */
#define PHANT_TX_BLOB_NONE 0x02000u           /* type 3 without a versioned hash */
#define PHANT_TX_BLOB_VERSION 0x04000u        /* some versioned hash's first byte is not 0x01 */
#define PHANT_TX_BLOB_FEE_BELOW_BASE 0x08000u /* type 3: max_fee_per_blob_gas < blob_base_fee */
#define PHANT_TX_AUTH_NONE 0x10000u           /* type 4 with an empty authorization list */
#define PHANT_TX_FLOOR_GAS 0x20000u           /* PRAGUE: gas_limit < floor_gas */
/* (0x40000 stays free: the blob term is part of upfront_cost, and PHANT_TX_COST_OVERFLOW covers it) */
#define PHANT_TX_ERROR_BITS_EX (0x7ffu | 0x7f000u) /* the error bits of the _ex call; first_bad counts these */
typedef struct phant_txs_ex_in {
    uint32_t struct_size; /* = sizeof(phant_txs_ex_in) */
    uint32_t fork;        /* PHANT_TXS_FORK_* */
    phant_txs_in base;    /* base.struct_size = sizeof(phant_txs_in) */
    const uint8_t *blob_base_fee; /* 32 bytes big-endian, host memory, or NULL */
    uint32_t auth_cap;    /* rows the per-authorization outputs hold */
    uint32_t reserved;    /* 0 */
} phant_txs_ex_in;
typedef struct phant_txs_ex_out {
    uint32_t struct_size;   /* = sizeof(phant_txs_ex_out) */
    uint32_t n_auth;        /* result: the authorization tuples of all decodable type-4 transactions */
    uint64_t blob_gas_used; /* result: 131072 x the versioned hashes of all decodable type-3 transactions */
    phant_txs_out base;     /* base.first_bad counts the new error bits too */
    /* per transaction, n rows; any may be NULL */
    uint8_t *max_fee_per_blob_gas; /* 32, zero unless type 3 */
    uint64_t *blob_off;            /* into txs: the first byte of the versioned-hash list's payload; 0 unless type 3 */
    uint32_t *blobs;               /* its hashes (33 RLP bytes each) */
    uint32_t *auth_first;          /* n + 1; auth_first[n] == n_auth */
    uint64_t *floor_gas;           /* EIP-7623; 0 below PRAGUE and for undecodable rows */
    /* per authorization, in (transaction, position) order, min(n_auth, auth_cap) rows written; any may be NULL */
    uint8_t *auth_chain_id; /* 32 big-endian */
    uint8_t *auth_address;  /* 20 */
    uint64_t *auth_nonce;
    uint8_t *auth_hash;     /* 32 */
    uint8_t *auth_sig;      /* 65: r || s || y_parity */
    uint8_t *authority;     /* 20, zero unless auth_status == PHANT_SIG_OK */
    uint8_t *auth_status;   /* PHANT_SIG_* or PHANT_AUTH_* */
} phant_txs_ex_out;
PHANT_API int32_t phant_block_transactions_ex(phant_ctx *ctx, const phant_txs_ex_in *in, phant_txs_ex_out *out);
PHANT_API int32_t phant_block_transactions_ex_dev(phant_ctx *ctx, const phant_txs_ex_in *in, phant_txs_ex_out *out);

/* ------------------------------------------------- chain segments of block bodies: many blocks' transactions in one call
 * What phant_block_transactions_ex and phant_block_roots answer block by block, for the bodies of n_blocks blocks in ONE call:
 * the headers of a segment go through phant_header_chain, the bodies they commit to through this.  A recovery launch lasts as
 * long as one lane's chain of multiplications whatever the number of signatures (up to about 65 000), so a segment's
 * signatures cost what one block's cost.
 *
 * Input.  fork (one PHANT_TXS_FORK_* per call: a caller splits a range at a fork boundary), chain_id, flags
 * (PHANT_TXS_HAVE_GAS_LIMIT, PHANT_TXS_NO_RECOVERY, as above).  n, txs, tx_off (n + 1), tx_bytes: as in phant_txs_in, all
 * blocks' transactions back to back.  block_first (n_blocks + 1): never backwards, from 0 to n; block b owns the transactions
 * [block_first[b], block_first[b + 1]); an empty block is ordinary.  n_wd, withdrawals, wd_off (n_wd + 1), wd_bytes, wd_first
 * (n_blocks + 1): each withdrawal is its RLP list exactly as it stands in the block, which is its trie value; wd_first ==
 * NULL: the segment has no withdrawal lists (before Shanghai) -- n_wd must then be 0 and withdrawals, wd_off and both
 * withdrawals_root pointers NULL.  Per block, laid out like the arrays of phant_headers_in, so that a caller can point at the
 * same memory: base_fee (n_blocks x 32 big-endian; NULL skips the two fee rules), gas_limit (n_blocks, read with
 * PHANT_TXS_HAVE_GAS_LIMIT), blob_base_fee (n_blocks x 32; NULL skips its rule; the caller derives block b's from its
 * parent's excess_blob_gas).  Expected values, each may be NULL: transactions_root, withdrawals_root (n_blocks x 32),
 * blob_gas_used (n_blocks).  UNLIKE phant_block_transactions_ex, whose base_fee and blob_base_fee are host memory in both
 * forms, every array here is host memory in the host form and DEVICE memory in the device form.  The host form does not read
 * tx_bytes and wd_bytes (the totals are tx_off[n] and wd_off[n_wd]).
 *
 * Output, any pointer may be NULL.  txs: every per-transaction and per-authorization row of phant_txs_ex_out over the n
 * transactions, auth_first (n + 1) global over the segment; its scalars keep their meaning over the whole segment
 * (base.first_bad: the least flagged i; n_auth; blob_gas_used: the total).  DEFINITION: the row of transaction i in block b
 * is exactly row i of phant_block_transactions_ex called over all n transactions with block b's base_fee, gas_limit and
 * blob_base_fee -- so data_off, al_off and blob_off are offsets into the segment's txs, and a zero row stays zero.
 *   tx_block (n)                 the block of transaction i
 *   block_first_bad (n_blocks)   the least i - block_first[b] whose flags carry an error bit, the block's count if none
 *   block_blob_gas_used (n_blocks, uint64_t)  131072 x the versioned hashes of the block's decodable type-3 transactions
 *   transactions_root, withdrawals_root (n_blocks x 32)  calculateMPTRoot (blockchain.zig:209-235: the key of item i is
 *                                rlp(i)) over the block's raw transactions / withdrawals; an empty list: empty_mpt_root
 *   block_flags (n_blocks)       below
 *   first_bad_block (always written)  the least b with block_flags[b] != 0, n_blocks if none
 * When neither root is asked for nor expected, no trie is built. */
#define PHANT_BODY_TX 1u       /* some transaction of the block carries a bit of PHANT_TX_ERROR_BITS_EX */
#define PHANT_BODY_TXS_ROOT 2u /* in->transactions_root given and != the computed root */
#define PHANT_BODY_WD_ROOT 4u  /* in->withdrawals_root given and != the computed root */
#define PHANT_BODY_BLOB_GAS 8u /* in->blob_gas_used given and != block_blob_gas_used */
/* A bad transaction or block is a flag, never an error.  PHANT_E_INVALID_ARG, before anything is indexed with the offending
 * value and with nothing written: a wrong struct_size (of either struct, of out->txs or of out->txs.base), fork >
 * PHANT_TXS_FORK_PRAGUE, an unknown flag bit, reserved != 0; a NULL input with a non-zero count (txs / tx_off with n,
 * block_first with n_blocks, withdrawals / wd_off with n_wd, gas_limit with PHANT_TXS_HAVE_GAS_LIMIT); tx_off, wd_off,
 * block_first or wd_first that do not run from 0 to their totals (device form: tx_bytes, wd_bytes; n; n_wd) or go backwards;
 * n_wd, withdrawals, wd_off or a withdrawals_root without wd_first; sender, sig_status, authority or auth_status together with
 * PHANT_TXS_NO_RECOVERY.  PHANT_E_UNSUPPORTED: a transaction or a withdrawal of 2^32 bytes or more, 2^32 bytes of trie
 * values or 2^31 - 1 items in one call.  n_blocks == 0 is PHANT_OK with first_bad_block = 0 and the scalars of txs zero; so
 * is n == 0 (the roots are then those of empty lists).  The host form checks on the host before any copy: one staged
 * upload, the launches, one copy back of the span up to the last wanted output.
 *
 * Device form: every array is device memory, the uint64_t arrays 8-byte and the uint32_t arrays 4-byte aligned, byte arrays
 * not at all; the structs are host memory.  The four offset arrays are checked by a kernel whose verdict the host reads
 * before any other kernel indexes with them.  The call synchronises the ctx stream (the scalars are valid when it returns). */
typedef struct phant_bodies_in {
    uint32_t struct_size; /* = sizeof(phant_bodies_in) */
    uint32_t fork;        /* PHANT_TXS_FORK_* */
    uint32_t flags;       /* PHANT_TXS_* */
    uint32_t n_blocks;
    uint32_t n;           /* transactions of all blocks */
    uint32_t n_wd;        /* withdrawals of all blocks */
    uint32_t auth_cap;    /* rows the per-authorization outputs hold */
    uint32_t reserved;    /* 0 */
    uint64_t chain_id;
    const uint8_t *txs;
    const uint64_t *tx_off;       /* n + 1 */
    uint64_t tx_bytes;            /* device form: tx_off[n] as the caller states it */
    const uint32_t *block_first;  /* n_blocks + 1 */
    const uint8_t *withdrawals;
    const uint64_t *wd_off;       /* n_wd + 1 */
    uint64_t wd_bytes;            /* device form: wd_off[n_wd] as the caller states it */
    const uint32_t *wd_first;     /* n_blocks + 1, or NULL */
    const uint8_t *base_fee;      /* n_blocks x 32, or NULL */
    const uint64_t *gas_limit;    /* n_blocks */
    const uint8_t *blob_base_fee; /* n_blocks x 32, or NULL */
    const uint8_t *transactions_root; /* expected, n_blocks x 32, or NULL */
    const uint8_t *withdrawals_root;  /* expected, n_blocks x 32, or NULL */
    const uint64_t *blob_gas_used;    /* expected, n_blocks, or NULL */
} phant_bodies_in;
typedef struct phant_bodies_out {
    uint32_t struct_size;     /* = sizeof(phant_bodies_out) */
    uint32_t first_bad_block; /* result */
    phant_txs_ex_out txs;     /* txs.struct_size = sizeof(phant_txs_ex_out), txs.base.struct_size = sizeof(phant_txs_out) */
    uint32_t *tx_block;
    uint32_t *block_first_bad;
    uint64_t *block_blob_gas_used;
    uint8_t *transactions_root;
    uint8_t *withdrawals_root;
    uint32_t *block_flags;
} phant_bodies_out;
PHANT_API int32_t phant_block_bodies(phant_ctx *ctx, const phant_bodies_in *in, phant_bodies_out *out);
PHANT_API int32_t phant_block_bodies_dev(phant_ctx *ctx, const phant_bodies_in *in, phant_bodies_out *out);
/* Host only, strict: the packed arrays phant_block_bodies takes from n raw blocks.  Block b = blob[off[b] .. off[b+1]) =
 * [header, transactions, uncles, withdrawals?], or with PHANT_BODIES_NO_HEADER an eth-style body [transactions, uncles,
 * withdrawals?].  Canonical RLP throughout and nothing behind the item; the header, when there, is a list and is not looked
 * into (phant_headers_decode_rlp does that).  A transaction item is a list (a legacy transaction: its whole encoding is the
 * value) or a non-empty string whose first byte is at most 0x7f (a typed one: its payload is the value); a withdrawal is a
 * list, its whole encoding the value; uncles must be the empty list (`runBlock`: NotEmptyUncles).  status[b] (n bytes) says
 * which rule block b broke first, and such a block contributes no rows: block_first[b + 1] == block_first[b], likewise
 * wd_first.  A block without a withdrawals list has none; whether it should have one is its header's business.
 * Sizing in two steps: n, n_wd, tx_bytes and wd_bytes are always written; when one of them exceeds its capacity (tx_cap,
 * wd_cap: items; tx_bytes_cap, wd_bytes_cap: bytes; a NULL array has capacity 0) NOTHING else is written, status included, and
 * the call still returns PHANT_OK: call again with arrays of the reported sizes (tx_off tx_cap + 1, block_first and wd_first
 * n + 1, wd_off wd_cap + 1 entries).  PHANT_E_INVALID_ARG: NULL blob / off / split / status with n > 0, a wrong struct_size,
 * unknown flags, offsets that go backwards. */
#define PHANT_BODIES_NO_HEADER 1u
#define PHANT_SPLIT_OK 0
#define PHANT_SPLIT_BAD_RLP 1        /* not a canonical list of 3 or 4 (2 or 3) lists with nothing behind it */
#define PHANT_SPLIT_BAD_TX 2         /* a transaction item that is neither a list nor a string beginning with a type byte */
#define PHANT_SPLIT_UNCLES 3         /* the uncles are not the empty list */
#define PHANT_SPLIT_BAD_WITHDRAWAL 4 /* a withdrawal that is not a list */
typedef struct phant_bodies_split {
    uint32_t struct_size; /* = sizeof(phant_bodies_split) */
    uint32_t reserved;    /* 0 */
    uint32_t tx_cap, wd_cap;
    uint64_t tx_bytes_cap, wd_bytes_cap;
    uint8_t *txs;
    uint64_t *tx_off;
    uint32_t *block_first;
    uint8_t *withdrawals;
    uint64_t *wd_off;
    uint32_t *wd_first;
    uint32_t n, n_wd;           /* results */
    uint64_t tx_bytes, wd_bytes; /* results */
} phant_bodies_split;
PHANT_API int32_t phant_bodies_decode_rlp(const uint8_t *blob, const uint64_t *off, uint32_t n, uint32_t flags,
                                          phant_bodies_split *split, uint8_t *status);

/* ------------------------------------------------- receipts of a chain segment from raw messages: decode, blooms, roots
 * What phant_block_receipts answers for one block from the FIELDS an EVM has just produced, for the receipts of n_blocks blocks as a
 * peer sends them -- raw RLP -- in ONE call: the headers of a segment go through phant_header_chain, its bodies through
 * phant_block_bodies, the receipts they commit to through this.  The reference never compares receipts with a header
 * (src/blockchain/blockchain.zig:184-191 builds receipts without logs, :86-88 leaves the bloom as a TODO); this is a part the drop-in adds.
 *
 * Input.  n, receipts, rc_off (n + 1), rc_bytes: the receipt values of all blocks back to back; block_first (n_blocks + 1): never
 * backwards, from 0 to n; an empty block is ordinary.  form says what one value is:
 *   PHANT_RCPTS_CONSENSUS  [type byte 0x01 .. 0x7f, when typed] ++ rlp([status_or_root, cum_gas, bloom(256), logs]) -- what eth/68 and
 *                          earlier carry and what the receipts trie holds; the trie value is the bytes as given
 *   PHANT_RCPTS_ETH69      rlp([tx_type, status_or_root, cum_gas, logs]) (EIP-7642), tx_type a canonical integer 0 .. 0x7f; the trie
 *                          value is BUILT: [tx_type, when != 0] ++ rlp_list(status item ++ gas item ++ 0xb9 0x01 0x00 ++ computed
 *                          bloom ++ logs item), the three items copied as they stand
 * A row is decodable when it is canonical RLP throughout with nothing behind the item, has exactly the form's items, status_or_root is
 * the empty string, 0x01 or a 32-byte string (a pre-Byzantium post-state root), cum_gas a canonical integer of at most 8 bytes, the
 * bloom a string of exactly 256 bytes, and logs a list of [address(20), [topic(32) ...], data] of exactly three items each.  In the
 * consensus form a leading 0x00 is undecodable.  A length field may state up to 2^64 - 1 anywhere: nothing outside
 * [rc_off[i], rc_off[i + 1]) is ever read.  Expected values, one row per block, each may be NULL: receipts_root (32 bytes),
 * logs_bloom (256), gas_used (uint64_t), tx_count (uint32_t).  The host form does not read rc_bytes (the total is rc_off[n]).
 *
 * Output, any pointer may be NULL.  Per receipt (n rows): tx_type; status (0, 1, or 2 for a post-state root); cum_gas; gas_used =
 * cum_gas minus the predecessor's in the same block modulo 2^64, the block's first against 0; log_first (n + 1); bloom (n x 256,
 * computed from the logs); flags (below).  An undecodable row has zero fields, no logs and a zero bloom, and its trie value is its raw
 * bytes in BOTH forms: the root of its block is then defined and wrong, and the block is flagged anyway.
 * Per log (n_logs rows, from all decodable receipts in order): log_receipt; address (20 bytes); topic_first (n_logs + 1); topics
 * (n_topics x 32); data_at (an offset into `receipts`), data_len.  n_logs and n_topics are always written; when one exceeds its cap
 * (log_cap, topic_cap: the rows the per-log outputs hold) no per-log array is touched and the call still returns PHANT_OK.
 * encoded, encoded_off (n + 1): the consensus encodings in index order -- what an ETH69 caller stores; a copy of the input in the
 * consensus form.  encoded_len is always written; when it exceeds encoded_cap neither buffer is touched and the call still returns
 * PHANT_OK (a NULL `encoded` has no capacity to exceed).
 * Per block: receipts_root (calculateMPTRoot over the values, key rlp(index); an empty block: empty_mpt_root); logs_bloom (the OR of the
 * block's computed blooms); block_gas_used (the last decodable row's cum_gas, 0 without one); block_first_bad (the least i -
 * block_first[b] whose flags carry an error bit, the block's count if none); block_flags (below); first_bad_block (always written: the
 * least b with block_flags[b] != 0, n_blocks if none).  No trie is built when no root is wanted or expected.  No Keccak runs over the
 * logs when nothing needs a bloom: the consensus form needs one for PHANT_RCPT_BLOOM, the ETH69 form for a root, the encodings, the
 * bloom outputs and an expected logs_bloom. */
#define PHANT_RCPTS_CONSENSUS 0u
#define PHANT_RCPTS_ETH69 1u
#define PHANT_RCPT_UNDECODABLE 1u     /* the row is not a receipt of the call's form */
#define PHANT_RCPT_BLOOM 2u           /* consensus form: the embedded bloom is not the logs' bloom */
#define PHANT_RCPT_GAS_ORDER 4u       /* this row and its predecessor in the block are decodable and cum_gas is not greater than the
                                         predecessor's; the block's first row: its cum_gas is 0 */
#define PHANT_RCPT_POST_STATE 0x100u  /* informative: status_or_root is a 32-byte post-state root */
#define PHANT_RCPT_ERROR_BITS 7u
#define PHANT_RBLOCK_RECEIPT 1u   /* some row of the block carries a bit of PHANT_RCPT_ERROR_BITS */
#define PHANT_RBLOCK_ROOT 2u      /* in->receipts_root given and != the computed root */
#define PHANT_RBLOCK_BLOOM 4u     /* in->logs_bloom given and != the block's computed bloom */
#define PHANT_RBLOCK_GAS_USED 8u  /* in->gas_used given and != block_gas_used */
#define PHANT_RBLOCK_COUNT 16u    /* in->tx_count given and != the block's receipts */
/* A bad receipt or block is a flag, never an error.  PHANT_E_INVALID_ARG, before anything is indexed with the offending value and with
 * nothing written: a wrong struct_size, an unknown form, reserved != 0, a NULL input with a non-zero count (receipts / rc_off with n,
 * block_first with n_blocks), receipts without a block, rc_off or block_first that do not run from 0 to their totals (device form:
 * rc_bytes; n) or go backwards.  PHANT_E_UNSUPPORTED: a receipt of 2^32 bytes or more, 2^32 bytes of receipts or of trie values (an
 * ETH69 receipt counted with the 268 bytes it can grow by) or 2^31 - 1 items in one call.  n_blocks == 0 is PHANT_OK with
 * first_bad_block, n_logs, n_topics and encoded_len 0; so is n == 0.  The host form checks on the host before any copy: one staged
 * upload, the launches, one copy back of the span up to the last wanted output (plain copies beyond the pinned stage).
 *
 * Device form: every array is device memory, the uint64_t arrays 8-byte and the uint32_t arrays 4-byte aligned, byte arrays not at all;
 * the structs are host memory.  rc_off and block_first are checked by a kernel whose verdict the host reads before any other kernel
 * indexes with them.  The call synchronises the ctx stream (the scalars are valid when it returns); the copies of the per-log rows and
 * of the encodings are in stream order behind it. */
typedef struct phant_rcpt_segs_in {
    uint32_t struct_size; /* = sizeof(phant_rcpt_segs_in) */
    uint32_t form;        /* PHANT_RCPTS_* */
    uint32_t n_blocks;
    uint32_t n;           /* receipts of all blocks */
    uint32_t log_cap;     /* rows the per-log outputs hold */
    uint32_t topic_cap;   /* rows `topics` holds */
    uint32_t reserved[2]; /* 0 */
    const uint8_t *receipts;
    const uint64_t *rc_off;      /* n + 1 */
    uint64_t rc_bytes;           /* device form: rc_off[n] as the caller states it */
    const uint32_t *block_first; /* n_blocks + 1 */
    const uint8_t *receipts_root; /* expected, n_blocks x 32, or NULL */
    const uint8_t *logs_bloom;    /* expected, n_blocks x 256, or NULL */
    const uint64_t *gas_used;     /* expected, n_blocks, or NULL */
    const uint32_t *tx_count;     /* expected, n_blocks, or NULL */
} phant_rcpt_segs_in;
typedef struct phant_rcpt_segs_out {
    uint32_t struct_size;     /* = sizeof(phant_rcpt_segs_out) */
    uint32_t first_bad_block; /* result */
    uint32_t n_logs;          /* result */
    uint32_t n_topics;        /* result */
    uint64_t encoded_cap;     /* bytes of encoded */
    uint64_t encoded_len;     /* result */
    uint8_t *tx_type;
    uint8_t *status;
    uint64_t *cum_gas;
    uint64_t *gas_used;
    uint32_t *log_first;
    uint8_t *bloom;
    uint32_t *flags;
    uint32_t *log_receipt;
    uint8_t *address;
    uint32_t *topic_first;
    uint8_t *topics;
    uint64_t *data_at;
    uint32_t *data_len;
    uint8_t *encoded;
    uint64_t *encoded_off;
    uint8_t *receipts_root;
    uint8_t *logs_bloom;
    uint64_t *block_gas_used;
    uint32_t *block_first_bad;
    uint32_t *block_flags;
} phant_rcpt_segs_out;
PHANT_API int32_t phant_block_receipt_segments(phant_ctx *ctx, const phant_rcpt_segs_in *in, phant_rcpt_segs_out *out);
PHANT_API int32_t phant_block_receipt_segments_dev(phant_ctx *ctx, const phant_rcpt_segs_in *in, phant_rcpt_segs_out *out);
/* Host only, strict: the packed arrays phant_block_receipt_segments takes from the n per-block elements of a `Receipts` message.
 * Block b = blob[off[b] .. off[b+1]) = the list of its receipts, canonical RLP with nothing behind it.  Without
 * PHANT_RCPTS_SPLIT_ETH69 an item is a list (a legacy receipt: its whole encoding is the value) or a non-empty string whose first byte
 * is at most 0x7f (a typed one: its payload is the value); with it every item is a list, its whole encoding the value.  The splitter
 * does not look into receipts.  status[b] (n bytes) says which rule block b broke first, and such a block contributes no rows:
 * block_first[b + 1] == block_first[b].  Sizing in two steps: n and rc_bytes are always written; when one exceeds its capacity (rc_cap:
 * items; rc_bytes_cap: bytes; a NULL array has capacity 0) NOTHING else is written, status included, and the call still returns
 * PHANT_OK: call again with arrays of the reported sizes (rc_off rc_cap + 1, block_first n + 1 entries).  PHANT_E_INVALID_ARG: NULL
 * blob / off / split / status with n > 0, a wrong struct_size, unknown flags, offsets that go backwards. */
#define PHANT_RCPTS_SPLIT_ETH69 1u
#define PHANT_SPLIT_BAD_RECEIPT 5 /* an item that is neither a list nor a string beginning with a type byte (ETH69: not a list) */
typedef struct phant_receipts_split {
    uint32_t struct_size; /* = sizeof(phant_receipts_split) */
    uint32_t reserved;    /* 0 */
    uint32_t rc_cap;
    uint32_t n;           /* result */
    uint64_t rc_bytes_cap;
    uint8_t *receipts;
    uint64_t *rc_off;
    uint32_t *block_first;
    uint64_t rc_bytes;    /* result */
} phant_receipts_split;
PHANT_API int32_t phant_receipts_decode_rlp(const uint8_t *blob, const uint64_t *off, uint32_t n, uint32_t flags,
                                            phant_receipts_split *split, uint8_t *status);

/* ------------------------------------------------- execution requests of a chain segment: deposits, requests hash (EIP-7685, EIP-6110)
 * Since Prague a header's 21st field, requests_hash, commits to the block's execution requests.  phant_header_chain hashes it into the
 * block hash; this call computes it for every block of a segment and holds it against the header's.  The deposit requests (type 0) are
 * not in a block body: they are rebuilt from the logs phant_block_receipt_segments leaves decoded.  The requests the EVM's system calls
 * produce (types 1 and 2 today) come from the caller.  tests/requests_ref.py is the same definition in Python with hashlib.sha256.
 *
 * Input.  The log rows exactly as phant_block_receipt_segments answers them: receipts with rc_bytes, block_first (n_blocks + 1, in
 * receipts), log_first (n + 1), address (n_logs x 20), topic_first (n_logs + 1), topics (n_topics x 32), data_at and data_len (n_logs;
 * data_at an offset into `receipts`, of any alignment) -- in the device form the device arrays of that call, handed on without a copy.
 * deposit_contract: the 20 bytes the caller's chain configuration names (the library has no chain table).  The caller's requests, n_req
 * rows: req_block_first (n_blocks + 1, in rows), req_type (n_req bytes), req_bytes with req_off (n_req + 1); n_req == 0 with NULL arrays
 * is legal.  active (n_blocks bytes, or NULL for all): a zero byte marks a block before the fork -- it has no deposit rows, a zero
 * requests_hash and no flags, and neither its logs nor its rows are looked at.  requests_hash: the expected values, n_blocks x 32, or NULL.
 *
 * A log is a deposit CANDIDATE when its block is active, its address equals deposit_contract over all 20 bytes, it has at least one
 * topic and its first topic is 649bbc62d0e31342afea4e5cd82d4049e7e1ee912fc0889aa790803be39038c5 =
 * keccak256("DepositEvent(bytes,bytes,bytes,bytes,bytes)"); other logs of the contract are ignored (EIP-6110).  A candidate is
 * WELL-FORMED when data_len == 576, [data_at, data_at + 576) lies inside [0, rc_bytes) -- nothing outside is ever read --, the five
 * 32-byte big-endian words at 0, 32, 64, 96, 128 of its data are exactly 160, 256, 320, 384, 512 and the words at 160, 256, 320, 384, 512
 * are exactly 48, 32, 8, 96, 8 (all 32 bytes of each word are compared).  A well-formed candidate's request row is the 192 bytes
 * data[192:240] ++ data[288:320] ++ data[352:360] ++ data[416:512] ++ data[544:552]: pubkey, withdrawal credentials, amount, signature
 * and index as they stand.  A candidate that is not well-formed yields no row and sets PHANT_QBLOCK_DEPOSIT_LAYOUT on its block (EIP-6110
 * makes such a block invalid).
 * A block's requests: type 0 = the block's rows in log order, present when there is at least one; then the caller's rows of the block
 * in the order given, a row without data left out.  h_t = sha256(type ++ data) for each present request; requests_hash = sha256(h_0 ++
 * h_1 ++ ...); a block with nothing: sha256("") = e3b0c442 98fc1c14 9afbf4c8 996fb924 27ae41e4 649b934c a495991b 7852b855.
 * Within a block the caller's types must be 1 .. 255 and strictly ascending, rows without data included: otherwise PHANT_QBLOCK_ORDER,
 * and the hash is still the one of the rows as given.
 *
 * Output, any pointer may be NULL.  n_deposits and first_bad_block (the least b with block_flags[b] != 0, n_blocks if none) are always
 * written.  Per deposit, at most deposit_cap rows: deposit_log (the log's index), deposit (192 bytes).  Per block: deposit_first
 * (n_blocks + 1), requests_hash, block_flags.  When n_deposits > deposit_cap no per-deposit array is touched and the call still
 * returns PHANT_OK with hashes and flags complete (the rows the hashes read live in the call's arena).
 *
 * A bad block is a flag, never an error.  PHANT_E_INVALID_ARG, with nothing written: a wrong struct_size, reserved != 0, a NULL input
 * with a non-zero count (block_first with n_blocks; log_first with n; address, topic_first, data_at, data_len with n_logs; topics with
 * n_topics; receipts with rc_bytes; req_block_first, req_type, req_off with n_req; req_bytes with bytes), rows without a block, logs
 * without a receipt, topics without a log, or block_first, log_first, topic_first, req_block_first or req_off that do not run from 0 to
 * their totals (n, n_logs, n_topics, n_req; device form: req_total) or go backwards.  n_blocks == 0 is PHANT_OK with both scalars 0.
 * The host form checks on the host before any copy and does not read req_total (the total is req_off[n_req]).  Device form: every array
 * is device memory, the uint64_t arrays 8-byte and the uint32_t arrays 4-byte aligned, byte arrays not at all; the structs are host
 * memory; the firsts and offsets are checked by a kernel whose verdict the host reads before any other kernel indexes with them.  The
 * call synchronises the ctx stream (the scalars are valid when it returns); the copies of the per-deposit rows are in stream order behind
 * it.  The launches depend on neither n_blocks nor n_logs; a call takes as long as its longest message: three compressions per deposit,
 * serial in the one lane that hashes a block's type-0 request. */
#define PHANT_QBLOCK_DEPOSIT_LAYOUT 1u /* a deposit candidate of the block is not well-formed */
#define PHANT_QBLOCK_ORDER 2u          /* a caller's row of type 0, or types not strictly ascending */
#define PHANT_QBLOCK_HASH 4u           /* in->requests_hash given and != the computed hash */
typedef struct phant_requests_in {
    uint32_t struct_size; /* = sizeof(phant_requests_in) */
    uint32_t n_blocks;
    uint32_t n;           /* receipts of all blocks */
    uint32_t n_logs;
    uint32_t n_topics;
    uint32_t n_req;       /* the caller's rows of all blocks */
    uint32_t deposit_cap; /* rows the per-deposit outputs hold */
    uint32_t reserved;    /* 0 */
    const uint8_t *receipts;
    uint64_t rc_bytes;
    const uint32_t *block_first;     /* n_blocks + 1 */
    const uint32_t *log_first;       /* n + 1 */
    const uint8_t *address;          /* n_logs x 20 */
    const uint32_t *topic_first;     /* n_logs + 1 */
    const uint8_t *topics;           /* n_topics x 32 */
    const uint64_t *data_at;         /* n_logs */
    const uint32_t *data_len;        /* n_logs */
    const uint32_t *req_block_first; /* n_blocks + 1 */
    const uint8_t *req_type;         /* n_req */
    const uint8_t *req_bytes;
    const uint64_t *req_off;         /* n_req + 1 */
    uint64_t req_total;              /* device form: req_off[n_req] as the caller states it */
    const uint8_t *active;           /* n_blocks, or NULL: every block */
    const uint8_t *requests_hash;    /* expected, n_blocks x 32, or NULL */
    uint8_t deposit_contract[20];
} phant_requests_in;
typedef struct phant_requests_out {
    uint32_t struct_size;     /* = sizeof(phant_requests_out) */
    uint32_t n_deposits;      /* result */
    uint32_t first_bad_block; /* result */
    uint32_t reserved;        /* 0 */
    uint32_t *deposit_log;
    uint8_t *deposit;
    uint32_t *deposit_first;
    uint8_t *requests_hash;
    uint32_t *block_flags;
} phant_requests_out;
PHANT_API int32_t phant_block_requests(phant_ctx *ctx, const phant_requests_in *in, phant_requests_out *out);
PHANT_API int32_t phant_block_requests_dev(phant_ctx *ctx, const phant_requests_in *in, phant_requests_out *out);

/* ------------------------------------------------- log filters over a chain segment: exact matches and bloom screening
 * Which logs does a filter select -- the question of eth_getLogs and eth_subscribe("logs").  phant_block_log_filters answers it exactly
 * over the log rows phant_block_receipt_segments leaves decoded, for many filters in one call; phant_log_filters_bloom answers "which
 * blocks can hold a match" from nothing but 2048-bit blooms (headers' logs_bloom, or receipts'), so that a node that holds only headers
 * knows which receipts to fetch.  tests/filters_ref.py is the same definition in Python.
 *
 * The filters, n_filters of them (phant_log_filters): addr_first (n_filters + 1) indexes addr (n_addr x 20 bytes): filter f's address
 * set is addr[addr_first[f] .. addr_first[f + 1]).  topic_first (4 n_filters + 1) indexes topic (n_topic x 32 bytes): set (f, p), the
 * values topic position p may take, is entry 4 f + p, p = 0 .. 3.  block_lo, block_hi (n_filters each): the blocks [lo, hi) of the
 * segment the filter looks at; either may be NULL: 0 and n_blocks (n_blooms for the bloom call).  An empty set is a wildcard;
 * duplicates inside a set are legal and mean nothing.
 * Log l of block b MATCHES filter f when block_lo[f] <= b < block_hi[f], the address set is empty or address[l] equals one of its
 * entries over all 20 bytes, and for every p with a non-empty set the log has more than p topics and its topic p equals an entry of
 * set (f, p) over all 32 bytes.  An address never matches a topic entry, a topic at one position never the set of another.
 *
 * phant_block_log_filters.  Input: the log rows as phant_block_receipt_segments answers them -- block_first (n_blocks + 1, in
 * receipts), log_first (n + 1), address (n_logs x 20), topic_first (n_logs + 1), topics (n_topics x 32); in the device form its device
 * arrays, handed on without a copy; the logs' data is no input.  Output, any pointer may be NULL: n_matches is always written;
 * filter_first (n_filters + 1) and filter_count (n_filters); match_log, at most match_cap rows: the logs' indices, ordered by filter
 * and then by log -- each filter's logs in chain order.  When n_matches > match_cap match_log is not touched and the call still returns
 * PHANT_OK with the counts complete.  A set of at most PHANT_LOGFILTER_LINEAR_MAX (include/phant_gpu_diag.h) entries is compared entry
 * by entry, a larger one looked up in one keyed open-addressing table built over all such sets of the call; the launches depend on
 * neither n_filters nor n_logs (but on whether there is such a set).  n_filters x ceil(n_logs / 64) >= 2^31: PHANT_E_UNSUPPORTED.
 *
 * phant_log_filters_bloom.  Input: blooms, n_blooms x 256 bytes; block_lo and block_hi index blooms.  Output, either may be NULL: may,
 * n_filters x ceil(n_blooms / 64) words: bit b % 64 of word f * ceil(n_blooms / 64) + b / 64 is set when bloom b can hold a match of
 * f; the padding bits are zero; may_count (n_filters): the set bits of each filter.  Bloom b CAN HOLD a match of f when b is in range,
 * the address set is empty or all three bits of one of its entries are set in the bloom, and the same for every non-empty topic set.
 * An entry's bits are Ethereum's: the low 11 bits of each of the big-endian 16-bit words at bytes 0, 2 and 4 of its Keccak-256; value v
 * is bit 7 - (2047 - v) % 8 of byte (2047 - v) / 8.  No false negatives: a block that holds an exact match is set.  The blooms cross
 * the device's memory once whatever n_filters is.  n_filters x ceil(n_blooms / 64) >= 2^31: PHANT_E_UNSUPPORTED.
 *
 * PHANT_E_INVALID_ARG, with nothing written: a wrong struct_size, reserved != 0, a NULL input with a non-zero count, rows without a
 * block, logs without a receipt, topics without a log, entries without a filter, 2^30 or more filters, firsts (the rows' and the filters') that do not run from 0 to their totals or
 * go backwards, block_lo[f] > block_hi[f], block_hi[f] > n_blocks (n_blooms).  n_filters == 0 is PHANT_OK: n_matches = 0 and no array
 * is written; n_logs == 0 and n_blooms == 0 are PHANT_OK with zero counts.  Device form: every array is device memory, the uint64_t
 * arrays 8-byte and the uint32_t arrays 4-byte aligned, byte arrays not at all; the structs are host memory; firsts and ranges are
 * checked by a kernel whose verdict the host reads before any other kernel indexes with them.  The calls synchronise the ctx stream;
 * the copy of match_log is in stream order behind it. */
typedef struct phant_log_filters {
    uint32_t struct_size; /* = sizeof(phant_log_filters) */
    uint32_t n_filters;
    uint32_t n_addr;
    uint32_t n_topic;
    const uint32_t *addr_first;  /* n_filters + 1 */
    const uint8_t *addr;         /* n_addr x 20 */
    const uint32_t *topic_first; /* 4 n_filters + 1 */
    const uint8_t *topic;        /* n_topic x 32 */
    const uint32_t *block_lo;    /* n_filters, or NULL: 0 */
    const uint32_t *block_hi;    /* n_filters, or NULL: n_blocks / n_blooms */
    uint64_t reserved;           /* 0 */
} phant_log_filters;
typedef struct phant_logmatch_in {
    uint32_t struct_size; /* = sizeof(phant_logmatch_in) */
    uint32_t n_blocks;
    uint32_t n; /* receipts of all blocks */
    uint32_t n_logs;
    uint32_t n_topics;
    uint32_t match_cap; /* rows match_log holds */
    uint32_t reserved;  /* 0 */
    uint32_t reserved2; /* 0 */
    const uint32_t *block_first; /* n_blocks + 1 */
    const uint32_t *log_first;   /* n + 1 */
    const uint8_t *address;      /* n_logs x 20 */
    const uint32_t *topic_first; /* n_logs + 1 */
    const uint8_t *topics;       /* n_topics x 32 */
} phant_logmatch_in;
typedef struct phant_logmatch_out {
    uint32_t struct_size; /* = sizeof(phant_logmatch_out) */
    uint32_t n_matches;   /* result */
    uint32_t reserved;    /* 0 */
    uint32_t reserved2;   /* 0 */
    uint32_t *filter_first; /* n_filters + 1 */
    uint32_t *match_log;    /* match_cap */
    uint32_t *filter_count; /* n_filters */
} phant_logmatch_out;
PHANT_API int32_t phant_block_log_filters(phant_ctx *ctx, const phant_logmatch_in *in, const phant_log_filters *filters, phant_logmatch_out *out);
PHANT_API int32_t phant_block_log_filters_dev(phant_ctx *ctx, const phant_logmatch_in *in, const phant_log_filters *filters, phant_logmatch_out *out);
PHANT_API int32_t phant_log_filters_bloom(phant_ctx *ctx, const uint8_t *blooms, uint32_t n_blooms, const phant_log_filters *filters,
                                          uint64_t *may, uint32_t *may_count);
PHANT_API int32_t phant_log_filters_bloom_dev(phant_ctx *ctx, const uint8_t *d_blooms, uint32_t n_blooms, const phant_log_filters *filters,
                                              uint64_t *d_may, uint32_t *d_may_count);

/* ------------------------------------------------- fee history over a chain segment: reward percentiles
 * The priority fee at chosen percentiles of each block's gas used -- the `reward` of eth_feeHistory.  phant_block_fee_history joins
 * the rows two segment calls leave behind: every transaction's effective_gas_price (phant_block_bodies) and every receipt's gas_used
 * (phant_block_receipt_segments).  tests/feehist_ref.py is the same definition in Python integers.
 *
 * A segment has n_blocks blocks; block_first (n_blocks + 1) gives block b the rows [block_first[b], block_first[b + 1]) of all n row
 * arrays.  Transaction i of a block is also receipt i of that block: the caller asserts this (phant_amd/types/block.py's
 * validate_receipts checks the counts).  Input: price (n x 32, big-endian: effective_gas_price as phant_block_bodies answers it;
 * before London, the gas price), base_fee (n_blocks x 32, big-endian, laid out like phant_bodies_in.base_fee; NULL means zero),
 * gas_used (n, as phant_block_receipt_segments answers it), percentile (n_percentiles, HOST memory in both forms): basis points, each
 * at most 10000, in any order, repeats allowed.
 *
 *   tip[i] = price[i] - base_fee[block of i]; where price[i] < base_fee: tip[i] = 0 and the block gets PHANT_FEE_BELOW_BASE -- a flag,
 *     never an error.
 *   Within a block the rows are ordered by (tip, row index) ascending -- a stable sort; order[block_first[b] + r] is the GLOBAL row
 *     with rank r in block b.
 *   S_r = the sum of gas_used over the ranks 0 .. r of the block, exact (96 bits, as phant_block_settle's cum); G = S_last is the
 *     block's gas.
 *   reward[b][k] = the tip of the row at the least rank r with S_r >= threshold, threshold = floor(G x percentile[k] / 10000).  Such
 *     an r always exists.  This is geth's loop: start at rank 0 and advance while the sum is below the threshold and a row is left.
 *     THE THRESHOLD IS TAKEN IN INTEGERS, not in float64 as geth takes it (uint64(float64(gasUsed) * p / 100)): no answer depends on
 *     how a product rounds.  No division is made: S_r >= floor(G p / 10000) holds exactly when 10000 (S_r + 1) > G p, in 128 bits.
 *     An empty block has all rewards zero and flags 0.
 *
 * Output, every pointer may be NULL: reward (n_blocks x n_percentiles x 32, big-endian), tip (n x 32, big-endian), order (n),
 * block_gas_used (n_blocks: G clamped to 2^64 - 1), block_flags (n_blocks); first_bad_block is always written: the least flagged block,
 * or n_blocks if none.
 *
 * PHANT_E_INVALID_ARG, with nothing written and before anything is indexed with the offending value: a wrong struct_size, reserved != 0,
 * a NULL input with a non-zero count, rows without a block, a percentile above 10000, block_first that does not run from 0 to n or goes
 * backwards.  PHANT_E_UNSUPPORTED: a block of more than PHANT_FEEHIST_BLOCK_MAX rows (the ranking is quadratic in a block's rows; the cap
 * keeps a hostile block_first from buying seconds of device time -- at 21000 gas a row it is 1.4 G gas, beyond any chain);
 * n_blocks x n_percentiles >= 2^31.  PHANT_OK: n_blocks == 0 (first_bad_block = 0); n_percentiles == 0 (tip, order and the per-block
 * outputs are still written); n == 0.
 *
 * Device form: every array but percentile is device memory, handed on without a copy; the uint64_t arrays are 8-byte, the uint32_t
 * arrays 4-byte aligned, byte arrays not at all; both structs are host memory.  block_first and the cap are checked by a kernel whose
 * verdict the host reads before any other kernel indexes with them.  The call synchronises the ctx stream.  The launches depend on
 * neither n_blocks, n nor n_percentiles. */
#define PHANT_FEE_BELOW_BASE 0x1u      /* block_flags: a row's price is below the block's base fee (its tip counts as 0) */
#define PHANT_FEEHIST_BLOCK_MAX 65536u /* the most rows a block may have */
typedef struct phant_fee_history_in {
    uint32_t struct_size; /* = sizeof(phant_fee_history_in) */
    uint32_t n_blocks;
    uint32_t n; /* rows (transactions = receipts) of all blocks */
    uint32_t n_percentiles;
    const uint32_t *block_first; /* n_blocks + 1 */
    const uint8_t *price;        /* n x 32, big-endian */
    const uint8_t *base_fee;     /* n_blocks x 32, big-endian, or NULL: zero */
    const uint64_t *gas_used;    /* n */
    const uint32_t *percentile;  /* n_percentiles basis points, HOST memory in both forms */
    uint64_t reserved;           /* 0 */
} phant_fee_history_in;
typedef struct phant_fee_history_out {
    uint32_t struct_size;     /* = sizeof(phant_fee_history_out) */
    uint32_t first_bad_block; /* result */
    uint8_t *reward;          /* n_blocks x n_percentiles x 32, big-endian */
    uint8_t *tip;             /* n x 32, big-endian */
    uint32_t *order;          /* n */
    uint64_t *block_gas_used; /* n_blocks */
    uint32_t *block_flags;    /* n_blocks */
    uint64_t reserved;        /* 0 */
} phant_fee_history_out;
PHANT_API int32_t phant_block_fee_history(phant_ctx *ctx, const phant_fee_history_in *in, phant_fee_history_out *out);
PHANT_API int32_t phant_block_fee_history_dev(phant_ctx *ctx, const phant_fee_history_in *in, phant_fee_history_out *out);

/* ------------------------------------------------- a block's transactions against the pre-state: nonces, EOA and witness rows
 * phant_block_txs_prestate joins the rows phant_block_transactions[_ex] answers (keyed by transaction) with the rows
 * phant_exec_witness_prestate answers (keyed by witness row), and decides what `processTransaction` checks first
 * (src/blockchain/blockchain.zig:270-276: InvalidTxNonce, NotEnoughBalance, SenderIsNotEOA) as far as it can be decided for the whole
 * block before any transaction runs.  tests/txstate_ref.py is the same definition in Python integers.
 *
 * row_of(a) = the LOWEST j with addresses[j] == a over all 20 bytes, else PHANT_ROW_NONE.  A row j is PROVEN when account_status[j] is
 * PHANT_PROOF_PRESENT or PHANT_PROOF_ABSENT (the empty account, by phant_exec_witness_prestate's contract); the account arrays are read
 * as they are.
 *
 * Transaction i PARTICIPATES when sig_status[i] == PHANT_SIG_OK and tx_flags[i] has none of PHANT_TX_UNDECODABLE, PHANT_TX_BAD_V,
 * PHANT_TX_SIGNATURE.  Any other row has no sender: sender_row = to_row = PHANT_ROW_NONE, expected_nonce = 0, spent_before = 0,
 * state_flags = PHANT_TXST_SKIPPED, which is no error bit here (the transactions call has reported the row).  A participating row:
 *   sender_row = s = row_of(sender).  s is NONE or not proven: PHANT_TXST_SENDER_UNKNOWN; the row joins no sequence, expected_nonce and
 *     spent_before are 0 and no further sender rule is evaluated (the block cannot be executed from this witness).
 *   Otherwise the row joins the SEQUENCE of s: the participating rows with that sender row, in block order.  rank = the rows of the
 *     sequence before i.  expected_nonce = nonces[s] + rank, saturating at 2^64 - 1: a sender's nonce moves by exactly one for each of
 *     its transactions, whatever the EVM does with them, and every verdict assumes that every earlier row was included.
 *     spent_before = the sum of upfront_cost over the rows of the sequence before i, a row with PHANT_TX_COST_OVERFLOW counting as 2^256;
 *     written clamped to 2^256 - 1, with PHANT_TXST_SPENT_SATURATED when it was clamped.
 *   UNDETERMINED rows, fork >= PHANT_TXS_FORK_PRAGUE only: (1) the sender's code is a delegation designator -- code_hashes[s] is not
 *     the empty code hash, code_index[s] names a code of exactly 23 bytes, and that code begins ef 01 00 --, or (2) the sender is the
 *     `authority` of a tuple with auth_status == PHANT_SIG_OK in a participating transaction j < i (not j == i).  Delegated code may
 *     CREATE and a set-code tuple may bump the nonce: the row gets PHANT_TXST_UNDETERMINED, is counted in n_undetermined, the nonce, EOA
 *     and balance rules are NOT evaluated for it -- deciding it needs the full EIP-7702 tuple processing and stays with the CALLER --,
 *     and expected_nonce and spent_before are still written.
 *   A determined row: PHANT_TXST_NONCE_LOW when nonce[i] < expected_nonce, PHANT_TXST_NONCE_HIGH when nonce[i] > expected_nonce (A
 *     DEVIATION: the two split the reference's one InvalidTxNonce).  EIP-3607: a code hash that is not the empty one is
 *     PHANT_TXST_NOT_EOA below PRAGUE; from PRAGUE on PHANT_TXST_CODE_MISSING when code_index[s] == PHANT_CODE_NONE (nobody can tell
 *     statelessly whether it is a designator), else PHANT_TXST_NOT_EOA (A DEVIATION: the designator exemption is newer than the
 *     reference's SenderIsNotEOA).  PHANT_TXST_NEEDS_INFLOW (advisory): balances[s] < spent_before + the row's own cost, in full
 *     width; when the bit is clear the reference's balance check for this row cannot fail, because an undelegated EOA loses at most
 *     its upfront costs.  PHANT_TXST_BALANCE_SHORT: NEEDS_INFLOW and i == 0 (nothing ran before the block's first transaction).
 *   Recipient, unless PHANT_TX_IS_CREATE (then to_row = NONE): to_row = row_of(to); PHANT_TXST_TO_UNKNOWN when that is NONE or not proven.
 * Tuple k belongs to transaction j when auth_first[j] <= k < auth_first[j + 1]; auth_first NULL: the call has no tuples.
 * Per account: sends[j] = the length of row j's sequence; roles[j] = who named the row (PHANT_ROLE_*: the sender or recipient of a
 * participating transaction, the authority of a PHANT_SIG_OK tuple of one, a probe).  Per probe (any further address the caller wants
 * located: coinbase, withdrawal recipients, access-list and delegation targets): probe_row = row_of(probe).  (The targets of the
 * block's access lists need no probes: phant_block_access_lists, below, decodes the lists and joins them itself.)
 * first_bad (always written): the least i whose state_flags carry an error bit, n if none (0 for n == 0); n_undetermined.
 *
 * Any output pointer may be NULL.  PHANT_E_INVALID_ARG, before anything is indexed with the offending value: a wrong struct_size, an
 * unknown fork, reserved != 0, a NULL input whose count is not zero (auth_first may be NULL, code_off may not when n_codes > 0), auth_first
 * not non-decreasing within [0, n_auth], code_off not non-decreasing within [0, code_bytes], a code_index that is neither < n_codes
 * nor PHANT_CODE_NONE.  Nothing outside the stated extents is read; of `codes` only the first three bytes of the codes of 23 bytes.
 * Host form: checked on the host before anything is copied; one staged upload, the launches, one copy back of the wanted outputs,
 * one synchronisation.  Device form: every array is device memory (uint64_t arrays 8-byte, uint32_t arrays 4-byte aligned), both
 * structs host memory; the offsets and indices are checked by a kernel whose verdict the host reads before any other kernel uses
 * them; the call synchronises the ctx stream. */
#define PHANT_ROW_NONE 0xffffffffu
#define PHANT_TXST_SENDER_UNKNOWN 0x001u  /* the witness lacks the sender, or its row is not proven */
#define PHANT_TXST_TO_UNKNOWN 0x002u      /* ... the recipient */
#define PHANT_TXST_NONCE_LOW 0x004u       /* InvalidTxNonce: nonce < expected_nonce */
#define PHANT_TXST_NONCE_HIGH 0x008u      /* InvalidTxNonce: nonce > expected_nonce */
#define PHANT_TXST_BALANCE_SHORT 0x010u   /* NotEnoughBalance, certain: the block's first transaction */
#define PHANT_TXST_NOT_EOA 0x020u         /* SenderIsNotEOA (EIP-3607) */
#define PHANT_TXST_CODE_MISSING 0x040u    /* PRAGUE: the sender has code the witness does not carry */
#define PHANT_TXST_ERROR_BITS 0x07fu      /* first_bad counts these */
#define PHANT_TXST_SKIPPED 0x100u         /* no error: the row does not participate */
#define PHANT_TXST_UNDETERMINED 0x200u    /* advisory: the sender rules were not evaluated */
#define PHANT_TXST_NEEDS_INFLOW 0x400u    /* advisory: the balance does not cover spent_before + the row's cost */
#define PHANT_TXST_SPENT_SATURATED 0x800u /* advisory: spent_before was clamped to 2^256 - 1 */
#define PHANT_ROLE_SENDER 1u
#define PHANT_ROLE_RECIPIENT 2u
#define PHANT_ROLE_AUTHORITY 4u
#define PHANT_ROLE_PROBE 8u
typedef struct phant_txstate_in {
    uint32_t struct_size; /* = sizeof(phant_txstate_in) */
    uint32_t fork;        /* PHANT_TXS_FORK_* */
    uint32_t n;           /* transaction rows */
    uint32_t n_auth;      /* authorization rows */
    uint32_t n_accounts;  /* pre-state rows */
    uint32_t n_codes;
    uint32_t n_probe;
    uint32_t reserved;    /* 0 */
    /* per transaction, straight from phant_txs_out / phant_txs_ex_out */
    const uint8_t *sender;       /* n x 20 */
    const uint8_t *sig_status;   /* n */
    const uint32_t *tx_flags;    /* n: phant_txs_out.flags */
    const uint64_t *nonce;       /* n */
    const uint8_t *upfront_cost; /* n x 32 */
    const uint8_t *to;           /* n x 20 */
    const uint32_t *auth_first;  /* n + 1, or NULL */
    const uint8_t *authority;    /* n_auth x 20 */
    const uint8_t *auth_status;  /* n_auth */
    /* per pre-state row, straight from phant_exec_witness_info / phant_prestate */
    const uint8_t *addresses;      /* n_accounts x 20 */
    const uint8_t *account_status; /* n_accounts */
    const uint64_t *nonces;        /* n_accounts */
    const uint8_t *balances;       /* n_accounts x 32 */
    const uint8_t *code_hashes;    /* n_accounts x 32 */
    const uint32_t *code_index;    /* n_accounts */
    const uint64_t *code_off;      /* n_codes + 1 */
    const uint8_t *codes;
    uint64_t code_bytes;
    const uint8_t *probe;          /* n_probe x 20 */
} phant_txstate_in;
typedef struct phant_txstate_out {
    uint32_t struct_size;    /* = sizeof(phant_txstate_out) */
    uint32_t first_bad;      /* result */
    uint32_t n_undetermined; /* result */
    uint32_t reserved;
    /* per transaction */
    uint32_t *sender_row;
    uint32_t *to_row;
    uint64_t *expected_nonce;
    uint8_t *spent_before;   /* 32 big-endian */
    uint32_t *state_flags;   /* PHANT_TXST_* */
    /* per pre-state row */
    uint32_t *sends;
    uint8_t *roles;          /* PHANT_ROLE_* */
    /* per probe */
    uint32_t *probe_row;
} phant_txstate_out;
PHANT_API int32_t phant_block_txs_prestate(phant_ctx *ctx, const phant_txstate_in *in, phant_txstate_out *out);
PHANT_API int32_t phant_block_txs_prestate_dev(phant_ctx *ctx, const phant_txstate_in *in, phant_txstate_out *out);

/* ------------------------------------------------- a block of plain transfers settled: balances, gas, account writes
 * phant_block_settle takes the rows phant_block_transactions[_ex] and phant_block_txs_prestate answer, the pre-state rows of the
 * witness and the block's withdrawals, and does what `applyBody` (src/blockchain/blockchain.zig:155-205) and `processTransaction`
 * (:262-343) do for the transactions that meet no code: the gas each uses, the running gas_available, the sender's exact balance
 * before each, and per pre-state row exactly the account_op / nonces / balances / code_hashes phant_exec_witness_poststate reads.
 * tests/settle_ref.py is the same definition in Python integers.
 *
 * A row j is PROVEN as above.  coinbase_row and wd_row[j] are probe_row entries of the pre-state call (the coinbase and the
 * withdrawal addresses passed as probes), or PHANT_ROW_NONE.
 *
 * The CLASS of transaction i follows from the row's own inputs alone, never from a running value:
 *   UPSTREAM (PHANT_SETTLE_UPSTREAM, an error bit): tx_flags[i] has an error bit of the transactions call (every PHANT_TX_* bit but
 *     PHANT_TX_IS_CREATE), state_flags[i] has PHANT_TXST_SKIPPED or one of PHANT_TXST_ERROR_BITS, or effective_gas_price < base_fee.
 *     Also -- which cannot happen behind calls that raised none of those bits -- sender_row is NONE, to_row is NONE without
 *     PHANT_TX_IS_CREATE, or gas_used x effective_gas_price + value exceeds 2^256 - 1 (it is at most upfront_cost).
 *   NOT_PLAIN (PHANT_SETTLE_NOT_PLAIN, advisory; counted in n_not_plain, the least index in first_not_plain, n if none): otherwise, when
 *     type is 3 or 4, PHANT_TX_IS_CREATE, PHANT_TXST_UNDETERMINED, code_hashes[to_row] is not the empty code hash, or `to` is a
 *     precompile of the fork: its first 19 bytes are zero and the last is in 1..0x09 (LONDON), 1..0x0a (CANCUN), 1..0x11 (PRAGUE).
 *     These rows need the EVM and stay with the CALLER.
 *   PLAIN otherwise.
 * UPSTREAM and NOT_PLAIN rows contribute no event and no gas; settle_flags holds the class bit, cumulative_gas_used and
 * balance_before are 0.
 *
 * A plain row i: gas_used_i = max(intrinsic_gas, floor_gas) (floor_gas NULL: 0); cum_before_i = the sum of gas_used over the plain
 * rows before i.  PHANT_SETTLE_GAS_LIMIT (error) when gas_limit_i + cum_before_i > block_gas_limit, in full width (the reference's
 * gas_available check).  cumulative_gas_used[i] = cum_before_i + gas_used_i, clamped to 2^64 - 1.  Its EVENTS (row, time, value):
 *   (sender_row, 2i, -(gas_used_i x effective_gas_price_i + value_i)),  (to_row, 2i + 1, +value_i),
 *   (coinbase_row, 2i + 1, +gas_used_i x (effective_gas_price_i - base_fee)) when coinbase_row is proven.
 * Withdrawal j is the event (wd_row[j], 2n + j, +wd_amount_gwei[j] x 10^9) when wd_row[j] is proven; otherwise it is dropped,
 * wd_flags[j] = PHANT_SETTLE_WD_UNKNOWN and n_wd_unknown counts it.  block_flags has PHANT_SETTLE_COINBASE_UNKNOWN when there is a
 * plain row and coinbase_row is NONE or not proven.
 * balance_before[i] = balances[sender_row] plus every event on that row with time < 2i: exact and signed, written clamped to
 * [0, 2^256 - 1].  PHANT_SETTLE_BALANCE_SHORT (error) when the unclamped value is below upfront_cost_i: the reference's
 * NotEnoughBalance (blockchain.zig:273) -- the exact check phant_block_txs_prestate leaves open behind PHANT_TXST_NEEDS_INFLOW.
 * Self-transfers, a sender that is the coinbase and a withdrawal to a sender need no rule of their own: the times order them.
 * EVERY VERDICT ASSUMES THAT EVERY EARLIER PLAIN ROW WAS APPLIED, flagged or not: only the verdicts up to first_bad carry consensus
 * meaning (a block with first_bad < n is invalid whatever comes behind), as the nonces of phant_block_txs_prestate do.
 *
 * Per pre-state row.  A row is TOUCHED when it is the sender or recipient of a plain row, the proven coinbase while a plain row
 * exists, or the target of a withdrawal that was not dropped.  Untouched: account_op = PHANT_POST_KEEP, nonces_after, balances_after
 * the pre-state's.  Touched: nonces_after = nonces + its plain sends, saturating at 2^64 - 1; balances_after = the balance plus all
 * its events -- above 2^256 - 1: clamped, with PHANT_SETTLE_ACCT_OVERFLOW in account_flags; negative (possible only behind a
 * BALANCE_SHORT row): 0, with PHANT_SETTLE_ACCT_NEGATIVE.  EIP-161, as processTransaction's last loop and the Shanghai withdrawal
 * rule apply it: a touched row with nonces_after == 0, balances_after == 0 and the empty code hash is PHANT_POST_DELETE when
 * account_status is PRESENT and PHANT_POST_KEEP when it is ABSENT; every other touched row is PHANT_POST_SET.  Evaluating this once
 * at the end of the block equals evaluating it after every transaction: a codeless account that never sends (nonce 0) only ever
 * GAINS balance here, so if it is empty at the end it was empty at every touch, and if it is not, nothing was deleted in between
 * that the end would not show.  code_hashes_after is always the pre-state's (no plain row changes code).
 *
 * Scalars (always written): first_bad = the least i with an error bit, n if none; n_not_plain; first_not_plain; block_flags;
 * n_wd_unknown; gas_used = the block's, clamped to 2^64 - 1.  The block is SETTLED when first_bad == n, n_not_plain == 0,
 * block_flags == 0, n_wd_unknown == 0 and no account_flags bit is set: the outputs then are what the reference's loop leaves.
 *
 * Any output pointer may be NULL.  PHANT_E_INVALID_ARG, before anything is indexed with the offending value: a wrong struct_size, an
 * unknown fork, reserved != 0, a NULL input whose count is not zero (floor_gas may be NULL), a sender_row, to_row, wd_row or
 * coinbase_row that is neither < n_accounts nor PHANT_ROW_NONE.  PHANT_E_UNSUPPORTED: 3 n + n_wd or n_accounts beyond 2^31 - 1.
 * Host form: checked on the host before anything is copied; one staged upload, the launches, one copy back of the wanted outputs, one
 * synchronisation.  Device form: every array is device memory (uint64_t arrays 8-byte, uint32_t arrays 4-byte aligned), both structs
 * host memory; the row indices are checked by a kernel whose verdict the host reads before any other kernel uses them; the call
 * synchronises the ctx stream. */
#define PHANT_SETTLE_UPSTREAM 0x001u      /* an earlier call flagged the row, or its price is below the base fee */
#define PHANT_SETTLE_GAS_LIMIT 0x002u     /* the block's gas does not cover gas_limit behind the rows before */
#define PHANT_SETTLE_BALANCE_SHORT 0x004u /* NotEnoughBalance, exact */
#define PHANT_SETTLE_ERROR_BITS 0x007u    /* first_bad counts these */
#define PHANT_SETTLE_NOT_PLAIN 0x100u     /* advisory: the row needs the EVM */
#define PHANT_SETTLE_COINBASE_UNKNOWN 1u  /* block_flags */
#define PHANT_SETTLE_WD_UNKNOWN 1u        /* wd_flags[j] */
#define PHANT_SETTLE_ACCT_OVERFLOW 1u     /* account_flags[j] */
#define PHANT_SETTLE_ACCT_NEGATIVE 2u
typedef struct phant_settle_in {
    uint32_t struct_size;  /* = sizeof(phant_settle_in) */
    uint32_t fork;         /* PHANT_TXS_FORK_* */
    uint32_t n;            /* transaction rows */
    uint32_t n_accounts;   /* pre-state rows */
    uint32_t n_wd;         /* withdrawals */
    uint32_t coinbase_row; /* or PHANT_ROW_NONE */
    uint32_t reserved[2];  /* 0 */
    uint64_t block_gas_limit;
    const uint8_t *base_fee; /* 32 big-endian */
    /* per transaction, straight from phant_txs_out / phant_txs_ex_out / phant_txstate_out */
    const uint8_t *type;                /* n */
    const uint32_t *tx_flags;           /* n: phant_txs_out.flags */
    const uint64_t *gas_limit;          /* n */
    const uint64_t *intrinsic_gas;      /* n */
    const uint64_t *floor_gas;          /* n, or NULL */
    const uint8_t *value;               /* n x 32 */
    const uint8_t *effective_gas_price; /* n x 32 */
    const uint8_t *upfront_cost;        /* n x 32 */
    const uint8_t *to;                  /* n x 20 */
    const uint32_t *sender_row;         /* n */
    const uint32_t *to_row;             /* n */
    const uint32_t *state_flags;        /* n */
    /* per pre-state row, straight from phant_prestate */
    const uint8_t *account_status; /* n_accounts */
    const uint64_t *nonces;        /* n_accounts */
    const uint8_t *balances;       /* n_accounts x 32 */
    const uint8_t *code_hashes;    /* n_accounts x 32 */
    /* per withdrawal */
    const uint32_t *wd_row;         /* n_wd */
    const uint64_t *wd_amount_gwei; /* n_wd */
} phant_settle_in;
typedef struct phant_settle_out {
    uint32_t struct_size;     /* = sizeof(phant_settle_out) */
    uint32_t first_bad;       /* results ... */
    uint32_t n_not_plain;
    uint32_t first_not_plain;
    uint32_t block_flags;     /* PHANT_SETTLE_COINBASE_UNKNOWN */
    uint32_t n_wd_unknown;
    uint64_t gas_used;
    /* per transaction */
    uint32_t *settle_flags;        /* PHANT_SETTLE_* */
    uint64_t *cumulative_gas_used;
    uint8_t *balance_before;       /* 32 big-endian */
    /* per pre-state row: what phant_poststate reads */
    uint8_t *account_op;           /* PHANT_POST_* */
    uint64_t *nonces_after;
    uint8_t *balances_after;       /* 32 big-endian */
    uint8_t *code_hashes_after;    /* 32 */
    uint8_t *account_flags;        /* PHANT_SETTLE_ACCT_* */
    /* per withdrawal */
    uint8_t *wd_flags;             /* PHANT_SETTLE_WD_UNKNOWN */
} phant_settle_out;
PHANT_API int32_t phant_block_settle(phant_ctx *ctx, const phant_settle_in *in, phant_settle_out *out);
PHANT_API int32_t phant_block_settle_dev(phant_ctx *ctx, const phant_settle_in *in, phant_settle_out *out);

/* ------------------------------------------------- a block's access lists: entries, warm sets and their witness rows
 * phant_block_access_lists decodes the access lists (EIP-2930, transaction types 1 - 4) of a block's transactions and joins every
 * entry with the pre-state rows of the witness: what `processTransaction` turns into state before the EVM runs
 * (src/blockchain/blockchain.zig:284-295: putAccessedAccount, putAccessedStorageKeys) and what the EVM host's getStorage needs for
 * every warm slot.  tests/access_ref.py is the same definition in plain Python.
 *
 * Transaction i's list is the payload txs[al_off[i], al_off[i] + al_len[i]): al_off / al_len straight from phant_txs_out; al_len == 0
 * is an empty list (a legacy transaction, an undecodable row, an empty list).  The call does not trust the counts of the transactions
 * call: it walks every span itself, by the rules phant_block_transactions applies -- [[address20, [key32, ...]], ...], canonical RLP,
 * nothing else inside a tuple --, and reads nothing outside the span.  A span that is not such a payload gets PHANT_AL_MALFORMED and
 * contributes NO tuple (tuple_first[i + 1] == tuple_first[i], warm_addresses = warm_keys = 0); it is a flag, never an error.
 *
 * A TUPLE is one [address, [keys ...]] item.  Tuples are numbered through the block in order (tuple_first[i] = the first of
 * transaction i), keys likewise (key_first[e] = the first of tuple e).  With row_of as phant_block_txs_prestate defines it:
 *   account_row[e] = row_of(address[e]): the LOWEST row with that address over all 20 bytes, else PHANT_ROW_NONE
 *   tuple_same[e]  = the least tuple e' of the SAME transaction with address[e'] == address[e] (e itself: a first occurrence)
 *   slot_row[k]    = with r = the account_row of k's tuple: the least s in [slot_first[r], slot_first[r + 1]) with slots[s] == key[k]
 *                    over all 32 bytes; PHANT_ROW_NONE when r is NONE or there is none (a slot of ANOTHER row with that address or
 *                    that key does not count)
 *   key_same[k]    = the least key k' of the same transaction with key[k'] == key[k] under an equal address, across tuples as well
 *   warm_addresses[i], warm_keys[i] = the first occurrences among i's tuples / keys: the sizes of the sets putAccessed* builds
 *   PHANT_AL_DUPLICATES (advisory) = some tuple or key of the row is not a first occurrence
 * n_tuples, n_keys: the totals over well-formed rows; n_missing_accounts, n_missing_slots (advisory: a block need not touch what its
 * lists name): the FIRST occurrences whose account_row / slot_row is PHANT_ROW_NONE; first_malformed: the least flagged i, n if none.
 * These five are always written.  n_accounts == 0: nothing is joined, every row is NONE, slot_first / slots / n_slots are not looked at.
 *
 * Any output pointer may be NULL.  tuple_cap / key_cap: the rows the per-tuple / per-key buffers hold (key_first: tuple_cap + 1
 * entries); a buffer nobody wants has no capacity to exceed.  If n_tuples > tuple_cap or n_keys > key_cap the call still returns
 * PHANT_OK with the totals, the per-transaction outputs written, and touches NONE of the per-tuple and per-key buffers: call again.
 * PHANT_E_INVALID_ARG, before anything is indexed with the offending value: a wrong struct_size, reserved != 0, a NULL input whose
 * count is not zero, a span that leaves [0, tx_bytes), slot_first that does not run from 0 to n_slots without going backwards.
 * PHANT_E_UNSUPPORTED: the spans together hold 2^31 bytes or more (fewer than 2^27 tuples and 2^26 keys fit below that), or
 * n_accounts or n_slots is above 2^30 -- the tables index with 32 bits and stay at most half full.  n == 0: PHANT_OK, zero totals.
 * Host form: checked on the host before anything is copied; only the bytes of the spans cross the bus, in one staged upload with the
 * tables; the launches; one copy back of the span that ends at the last wanted output; one synchronisation.  Device form: every array
 * is device memory (al_off 8-byte, uint32_t arrays 4-byte aligned), both structs host memory; the spans and slot_first are checked by
 * a kernel whose verdict the host reads before any other kernel uses them; the call synchronises the ctx stream. */
#define PHANT_AL_MALFORMED 0x1u  /* the span is no well-formed access-list payload; the row contributes nothing */
#define PHANT_AL_DUPLICATES 0x2u /* advisory: an address or an (address, key) pair repeats in the row */
typedef struct phant_access_in {
    uint32_t struct_size; /* = sizeof(phant_access_in) */
    uint32_t n;           /* transaction rows */
    uint32_t n_accounts;  /* pre-state rows */
    uint32_t n_slots;
    /* per transaction, straight from phant_txs_in / phant_txs_out */
    const uint8_t *txs;
    uint64_t tx_bytes;
    const uint64_t *al_off; /* n */
    const uint32_t *al_len; /* n */
    /* the pre-state tables, straight from phant_exec_witness_info */
    const uint8_t *addresses;   /* n_accounts x 20 */
    const uint32_t *slot_first; /* n_accounts + 1 */
    const uint8_t *slots;       /* n_slots x 32 */
    uint32_t reserved[2];       /* 0 */
} phant_access_in;
typedef struct phant_access_out {
    uint32_t struct_size;        /* = sizeof(phant_access_out) */
    uint32_t n_tuples;           /* result */
    uint32_t n_keys;             /* result */
    uint32_t n_missing_accounts; /* result */
    uint32_t n_missing_slots;    /* result */
    uint32_t first_malformed;    /* result */
    uint32_t tuple_cap;          /* in: rows of the per-tuple buffers */
    uint32_t key_cap;            /* in: rows of the per-key buffers */
    /* per transaction */
    uint32_t *tuple_first;    /* n + 1 */
    uint32_t *al_flags;       /* PHANT_AL_* */
    uint32_t *warm_addresses;
    uint32_t *warm_keys;
    /* per tuple */
    uint8_t *address;         /* 20 */
    uint32_t *key_first;      /* n_tuples + 1 */
    uint32_t *account_row;
    uint32_t *tuple_same;
    /* per key */
    uint8_t *key;             /* 32 */
    uint32_t *slot_row;
    uint32_t *key_same;
} phant_access_out;
PHANT_API int32_t phant_block_access_lists(phant_ctx *ctx, const phant_access_in *in, phant_access_out *out);
PHANT_API int32_t phant_block_access_lists_dev(phant_ctx *ctx, const phant_access_in *in, phant_access_out *out);

/* ------------------------------------------------------- proof verification
 * ABSENT in the reference: this is the call the TODO at
 * src/engine_api/execution_payload.zig:177-178 asks for (witness field
 * commented out at :121).  Semantics: DESIGN.md section 3, the inverse of the
 * node encodings of src/mpt/mpt.zig:187-193,216-231,254-261,285-314.
 *
 *   roots            n_roots x 32 bytes
 *   root_idx         n entries (which root proof i is against) or NULL = all 0
 *   keys             n x key_len bytes (key_len = 32 for state/storage tries)
 *   nodes            all proof nodes back to back, nodes_len bytes
 *   node_off         total_nodes + 1 byte offsets into `nodes`; in the host form
 *                    total_nodes = proof_first_node[n] (its last entry)
 *   proof_first_node n + 1 entries: proof i = nodes
 *                    [proof_first_node[i], proof_first_node[i+1]), root first.
 *                    A range that goes backwards or beyond total_nodes, a node
 *                    offset pair that goes backwards or beyond nodes_len, or a
 *                    root_idx >= n_roots gives that proof PHANT_PROOF_BAD_INPUT;
 *                    nothing outside the buffers is read whatever these arrays
 *                    (an untrusted witness) say
 *   status           n bytes out (PHANT_PROOF_*)
 *   value_off/len    n entries out, or NULL: for PRESENT, where in `nodes`
 *                    the value bytes sit
 * The device form also takes total_nodes (= entries of node_off minus one).
 */
PHANT_API int32_t phant_mpt_verify_batch(phant_ctx *ctx, const uint8_t *roots, uint32_t n_roots,
                                         const uint32_t *root_idx, const uint8_t *keys,
                                         uint32_t key_len, const uint8_t *nodes,
                                         uint64_t nodes_len, const uint64_t *node_off,
                                         const uint32_t *proof_first_node, uint32_t n,
                                         uint8_t *status, uint64_t *value_off,
                                         uint32_t *value_len);
PHANT_API int32_t phant_mpt_verify_batch_dev(phant_ctx *ctx, const uint8_t *d_roots,
                                             uint32_t n_roots, const uint32_t *d_root_idx,
                                             const uint8_t *d_keys, uint32_t key_len,
                                             const uint8_t *d_nodes, uint64_t nodes_len,
                                             const uint64_t *d_node_off, uint32_t total_nodes,
                                             const uint32_t *d_proof_first_node, uint32_t n,
                                             uint8_t *d_status, uint64_t *d_value_off,
                                             uint32_t *d_value_len);
/* phant_mpt_verify_batch_dev + phant_mpt_verdict_dev in one launch sequence: the pipeline's last kernel,
 * through which every status passes anyway, also counts the failures per root (d_fail_count: n_roots x
 * u32, overwritten).  Saves the extra memset + kernel of the separate verdict call. */
PHANT_API int32_t phant_mpt_verify_verdict_dev(phant_ctx *ctx, const uint8_t *d_roots,
                                               uint32_t n_roots, const uint32_t *d_root_idx,
                                               const uint8_t *d_keys, uint32_t key_len,
                                               const uint8_t *d_nodes, uint64_t nodes_len,
                                               const uint64_t *d_node_off, uint32_t total_nodes,
                                               const uint32_t *d_proof_first_node, uint32_t n,
                                               uint8_t *d_status, uint64_t *d_value_off,
                                               uint32_t *d_value_len, uint32_t *d_fail_count);
/* One verdict per root: d_fail_count[r] = number of proofs against root r
 * whose status is not PRESENT/ABSENT (n_roots x u32, overwritten).  This is
 * the word each rank all-reduces in the multi-GPU path.  A proof whose root
 * index is out of range (its status is BAD_INPUT) is counted against root 0,
 * so that an all-zero verdict always means "every proof passed". */
PHANT_API int32_t phant_mpt_verdict_dev(phant_ctx *ctx, const uint8_t *d_status,
                                        const uint32_t *d_root_idx, uint32_t n, uint32_t n_roots,
                                        uint32_t *d_fail_count);

/* -------------------------------------------------------------- node-set witnesses
 * The same verification for a witness that ships every trie node ONCE, in any order (SURVEY.md section
 * 8f row 3, "dedup'd node-set verification"): `nodes` / `node_off` hold a SET of total_nodes nodes, there
 * is no proof_first_node; every key is walked from its root and the node a 32-byte reference points to is
 * the node of the set with that Keccak-256 digest.  Statuses as above, except that a reference nothing in
 * the set hashes to gives MISSING_NODE, and BAD_HASH / EXTRA_NODES / INVALID_EMPTY cannot occur. */
PHANT_API int32_t phant_mpt_verify_nodeset(phant_ctx *ctx, const uint8_t *roots, uint32_t n_roots,
                                           const uint32_t *root_idx, const uint8_t *keys,
                                           uint32_t key_len, const uint8_t *nodes, uint64_t nodes_len,
                                           const uint64_t *node_off, uint32_t total_nodes, uint32_t n,
                                           uint8_t *status, uint64_t *value_off, uint32_t *value_len);
PHANT_API int32_t phant_mpt_verify_nodeset_dev(phant_ctx *ctx, const uint8_t *d_roots, uint32_t n_roots,
                                               const uint32_t *d_root_idx, const uint8_t *d_keys,
                                               uint32_t key_len, const uint8_t *d_nodes,
                                               uint64_t nodes_len, const uint64_t *d_node_off,
                                               uint32_t total_nodes, uint32_t n, uint8_t *d_status,
                                               uint64_t *d_value_off, uint32_t *d_value_len);
/* ... with the per-root verdict of phant_mpt_verify_verdict_dev from the same launch: d_fail_count[r] (n_roots x u32,
 * overwritten) = keys against root r whose status is not PRESENT / ABSENT; a key whose root index is out of range
 * counts against root 0. */
PHANT_API int32_t phant_mpt_verify_nodeset_verdict_dev(phant_ctx *ctx, const uint8_t *d_roots, uint32_t n_roots,
                                                       const uint32_t *d_root_idx, const uint8_t *d_keys,
                                                       uint32_t key_len, const uint8_t *d_nodes,
                                                       uint64_t nodes_len, const uint64_t *d_node_off,
                                                       uint32_t total_nodes, uint32_t n, uint8_t *d_status,
                                                       uint64_t *d_value_off, uint32_t *d_value_len,
                                                       uint32_t *d_fail_count);

/* ------------------------------------------------------------------ streaming
 * BASELINE config 5 (consecutive block witnesses, H2D overlapped with verification): up to
 * PHANT_MAX_SLOTS host-form verifications in flight on one ctx, each on its own stream with its own
 * staging and workspace.  phant_mpt_verify_submit queues copy-in, kernels and copy-out and returns;
 * every buffer of the call (inputs AND status / value outputs) stays borrowed until phant_wait(slot)
 * returns.  Copies only overlap with other slots' kernels when the buffers are pinned: allocate them with
 * phant_host_alloc (hipHostMalloc) or register them; pageable memory works but serialises.
 * The async pair SURVEY.md section 8(b) lists for this path. */
#define PHANT_MAX_SLOTS 4
PHANT_API int32_t phant_host_alloc(phant_ctx *ctx, size_t bytes, void **out);
PHANT_API int32_t phant_host_free(phant_ctx *ctx, void *p);
PHANT_API int32_t phant_mpt_verify_submit(phant_ctx *ctx, uint32_t slot, const uint8_t *roots,
                                          uint32_t n_roots, const uint32_t *root_idx,
                                          const uint8_t *keys, uint32_t key_len, const uint8_t *nodes,
                                          uint64_t nodes_len, const uint64_t *node_off,
                                          const uint32_t *proof_first_node, uint32_t n,
                                          uint8_t *status, uint64_t *value_off, uint32_t *value_len);
/* The same for a node-set witness (arguments of phant_mpt_verify_nodeset): the form a block's execution witness arrives in
 * (src/engine_api/execution_payload.zig:121) -- every node crosses the bus once.  Shares the slots with
 * phant_mpt_verify_submit (a slot holds one submission of either kind until phant_wait). */
PHANT_API int32_t phant_mpt_verify_nodeset_submit(phant_ctx *ctx, uint32_t slot, const uint8_t *roots,
                                                  uint32_t n_roots, const uint32_t *root_idx,
                                                  const uint8_t *keys, uint32_t key_len, const uint8_t *nodes,
                                                  uint64_t nodes_len, const uint64_t *node_off,
                                                  uint32_t total_nodes, uint32_t n, uint8_t *status,
                                                  uint64_t *value_off, uint32_t *value_len);
PHANT_API int32_t phant_wait(phant_ctx *ctx, uint32_t slot);

/* ------------------------------------------------------------ several GPUs, one process
 * phant's host is ONE process (src/main.zig:143-149), so the multi-GPU form of the path is inside the library: a
 * phant_comm owns one ctx (device, private stream, workspaces) per device and an RCCL communicator over them
 * (RCCL is looked up at run time; a one-device comm does not need it).  A witness shards with no data-path
 * collective -- proof i is verified on device phant_comm_owner(key_i) = (key_i[0] >> 4) mod N (trie keys are Keccak
 * outputs: uniform) -- and the only exchange is ONE all-reduce (sum) of the n_roots x u32 failure counts over xGMI.
 * devices = NULL: devices 0 .. n_devices - 1; n_devices = 0: all visible devices.  flags: PHANT_CTX_* of the
 * per-device ctxs (the stream flag is ignored).  Externally synchronised like a ctx. */
typedef struct phant_comm phant_comm;
PHANT_API int32_t phant_comm_create(const int32_t *devices, uint32_t n_devices, uint32_t flags, phant_comm **out);
PHANT_API void phant_comm_destroy(phant_comm *comm);
PHANT_API uint32_t phant_comm_size(const phant_comm *comm);
PHANT_API phant_ctx *phant_comm_ctx(phant_comm *comm, uint32_t rank); /* rank's ctx: for device-form calls on its device */
PHANT_API const char *phant_comm_last_error(const phant_comm *comm); /* NULL: why the last phant_comm_create on this thread failed */
PHANT_API uint32_t phant_comm_owner(const phant_comm *comm, const uint8_t *key, uint32_t key_len);
/* Host form of phant_mpt_verify_batch over all devices of the comm (same arguments and outputs, results in the
 * caller's proof order, value_off into the caller's node blob) + fail_count[r] (n_roots, may be NULL) = proofs against
 * root r that are not PRESENT / ABSENT, summed over the devices by the all-reduce: the "one pass/fail per root".
 * The index arrays are read on the host here (the witness is re-packed per device): inconsistent proof_first_node /
 * node_off, or a root_idx entry >= n_roots, make the CALL fail with PHANT_E_INVALID_ARG instead of costing single
 * proofs a BAD_INPUT. */
PHANT_API int32_t phant_mpt_verify_sharded(phant_comm *comm, const uint8_t *roots, uint32_t n_roots,
                                           const uint32_t *root_idx, const uint8_t *keys, uint32_t key_len,
                                           const uint8_t *nodes, uint64_t nodes_len, const uint64_t *node_off,
                                           const uint32_t *proof_first_node, uint32_t n, uint8_t *status,
                                           uint64_t *value_off, uint32_t *value_len, uint32_t *fail_count);
/* The same for a node-set witness (arguments of phant_mpt_verify_nodeset).  A flat set cannot be cut without knowing where
 * its nodes sit in their tries -- which only hashing them tells --, so the cut is the caller's: node_group[j] (total_nodes
 * bytes, or NULL) = the top nibble 0..15 of the keys node j lies under (a node at depth >= 1 of its trie: what a witness
 * producer that walks the tries knows for free), PHANT_NODE_SHARED for a node above that (the tries' root nodes) or of
 * unknown place.  Node j goes to device node_group[j] mod N, a shared one to every device; NULL = every node to every
 * device (correct, no byte saved: the devices then only split the keys).  The hints decide placement and nothing else: a
 * key whose nodes were sent elsewhere gets PHANT_PROOF_MISSING_NODE, as with any incomplete witness -- never a pass it
 * should not get. */
#define PHANT_NODE_SHARED 0xffu
PHANT_API int32_t phant_mpt_verify_nodeset_sharded(phant_comm *comm, const uint8_t *roots, uint32_t n_roots,
                                                   const uint32_t *root_idx, const uint8_t *keys, uint32_t key_len,
                                                   const uint8_t *nodes, uint64_t nodes_len, const uint64_t *node_off,
                                                   uint32_t total_nodes, const uint8_t *node_group, uint32_t n,
                                                   uint8_t *status, uint64_t *value_off, uint32_t *value_len,
                                                   uint32_t *fail_count);
/* Device form of the exchange for callers that keep their shards resident (phant_mpt_verify_verdict_dev on every
 * phant_comm_ctx): d_fail_count[rank] = that device's n_roots counters; summed in place on every device, on the
 * ranks' own streams (not waited for). */
PHANT_API int32_t phant_comm_allreduce_verdict(phant_comm *comm, uint32_t *const *d_fail_count, uint32_t n_roots);

/* mptize (src/mpt/mpt.zig:38-45, arguments as phant_mpt_root, every key at least one byte) with the work spread over the
 * comm's devices by the top key nibble: device d hashes the sub-tries of the nibbles x with x mod N == d
 * (phant_mpt_root_nodes, one forest pass), the host re-roots their root nodes (phant_mpt_strip_first_nibble) and forms
 * the root branch.  Single process: collecting the sixteen child references IS the exchange. */
PHANT_API int32_t phant_mpt_root_sharded(phant_comm *comm, const uint8_t *keys, const uint32_t *key_off,
                                         const uint8_t *vals, const uint64_t *val_off, uint32_t n, uint8_t out[32]);

/* StateDB.root() (arguments of phant_state_root) over the comm's devices: an account belongs to the device that owns the
 * top nibble of keccak256(address); every device turns its accounts into state-trie leaves (phant_state_trie_leaves) and
 * hashes the sub-tries of its nibbles, the root branch is formed on the host. */
PHANT_API int32_t phant_state_root_sharded(phant_comm *comm, const uint8_t *addrs, const uint64_t *nonces,
                                           const uint8_t *balances, const uint8_t *code, const uint64_t *code_off,
                                           const uint8_t *slot_keys, const uint8_t *slot_vals,
                                           const uint32_t *slot_first, uint32_t n, uint8_t out[32]);

/* ------------------------------------------------------------ block witness
 * The step before the kernel: the engine-API witness as JSON, parsed into
 * the packed arrays above and verified in one call.  phant has no witness type yet
 * (src/engine_api/execution_payload.zig:121 commented out, TODO at :175-178); the wire format taken is
 * the JSON-RPC encoding of MPT proofs, EIP-1186 eth_getProof result objects under a state root:
 *   { "stateRoot": "0x<32>", "accounts": [ { "address", "accountProof": [..], "storageHash", "codeHash",
 *     "nonce", "balance", "storageProof": [ { "key", "value", "proof": [..] } ] } ] }
 * with phant's hex conventions (src/common/hexutils.zig:22-37).  Parsing is host-only code (works
 * without a GPU); phant_witness_verify hashes the 20-byte addresses / 32-byte slots into trie keys on
 * the GPU (batched Keccak), verifies account proofs against stateRoot and storage proofs against each
 * account's storageHash in ONE batch, then checks on the host that every proven account leaf
 * rlp([nonce, balance, storageRoot, codeHash]) (src/state/types.zig:13-20) agrees with what the
 * witness declares.  status[i] per proof in document order (account proof, then its storage proofs).
 * The node-SET form of the document -- what an execution witness is (execution_payload.zig:121): every trie node once, in any
 * order, in a top-level "state" array, and NO "accountProof" / "proof" members --
 *   { "stateRoot": "0x<32>", "state": ["0x<rlp node>", ...], "accounts": [ { "address", "storageHash", "codeHash", "nonce",
 *     "balance", "storageProof": [ { "key", "value" } ] } ] }
 * is taken by the same entry points (all three parsers); phant_witness_verify then resolves references by hash
 * (phant_mpt_verify_nodeset: a reference nothing in the set hashes to is PHANT_PROOF_MISSING_NODE). */
typedef struct phant_witness phant_witness;
typedef struct phant_witness_info {
    uint32_t struct_size; /* = sizeof(phant_witness_info) */
    uint32_t n_proofs, n_roots, n_accounts, n_slots, total_nodes;
    uint64_t nodes_len;
    const uint8_t *roots;             /* n_roots x 32: stateRoot, then every account's storageHash */
    const uint32_t *root_idx;         /* n_proofs */
    const uint32_t *account_of;       /* n_proofs: which account the proof belongs to */
    const uint8_t *preimages;         /* 20-byte addresses / 32-byte slots, back to back */
    const uint32_t *preimage_off;     /* n_proofs + 1 */
    const uint8_t *nodes;
    const uint64_t *node_off;         /* total_nodes + 1 */
    const uint32_t *proof_first_node; /* n_proofs + 1 (node-set form: all zero) */
    uint32_t node_set;                /* != 0: the document's nodes are a SET (its "state" array): `nodes` / `node_off` hold every node once */
} phant_witness_info;
/* err (optional, err_cap bytes) receives a message with the byte offset on PHANT_E_INVALID_ARG */
PHANT_API int32_t phant_witness_parse_json(const char *json, uint64_t len, phant_witness **out,
                                           char *err, uint32_t err_cap);
/* the same with the accounts parsed on `threads` host threads (0 = as many as the host has, at most 32; 1 = the
 * calling thread only).  One thread decodes ~1.3 GB/s of JSON; the result is byte-identical. */
PHANT_API int32_t phant_witness_parse_json_mt(const char *json, uint64_t len, uint32_t threads,
                                              phant_witness **out, char *err, uint32_t err_cap);
/* The same document in its INDEX form: everything is parsed as above except the proof nodes' hex digits, which
 * stay in the JSON text -- the witness notes where they are and BORROWS `json` until it has been verified and
 * freed.  phant_witness_verify then ships the text instead of the decoded nodes, decodes the digits on the GPU
 * and fetches only the proven values back.  On the host this leaves the structural scan (one `memchr` per
 * string; profiles/ROWS_NEXT_TO_THE_PATH.md has the measured rates of both forms);
 * the price is 2 bytes over PCIe per node byte.  A node whose
 * digits are not hex is found by the GPU: phant_witness_verify returns PHANT_E_INVALID_ARG (message: which
 * node).  phant_witness_get reports nodes = NULL for this form. */
PHANT_API int32_t phant_witness_index_json(const char *json, uint64_t len, uint32_t threads,
                                           phant_witness **out, char *err, uint32_t err_cap);
PHANT_API void phant_witness_free(phant_witness *w);
/* pointers stay valid until phant_witness_free */
PHANT_API int32_t phant_witness_get(const phant_witness *w, phant_witness_info *info);
/* expected_state_root: the 32-byte state root the CALLER trusts (the parent header's stateRoot): account proofs are
 * verified against IT, whatever the document declares as "stateRoot" -- a witness is an untrusted message, and a
 * self-consistent trie under a root of the sender's choosing proves nothing about the chain.  A document whose own
 * stateRoot differs therefore fails at its account proofs (PHANT_PROOF_BAD_HASH; the storage proofs below them
 * PHANT_PROOF_MISMATCH).  NULL = verify against the document's own stateRoot: a CONSISTENCY check of the document
 * (tests, tools), not a validation. */
PHANT_API int32_t phant_witness_verify(phant_ctx *ctx, const phant_witness *w, const uint8_t *expected_state_root,
                                       uint8_t *status, uint32_t *n_failed);
/* The way back: w as the document phant_witness_parse_json reads -- the per-proof form, or the node-set form for a witness that
 * came from one.  Every declaration the witness holds is written and no other, hex at its full width: parsing the text gives the
 * same phant_witness_get arrays and the same declared fields.  Host only.  *len_out (required) always receives the document's
 * length in bytes (there is no terminating NUL); the text is written only if cap >= *len_out (buf may be NULL with cap == 0):
 * call again with a buffer of the reported size.  The index form (phant_witness_index_json) holds no decoded nodes:
 * PHANT_E_UNSUPPORTED. */
PHANT_API int32_t phant_witness_to_json(const phant_witness *w, char *buf, uint64_t cap, uint64_t *len_out);

/* ------------------------------------------------------- execution witness -> pre-state
 * The witness stateless clients exchange DECLARES nothing: every trie node once in any order, the bytecodes, and the preimages of
 * the touched keys --
 *   { "state": ["0x<rlp node>", ...], "codes": ["0x<bytecode>", ...], "keys": ["0x<20-byte address>" | "0x<address ++ 32-byte slot>", ...] }
 * ("codes" may be absent; unknown members such as "headers" are skipped; hex as phant_witness_parse_json).  Accounts are the distinct
 * addresses of the keys (20-byte keys and the prefixes of 52-byte ones) in order of first appearance; slots are grouped under their
 * account in order of first appearance; duplicate keys collapse.  A key of any other length is PHANT_E_INVALID_ARG (message: its
 * index and the byte offset; a 32-byte slot without its address is not supported).
 * phant_exec_witness_prestate resolves the pre-state the block runs on (src/state/statedb.zig:32 StateDB.init(accounts)) out of the
 * proofs, on the GPU, with ONE host synchronisation: trie keys hashed, the set hashed ONCE and walked twice -- the accounts from
 * state_root (the parent header's: the CALLER's trusted root, required), then every slot from the storage root its account's
 * proven leaf carries --, leaves decoded strictly, and every code hashed (next to the node-set kernels) and matched to the
 * proven codeHash.  Per account: status (PHANT_PROOF_*; a leaf that is no canonical account body: PHANT_PROOF_BAD_VALUE), nonce,
 * balance (32 bytes big-endian), storage root and code hash (an ABSENT account: the empty account), code_index = the lowest index
 * of a code whose keccak256 is the codeHash, PHANT_CODE_NONE for an empty codeHash or a code the witness does not carry (counted
 * in n_missing_code, not a failure: a block may never load it).  Per slot: status (PHANT_PROOF_MISMATCH: its account is neither
 * PRESENT nor ABSENT) and value (32 bytes big-endian, zero when ABSENT).  n_failed = accounts and slots neither PRESENT nor
 * ABSENT; n_unused_codes = codes no PRESENT account's codeHash matches.  Output pointers are caller-owned host memory (NULL: not
 * wanted), sized by phant_exec_witness_info's counts. */
#define PHANT_CODE_NONE 0xffffffffu
typedef struct phant_exec_witness phant_exec_witness;
typedef struct phant_exec_witness_info {
    uint32_t struct_size; /* = sizeof(phant_exec_witness_info) */
    uint32_t n_accounts, n_slots, n_codes, total_nodes;
    uint64_t nodes_len, code_bytes;
    const uint8_t *addresses;   /* n_accounts x 20 */
    const uint32_t *slot_first; /* n_accounts + 1: account i owns slots [slot_first[i], slot_first[i + 1]) */
    const uint8_t *slots;       /* n_slots x 32: the slot preimages */
    const uint8_t *codes;
    const uint64_t *code_off;   /* n_codes + 1 */
    const uint8_t *nodes;
    const uint64_t *node_off;   /* total_nodes + 1 */
} phant_exec_witness_info;
typedef struct phant_prestate {
    uint32_t struct_size; /* = sizeof(phant_prestate) */
    uint8_t *account_status;  /* n_accounts */
    uint64_t *nonces;         /* n_accounts */
    uint8_t *balances;        /* n_accounts x 32 */
    uint8_t *storage_roots;   /* n_accounts x 32 */
    uint8_t *code_hashes;     /* n_accounts x 32 */
    uint32_t *code_index;     /* n_accounts */
    uint8_t *slot_status;     /* n_slots */
    uint8_t *slot_vals;       /* n_slots x 32 */
    uint32_t n_failed, n_missing_code, n_unused_codes;
} phant_prestate;
/* err (optional, err_cap bytes) receives a message with the byte offset on PHANT_E_INVALID_ARG */
PHANT_API int32_t phant_exec_witness_parse_json(const char *json, uint64_t len, phant_exec_witness **out, char *err,
                                                uint32_t err_cap);
PHANT_API void phant_exec_witness_free(phant_exec_witness *w);
/* pointers stay valid until phant_exec_witness_free */
PHANT_API int32_t phant_exec_witness_get(const phant_exec_witness *w, phant_exec_witness_info *info);
PHANT_API int32_t phant_exec_witness_prestate(phant_ctx *ctx, const phant_exec_witness *w, const uint8_t *state_root,
                                              phant_prestate *out);

/* phant_exec_witness_poststate: the state root AFTER the block, from the same witness and the block's writes -- the check of
 * blockchain.zig:83-85 for a client that does not have the state.  The contract:
 *  - Pre-state proof: the call proves the pre-state itself, exactly as phant_exec_witness_prestate does, with the same kernels:
 *    the set is hashed once, the accounts are walked from parent_state_root (required), the slots from the proven storage roots;
 *    the statuses carry the same meaning.
 *  - Failed keys: a key that is neither PRESENT nor ABSENT counts in n_failed.  When n_failed != 0, state_root and storage_roots
 *    are zero-filled.  The call still returns PHANT_OK: an invalid witness is a result, not an error.
 *  - KEEP accounts: the body is unchanged, except that the storage root follows its slot writes.  A KEEP account that is ABSENT
 *    and has a slot write gets PHANT_PROOF_MISMATCH; a slot write under an ABSENT account is valid only with op == SET, which
 *    creates the account with a storage trie that starts empty.
 *  - SET accounts: the leaf becomes rlp([nonce, balance, post storage root, code_hash]) (src/state/types.zig:13-20).
 *  - DELETE accounts: the leaf is removed and the slot writes are ignored.  Deleting an ABSENT account is a no-op.
 *  - Slot writes: a non-zero write sets rlp(minimal big-endian); a zero write removes the slot (statedb.zig:112-119); a zero
 *    write to an ABSENT slot is a no-op.
 *  - The result is the root of the canonical trie over (old key set - removals + inserts): an insert into an empty branch slot,
 *    beside a leaf or inside an extension splits nodes as mptize would build them; a removal that leaves a branch with one child
 *    collapses it and the surviving child merges upward (a leaf takes the longer path, an extension merges with the extension
 *    above it, a branch hangs under an extension).
 *  - Too-thin witnesses: collapsing needs to know what the surviving child is.  If that child is a 32-byte reference that nothing
 *    in the set hashes to, every removed key under that branch gets PHANT_PROOF_MISSING_SIBLING and counts in n_failed; the
 *    child's type is never guessed.  A reference that is the child of an extension in the authenticated old trie is a branch and
 *    needs no lookup.  An inserted key whose path runs into an unresolved reference: PHANT_PROOF_MISSING_NODE.
 *  - Soundness: every byte that enters the new root is a post value the caller passed or a byte of a node reached from
 *    parent_state_root through references resolved by Keccak; nodes of the set not reachable from the trusted root are never read
 *    for content, and the declared order of the set is irrelevant.
 *  - Arguments: NULL ctx, w, io or root, a wrong struct_size, an op outside 0..2 or a NULL input array whose count is non-zero:
 *    PHANT_E_INVALID_ARG.  An array that the ops make unread may be NULL: nonces / balances / code_hashes when no account is SET,
 *    slot_vals when slot_write is NULL.  n_accounts == 0 leaves the root equal to the parent root.
 *  - storage_roots of an account that does not exist afterwards (deleted, or absent and not created): empty_mpt_root.
 *  - One host synchronisation (a second run of the call's kernels only when the device's key order is undecided or the item list
 *    outgrows its estimate: DESIGN.md section 7c). */
#define PHANT_PROOF_MISSING_SIBLING 24  /* poststate only: the key's proof holds, but re-rooting after a removal needs a node
                                           the witness does not carry */
#define PHANT_POST_KEEP 0
#define PHANT_POST_SET 1
#define PHANT_POST_DELETE 2
typedef struct phant_poststate {
    uint32_t struct_size; /* = sizeof(phant_poststate) */
    /* in: the block's writes, in the witness's own account / slot order (phant_exec_witness_info) */
    const uint8_t *account_op;   /* n_accounts: KEEP / SET / DELETE */
    const uint64_t *nonces;      /* n_accounts, read where op == SET */
    const uint8_t *balances;     /* n_accounts x 32 big-endian, read where op == SET */
    const uint8_t *code_hashes;  /* n_accounts x 32, read where op == SET */
    const uint8_t *slot_write;   /* n_slots: != 0 -> slot j's post value is slot_vals[j]; NULL = no slot is written */
    const uint8_t *slot_vals;    /* n_slots x 32 big-endian; an all-zero value removes the slot */
    /* out (NULL: not wanted) */
    uint8_t *state_root;         /* 32 */
    uint8_t *storage_roots;      /* n_accounts x 32: post storage roots */
    uint8_t *account_status;     /* n_accounts */
    uint8_t *slot_status;        /* n_slots */
    uint32_t n_failed;
} phant_poststate;
PHANT_API int32_t phant_exec_witness_poststate(phant_ctx *ctx, const phant_exec_witness *w,
                                               const uint8_t *parent_state_root, phant_poststate *io);

/* phant_exec_witness_advance: phant_exec_witness_poststate, and the nodes of the post-state it built as the witness of the NEXT
 * block -- what lets one witness over the keys of blocks N+1 .. N+k, proven against the root of block N, be checked block by
 * block, and what a client that keeps nodes by hash commits after the block (the "dirty set").  Host form only.  The contract:
 *  - io: arguments, ops, statuses, state_root, storage_roots and n_failed behave exactly as in phant_exec_witness_poststate, with
 *    the same errors; an io passed to both calls gives the same outputs.  next == NULL or a flag bit other than
 *    PHANT_ADVANCE_KEEP_OLD: PHANT_E_INVALID_ARG.
 *  - Failure: when n_failed != 0 (the call reports no root) *next = NULL, and the return is still PHANT_OK.
 *  - Result: otherwise *next is a phant_exec_witness: phant_exec_witness_get / _prestate / _poststate / _advance / _free work on it
 *    unchanged.  It has the keys of w, in the same account and slot order, and the codes of w: a contract the block creates has no
 *    code in it (phant_exec_witness_prestate counts it in n_missing_code), the code of a deleted account becomes unused.
 *  - Its "state" is the set of post-state nodes the call constructs: every node of 32 bytes or more, and every root node, of the
 *    post storage tries of the accounts that exist afterwards and have a slot among the keys, and then of the state trie.  It
 *    holds every node on the post-trie walk of every key of the witness, written or only read -- the walk ends as in rule 3 of
 *    phant_mpt_prove_nodeset; a removed key ends at the node it now diverges from or at an empty slot -- and the new nodes beside
 *    those paths that the writes reshaped: the shortened leaf or extension a split leaves, the survivor of a collapse merged
 *    upward.  Every position appears once; a node under 32 bytes lives inside its parent and is never a member.  Nothing is
 *    emitted for the storage trie of a deleted or never-created account or for a trie that is empty afterwards.  With
 *    n_accounts == 0 there are no nodes.
 *  - Determinism: the same inputs give the same bytes in the same order.  The order is the implementation's: the storage tries by
 *    account index, then the state trie; inside a trie by the position in path order of the list item that carries the node,
 *    deeper nodes first.
 *  - PHANT_ADVANCE_KEEP_OLD: all nodes of w follow the new ones, in w's order, nothing filtered.  This carries the siblings a
 *    producer added under PHANT_PROVE_MAY_REMOVE on to the next block; nodes that nothing reaches any more are harmless to every
 *    verifier here ("Soundness").
 *  - One host synchronisation, plus the second runs phant_exec_witness_poststate has and a rare third kind: the room for the nodes
 *    is estimated before the launch (the witness's own node bytes, a leaf per key, slack); nodes beyond it are counted, not
 *    written, and the call's kernels run again with the counted sizes. */
#define PHANT_ADVANCE_KEEP_OLD 1u
PHANT_API int32_t phant_exec_witness_advance(phant_ctx *ctx, const phant_exec_witness *w,
                                             const uint8_t *parent_state_root, phant_poststate *io, uint32_t flags,
                                             phant_exec_witness **next);

/* ---------------------------------------------------------------- trie root
 * Replaces src/mpt/mpt.zig:38 `mptize(arena, list: []const KeyVal) !Hash32`
 * (KeyVal = mpt.zig:13-34: key bytes expanded to nibbles, value borrowed).
 *   key i   = keys[key_off[i] .. key_off[i+1])   (bytes, any length <= 255)
 *   value i = vals[val_off[i] .. val_off[i+1])
 * Keys must be strictly increasing (mpt.zig:39) else PHANT_E_UNSORTED.
 * n == 0 gives mpt.zig:10 `empty_mpt_root`. */
PHANT_API int32_t phant_mpt_root(phant_ctx *ctx, const uint8_t *keys, const uint32_t *key_off,
                                 const uint8_t *vals, const uint64_t *val_off, uint32_t n,
                                 uint8_t out[32]);
/* The same over DEVICE-resident arrays (PCIe out of the picture): d_key_off / d_val_off are relative to d_keys /
 * d_vals, key_bytes / val_bytes their totals (= d_key_off[n] / d_val_off[n], known to the caller who packed them); the
 * root is written to d_root (device, 32 bytes, 4-byte aligned).  Keys of at most 255 bytes; the call synchronises the
 * ctx stream (it reads the depth histogram and the UNSORTED flag back while it builds). */
PHANT_API int32_t phant_mpt_root_dev(phant_ctx *ctx, const uint8_t *d_keys, const uint32_t *d_key_off, uint64_t key_bytes,
                                     const uint8_t *d_vals, const uint64_t *d_val_off, uint64_t val_bytes, uint32_t n,
                                     uint8_t *d_root);

/* ------------------------------------------------------- witness generation
 * The nodes a verifier needs for a set of queried keys, cut from the tries of a forest: the producing half of
 * phant_mpt_verify_nodeset.  What this call emits, phant_mpt_verify_nodeset accepts under the emitted roots with the statuses
 * reported here.
 *
 * 1. The forest: keys / key_off / vals / val_off / n as phant_mpt_root (sorted inside every trie, keys <= 255 bytes; the same
 *    errors), trie t owning keys [seg_first[t], seg_first[t + 1]) as in phant_mpt_root_nodes.  seg_first == NULL with
 *    n_tries == 1: one trie.
 * 2. The queries: key j = qkeys[qkey_off[j] .. qkey_off[j + 1]) (any length), against trie q_trie[j] (NULL: trie 0; an index >=
 *    n_tries is PHANT_E_INVALID_ARG), with q_flags[j] (NULL: all zero).  Queries may repeat and come in any order.
 * 3. For trie t the call emits the union over its queries of the hashed nodes from the root node down to where the walk of the
 *    verifier ends: at the key's leaf or branch value, at the leaf or extension whose path diverges from the key (that node
 *    included), or at the branch whose slot for the key's next nibble is empty.  A node shorter than 32 bytes lives inside its
 *    parent and is never a member; an extension and the branch under it are two nodes.  An empty trie and a trie without queries
 *    contribute nothing (their roots are still written).
 * 4. Every node POSITION is written once, however many queries pass through it; byte-identical nodes of two tries may both
 *    appear.  Nodes come grouped by trie in trie order: trie t's are nodes [trie_first_node[t], trie_first_node[t + 1]).  The
 *    order inside a trie is the implementation's, and the same inputs give the same bytes.
 * 5. PHANT_PROVE_MAY_REMOVE (bit 0 of q_flags[j]): the caller may remove this key, and phant_exec_witness_poststate must then
 *    be able to collapse a branch on its path.  Every flagged query that is PRESENT marks the position (nibble, or the value) it
 *    passes through in each branch on its path.  A branch of which exactly ONE occupied position is unmarked, that position
 *    holding a 32-byte reference, has the node under that position added to the set (that node only).  A branch collapses only if
 *    all but one of its positions vanish, and a position vanishes only through flagged keys: so this covers every set of
 *    removals among the flagged keys.
 * 6. Capacity.  total_nodes and nodes_len are always written.  If total_nodes > max_nodes or nodes_len > nodes_cap the call
 *    still returns PHANT_OK, and nodes / node_off are left untouched: call again with the reported sizes.
 *    Every output pointer may be NULL (not wanted).  struct_size must be sizeof(phant_prove_out), else PHANT_E_INVALID_ARG. */
#define PHANT_PROVE_MAY_REMOVE 1u
typedef struct phant_prove_out {
    uint32_t struct_size;      /* = sizeof(phant_prove_out) */
    uint32_t max_nodes;        /* node_off holds max_nodes + 1 entries */
    uint64_t nodes_cap;        /* bytes of nodes */
    uint8_t *nodes;            /* node bytes back to back */
    uint64_t *node_off;        /* total_nodes + 1 */
    uint32_t *trie_first_node; /* n_tries + 1 */
    uint8_t *roots;            /* n_tries x 32: the mptize roots */
    uint8_t *q_status;         /* n_queries: PHANT_PROOF_PRESENT / PHANT_PROOF_ABSENT */
    /* results */
    uint64_t nodes_len;
    uint32_t total_nodes;
    uint32_t reserved;
} phant_prove_out;
PHANT_API int32_t phant_mpt_prove_nodeset(phant_ctx *ctx, const uint8_t *keys, const uint32_t *key_off,
                                          const uint8_t *vals, const uint64_t *val_off, uint32_t n,
                                          const uint32_t *seg_first /* n_tries + 1, or NULL */, uint32_t n_tries,
                                          const uint8_t *qkeys, const uint32_t *qkey_off /* n_queries + 1 */,
                                          const uint32_t *q_trie /* or NULL */, const uint8_t *q_flags /* or NULL */,
                                          uint32_t n_queries, phant_prove_out *out);
/* The same over DEVICE-resident tries and queries (offsets relative to their blobs, key_bytes / val_bytes / qkey_bytes the blobs'
 * totals as in phant_mpt_root_dev).  `out` itself is host memory; the buffers it points to are device memory (roots 4-byte
 * aligned, node_off 8-byte aligned); an out-of-range q_trie entry is found on the device.  d_qkey_off is TRUSTED: the caller who packed
 * the queries guarantees n_queries + 1 ascending entries from 0 to qkey_bytes; the locate lanes read d_qkeys through it unchecked
 * (the forest's own offsets are checked on the device as in phant_mpt_root_dev).  The call synchronises the ctx stream. */
PHANT_API int32_t phant_mpt_prove_nodeset_dev(phant_ctx *ctx, const uint8_t *d_keys, const uint32_t *d_key_off, uint64_t key_bytes,
                                              const uint8_t *d_vals, const uint64_t *d_val_off, uint64_t val_bytes, uint32_t n,
                                              const uint32_t *d_seg_first /* n_tries + 1, or NULL */, uint32_t n_tries,
                                              const uint8_t *d_qkeys, const uint32_t *d_qkey_off, uint64_t qkey_bytes,
                                              const uint32_t *d_q_trie /* or NULL */, const uint8_t *d_q_flags /* or NULL */,
                                              uint32_t n_queries, phant_prove_out *out);

/* The per-proof form: an ordered node list per query, root first -- the EIP-1186 eth_getProof shape, the producing half of
 * phant_mpt_verify_batch.  (roots, root_idx = q_trie, nodes, node_off, proof_first_node) go into phant_mpt_verify_batch[_dev]
 * unchanged, and the statuses it finds are the q_status reported here.
 *
 * 1. The forest and the queries exactly as phant_mpt_prove_nodeset takes them (rules 1 and 2 above: the same sortedness, key-length
 *    and q_trie errors; queries of any length, repeated, in any order).  There are no q_flags: PHANT_PROVE_MAY_REMOVE names nodes
 *    off a key's path, which have no place in an ordered proof.
 * 2. Proof j = nodes [proof_first_node[j], proof_first_node[j + 1]), root first: the hashed nodes on the verifier's walk (DESIGN.md
 *    section 3) for query j, down to the key's leaf or branch value, to the leaf or extension whose path diverges from the key (that
 *    node included), or to the branch whose slot for the key's next nibble is empty.  A node shorter than 32 bytes lives inside its
 *    parent and is not listed; a trie's root node is always listed; an extension and the branch under it are two nodes.  An empty
 *    trie gives an empty proof (no nodes) with status PHANT_PROOF_ABSENT.
 * 3. Proofs lie back to back in query order, node_off[0] == 0, node k = nodes[node_off[k] .. node_off[k + 1]).  Repeated queries
 *    repeat their bytes.  The same inputs give the same bytes.
 * 4. roots is written for every trie, queried or not.  n_queries == 0: PHANT_OK, both totals 0, proof_first_node[0] = 0,
 *    node_off[0] = 0.
 * 5. Capacity, as rule 6 above: total_nodes and nodes_len are always written.  If total_nodes > max_nodes or nodes_len > nodes_cap
 *    the call still returns PHANT_OK and leaves nodes, node_off and proof_first_node untouched: call again with the reported sizes.
 *    Every output pointer may be NULL (not wanted; a buffer nobody wants has no capacity to exceed).  struct_size must be
 *    sizeof(phant_prove_batch_out), else PHANT_E_INVALID_ARG.
 * 6. All proofs together hold at most 2^32 - 1 nodes; more is PHANT_E_UNSUPPORTED. */
typedef struct phant_prove_batch_out {
    uint32_t struct_size;       /* = sizeof(phant_prove_batch_out) */
    uint32_t max_nodes;         /* node_off holds max_nodes + 1 entries */
    uint64_t nodes_cap;         /* bytes of nodes */
    uint8_t *nodes;             /* node bytes back to back */
    uint64_t *node_off;         /* total_nodes + 1 */
    uint32_t *proof_first_node; /* n_queries + 1 */
    uint8_t *roots;             /* n_tries x 32: the mptize roots */
    uint8_t *q_status;          /* n_queries: PHANT_PROOF_PRESENT / PHANT_PROOF_ABSENT */
    /* results */
    uint64_t nodes_len;
    uint32_t total_nodes;
    uint32_t reserved;
} phant_prove_batch_out;
PHANT_API int32_t phant_mpt_prove_batch(phant_ctx *ctx, const uint8_t *keys, const uint32_t *key_off,
                                        const uint8_t *vals, const uint64_t *val_off, uint32_t n,
                                        const uint32_t *seg_first /* n_tries + 1, or NULL */, uint32_t n_tries,
                                        const uint8_t *qkeys, const uint32_t *qkey_off /* n_queries + 1 */,
                                        const uint32_t *q_trie /* or NULL */, uint32_t n_queries, phant_prove_batch_out *out);
/* The same over DEVICE-resident tries and queries (offsets relative to their blobs, key_bytes / val_bytes / qkey_bytes the blobs'
 * totals as in phant_mpt_root_dev).  `out` itself is host memory; the buffers it points to are device memory (roots and
 * proof_first_node 4-byte aligned, node_off 8-byte aligned, nodes at any address); an out-of-range q_trie entry is found on the
 * device.  d_qkey_off is TRUSTED: the caller who packed the queries guarantees n_queries + 1 ascending entries from 0 to
 * qkey_bytes; the locate lanes read d_qkeys through it unchecked (the forest's own offsets are checked on the device as in
 * phant_mpt_root_dev).  The call synchronises the ctx stream. */
PHANT_API int32_t phant_mpt_prove_batch_dev(phant_ctx *ctx, const uint8_t *d_keys, const uint32_t *d_key_off, uint64_t key_bytes,
                                            const uint8_t *d_vals, const uint64_t *d_val_off, uint64_t val_bytes, uint32_t n,
                                            const uint32_t *d_seg_first /* n_tries + 1, or NULL */, uint32_t n_tries,
                                            const uint8_t *d_qkeys, const uint32_t *d_qkey_off, uint64_t qkey_bytes,
                                            const uint32_t *d_q_trie /* or NULL */, uint32_t n_queries, phant_prove_batch_out *out);

/* Callers of mptize ("next" rows):
 * src/blockchain/blockchain.zig:209-235 calculateMPTRoot -- key rlp(index) */
PHANT_API int32_t phant_index_root_rlp(phant_ctx *ctx, const uint8_t *items,
                                       const uint64_t *item_off, uint32_t n, uint8_t out[32]);
/* src/engine_api/execution_payload.zig:125-158 toBlock -- key = 32-byte
 * big-endian index */
PHANT_API int32_t phant_index_root_be32(phant_ctx *ctx, const uint8_t *items,
                                        const uint64_t *item_off, uint32_t n, uint8_t out[32]);

/* All index-keyed roots of one block in ONE pass -- what src/blockchain/blockchain.zig:198-204 computes with three
 * calculateMPTRoot calls (transactions, receipts, withdrawals; key rlp(index) as phant_index_root_rlp).  The trie hasher
 * works level by level, and at these sizes (<= a few hundred items) a level is pure latency: the lists go through it as one
 * forest, so that latency is paid once per block instead of once per list.  List l = items[l][item_off[l][0] ..
 * item_off[l][n[l]]) with n[l] + 1 offsets; n[l] == 0 (items[l] / item_off[l] may then be NULL) gives mpt.zig:10
 * empty_mpt_root.  roots_out = n_lists x 32 bytes, in list order.
 * Optionally the block's logs blooms in the same call (arguments as phant_logs_bloom; bloom_items == NULL: none). */
PHANT_API int32_t phant_block_roots(phant_ctx *ctx, const uint8_t *const *items, const uint64_t *const *item_off,
                                    const uint32_t *n, uint32_t n_lists, uint8_t *roots_out,
                                    const uint8_t *bloom_items, const uint64_t *bloom_item_off,
                                    const uint32_t *bloom_item_receipt, uint32_t n_bloom_items, uint32_t n_receipts,
                                    uint8_t *blooms);

/* ------------------------------------------------------- range proofs
 * phant_mpt_verify_ranges decides, for n_ranges ranges at once, whether a sorted run of consecutive leaves is EXACTLY what the trie
 * under a trusted root holds between an origin and the run's last key, and whether anything lies to the right of the run (snap
 * sync's AccountRange / StorageRanges; any state filled chunk by chunk from untrusted peers).  tests/range_ref.py is the same
 * definition in plain Python.
 *
 * Keys are 32 bytes (64 nibbles).  The call holds ONE node set for all its ranges: nodes[node_off[i] .. node_off[i+1]), any order,
 * every node hashed once; a node that nothing reachable refers to is never decoded.  Range r: roots[r], origins[r], has_proof[r]
 * and the leaves leaf_first[r] .. leaf_first[r+1]: keys (32 bytes each) and vals[val_off[j] .. val_off[j+1]), the full leaf values.
 *
 * For one range with leaves k_0 < ... < k_(m-1) the ITEM LIST is the concatenation of
 *  1. (has_proof) what lies to the LEFT of origin.  Walk origin's path from the root through the set.  At a branch at depth d every
 *     non-empty slot s < origin[d] is an opaque reference with path origin[0..d) + s.  Where the walk leaves the path at a leaf or an
 *     extension whose path is SMALLER than origin's nibbles there, that leaf (with its value from the node) or that extension's child
 *     (a known branch, with the extension's path) is an item; a GREATER one is none: it lies in the range and the leaves must supply
 *     it.  The walk ends at an empty slot, at origin's own leaf (no item: it is k_0, or the root will not match) or at a divergence.
 *  2. the m leaves with the caller's values.
 *  3. (has_proof and m > 0) what lies to the RIGHT of k_(m-1): the mirror walk -- slots s > k_(m-1)[d], a diverging leaf / extension
 *     only when it is GREATER.  has_more = this walk found an item.
 * The range is VALID iff the list is strictly ordered and prefix-free and the root of the trie over it (the empty list: the empty
 * root; a root node is always hashed) equals roots[r].  Without a proof origin is ignored and the leaves are the whole trie; with a
 * proof and no leaves the claim is "nothing at or above origin".  has_more is 0 without a proof, without leaves and on failure.
 *
 * status[r] is PHANT_RANGE_VALID or the first failure in this order:
 *  1. the leaf rules, at the least leaf that breaks one, there in this order: PHANT_RANGE_EMPTY_VALUE (length 0),
 *     PHANT_RANGE_VALUE_TOO_LONG (more than 560 bytes), PHANT_RANGE_BAD_ORDER (the key is not greater than the one before it),
 *     PHANT_RANGE_BELOW_ORIGIN (the first leaf of a range with a proof is below origin).  bad_leaf[r] = that leaf's index in the
 *     call, else 0xFFFFFFFF.
 *  2. the walks, origin's first: PHANT_PROOF_MISSING_NODE (a reference nothing in the set hashes to), PHANT_PROOF_BAD_NODE (not
 *     canonical RLP of a trie node, a branch with a value, a path beyond 64 nibbles).
 *  3. PHANT_RANGE_ROOT_MISMATCH: everything else -- an item of the proof that overlaps or precedes a leaf, a branch left with one
 *     child whose type the set does not say (such a reference is never looked up and merged), a leaf of the proof itself longer
 *     than 560 bytes, another root.
 * computed_root[r] = the root built (32 zero bytes on failure).  A failing range changes nothing about any other range of the call.
 * n_failed = ranges that are not VALID, first_failed = the least of them (n_ranges: none).
 *
 * Any output pointer may be NULL.  PHANT_E_INVALID_ARG, with nothing written: a wrong struct_size, reserved != 0, a NULL input
 * whose count is not zero (origins is needed when some has_proof is set -- the device form asks for it whenever n_ranges > 0;
 * nodes / node_off with n_nodes == 0 and keys / vals / val_off with n_leaves == 0 may be NULL), leaf_first / val_off / node_off
 * that do not start at 0, go backwards or do not end at n_leaves / vals_len / nodes_len, leaves or nodes (n_leaves, n_nodes != 0)
 * in a call without a range.  PHANT_E_UNSUPPORTED: 2^31 leaves + ranges or more.  PHANT_E_OOM: an item list (the leaves and what the
 * walks leave beside their paths) of 2^30 items or more, like memory that cannot be had.  n_ranges == 0 without leaves and nodes is
 * PHANT_OK.  Host form: checked on the host, one staged upload, the launches, one copy back that
 * ends at the last wanted output, one synchronisation.  Device form: every array is device memory (uint64_t arrays 8-byte, uint32_t
 * arrays 4-byte aligned; misaligned: PHANT_E_INVALID_ARG), both structs host memory; the offsets are checked by a kernel whose verdict
 * the host reads before any other kernel indexes with them; the call synchronises the ctx stream. */
#define PHANT_RANGE_VALID 1
#define PHANT_RANGE_EMPTY_VALUE 32    /* a leaf without a value */
#define PHANT_RANGE_VALUE_TOO_LONG 33 /* a leaf value of more than 560 bytes */
#define PHANT_RANGE_BAD_ORDER 34      /* a key not greater than the one before it */
#define PHANT_RANGE_BELOW_ORIGIN 35   /* the first leaf lies in front of the origin */
#define PHANT_RANGE_ROOT_MISMATCH 36  /* the leaves and the proof do not make the trusted root */
typedef struct phant_ranges_in {
    uint32_t struct_size; /* = sizeof(phant_ranges_in) */
    uint32_t n_ranges;
    uint32_t n_leaves;
    uint32_t n_nodes;
    uint32_t reserved[2]; /* 0 */
    uint64_t vals_len;
    uint64_t nodes_len;
    /* per range */
    const uint8_t *roots;       /* n_ranges x 32 */
    const uint8_t *origins;     /* n_ranges x 32 */
    const uint32_t *leaf_first; /* n_ranges + 1 */
    const uint8_t *has_proof;   /* n_ranges */
    /* per leaf */
    const uint8_t *keys;     /* n_leaves x 32 */
    const uint8_t *vals;     /* vals_len */
    const uint64_t *val_off; /* n_leaves + 1 */
    /* the node set */
    const uint8_t *nodes;     /* nodes_len */
    const uint64_t *node_off; /* n_nodes + 1 */
} phant_ranges_in;
typedef struct phant_ranges_out {
    uint32_t struct_size; /* = sizeof(phant_ranges_out) */
    uint32_t n_failed;    /* results ... */
    uint32_t first_failed;
    uint32_t reserved[2]; /* 0 */
    /* per range */
    uint8_t *status;        /* PHANT_RANGE_* / PHANT_PROOF_MISSING_NODE / PHANT_PROOF_BAD_NODE */
    uint8_t *has_more;      /* 0 / 1 */
    uint8_t *computed_root; /* 32 */
    uint32_t *bad_leaf;
} phant_ranges_out;
PHANT_API int32_t phant_mpt_verify_ranges(phant_ctx *ctx, const phant_ranges_in *in, phant_ranges_out *out);
PHANT_API int32_t phant_mpt_verify_ranges_dev(phant_ctx *ctx, const phant_ranges_in *in, phant_ranges_out *out);

/* ------------------------------------------- sharded trie roots (multi-GPU mptize)
 * a trie shards by the top key nibble -- 16 sub-tries, one exchange of <= 33-byte
 * child references, then the root branch.  A rank calls phant_mpt_root_nodes over its sub-tries (one
 * segment per top nibble, all keys of a segment sharing it): besides each segment's mptize root it gets
 * the RLP of that root NODE -- an extension [HP(x p), next] or a leaf [HP(x rest), value] -- and
 * phant_mpt_strip_first_nibble (host-only, no GPU) re-roots it one nibble lower: the node the full
 * trie's root branch refers to in slot x (is_ref = 0: a node, to be embedded if shorter than 32 bytes
 * and hashed otherwise, mpt.zig:104/:112), or, when the extension carried only that nibble, its child
 * reference itself (is_ref = 1: 32 hash bytes or an embedded RLP < 32 bytes).
 * phant_amd/shard.py::mptize_sharded is the tested composition (all-reduce of 16 x 33 bytes). */
PHANT_API int32_t phant_mpt_root_nodes(phant_ctx *ctx, const uint8_t *keys, const uint32_t *key_off,
                                       const uint8_t *vals, const uint64_t *val_off, uint32_t n,
                                       const uint32_t *seg_first /* n_tries + 1 */, uint32_t n_tries,
                                       uint8_t *roots /* n_tries x 32 */,
                                       uint8_t *node_rlp /* n_tries x node_cap */, uint32_t node_cap,
                                       uint32_t *node_len /* n_tries; 0 = empty trie; > node_cap = not written */);
PHANT_API int32_t phant_mpt_strip_first_nibble(const uint8_t *node, uint32_t len, uint8_t *out,
                                               uint32_t cap, uint32_t *out_len, uint32_t *is_ref);

/* State root: the `StateDB.root()` the reference lacks
 * (src/blockchain/blockchain.zig:83-85).  Inputs are the AccountState fields
 * of src/state/types.zig:13-20 in struct-of-arrays form:
 *   addrs n x 20, nonces n, balances n x 32 (big-endian u256),
 *   code blob + code_off[n+1], storage slots slot_keys/slot_vals m x 32
 *   (big-endian u256) with account i owning [slot_first[i], slot_first[i+1]).
 * Zero-valued slots are skipped (src/state/statedb.zig:112-119). */
PHANT_API int32_t phant_state_root(phant_ctx *ctx, const uint8_t *addrs, const uint64_t *nonces,
                                   const uint8_t *balances, const uint8_t *code,
                                   const uint64_t *code_off, const uint8_t *slot_keys,
                                   const uint8_t *slot_vals, const uint32_t *slot_first,
                                   uint32_t n, uint8_t out[32]);

/* The same over DEVICE-resident struct-of-arrays (a node that keeps its state in HBM: nothing of it crosses the bus): offsets
 * relative -- d_code_off[0] == 0, d_slot_first[0] == 0 --, code_bytes = d_code_off[n] and n_slots = d_slot_first[n] given by
 * the caller who packed them (checked on the device: PHANT_E_INVALID_ARG); d_slot_vals, d_balances and d_root 4-byte aligned.
 * The root is written to d_root (device, 32 bytes).  The call synchronises the ctx stream a few times (it reads counters back
 * while it builds: live slots, leaf bytes, the tries' depth histograms). */
PHANT_API int32_t phant_state_root_dev(phant_ctx *ctx, const uint8_t *d_addrs, const uint64_t *d_nonces,
                                       const uint8_t *d_balances, const uint8_t *d_code, const uint64_t *d_code_off,
                                       uint64_t code_bytes, const uint8_t *d_slot_keys, const uint8_t *d_slot_vals,
                                       const uint32_t *d_slot_first, uint32_t n_slots, uint32_t n, uint8_t *d_root);
/* phant_state_witness: the execution witness a node that HOLDS the state ships with a payload
 * (src/engine_api/execution_payload.zig:121) -- the producing half of phant_exec_witness_prestate / _poststate.  The contract:
 *  - The state: the struct-of-arrays of phant_state_root (host memory), every address once.
 *  - The keys: key k = wkeys[wkey_off[k] .. wkey_off[k + 1]) is a 20-byte address or a 52-byte address ++ slot, under the rules
 *    of phant_exec_witness_parse_json: accounts are the distinct addresses in order of first appearance, slots grouped under their
 *    account in order of first appearance, duplicates collapse (their flags are ORed).  Any other length: PHANT_E_INVALID_ARG,
 *    the key's index in phant_last_error.
 *  - The result is a phant_exec_witness, the object the parser returns: phant_exec_witness_get / _prestate / _poststate / _free
 *    work on it unchanged.  "state" holds the state-trie nodes on the paths of every touched address (an exclusion proof for an
 *    address the state does not hold), followed by the storage-trie nodes on the paths of every touched slot of an account the
 *    state holds (a zero-valued slot is not in the trie, statedb.zig:112-119: an exclusion proof; an account without live slots
 *    has the empty root and contributes nothing) -- each set as phant_mpt_prove_nodeset emits it, every node position once.
 *    "codes" holds each distinct non-empty bytecode of a touched account the state holds once, in order of first appearance,
 *    told apart by the code hash the state pass computes.  "keys" are the caller's keys, grouped as above.
 *  - state_root_out (required): the state root, equal to phant_state_root on the same arrays; the root to hand to _prestate.
 *  - wkey_flags (NULL: all zero): bit 0 = PHANT_PROVE_MAY_REMOVE.  On a 52-byte key it flags the slot in its account's storage
 *    trie, on a 20-byte key the account in the state trie: the siblings a collapse would need join the set (rule 5 above).
 *  - The storage forest is proven while its tables stand, the state trie behind it; the touched keys are hashed on the device.
 *    Host form only.  A call without keys returns a witness without nodes. */
PHANT_API int32_t phant_state_witness(phant_ctx *ctx, const uint8_t *addrs, const uint64_t *nonces, const uint8_t *balances,
                                      const uint8_t *code, const uint64_t *code_off, const uint8_t *slot_keys,
                                      const uint8_t *slot_vals, const uint32_t *slot_first, uint32_t n, const uint8_t *wkeys,
                                      const uint32_t *wkey_off /* n_wkeys + 1 */, const uint8_t *wkey_flags /* or NULL */,
                                      uint32_t n_wkeys, phant_exec_witness **out, uint8_t state_root_out[32]);

/* phant_state_proofs: eth_getProof for a node that HOLDS the state -- the per-proof twin of phant_state_witness.
 *  - The state and the keys as phant_state_witness takes them (host memory; 20-byte address or 52-byte address ++ slot, accounts
 *    in order of first appearance, slots grouped under their account, duplicates collapse; any other length:
 *    PHANT_E_INVALID_ARG, the key's index in phant_last_error).  There are no flags.
 *  - The result is a phant_witness in its per-proof form, the object phant_witness_parse_json returns: phant_witness_get /
 *    _verify / _to_json / _free work on it unchanged.  Proofs come in document order: an account's proof, then its storage
 *    proofs, each the ordered list phant_mpt_prove_batch cuts.  roots = the state root, then every account's storage root.
 *    The declared nonce / balance / storageHash / codeHash and the slot values are taken from the state.
 *  - An address the state does not hold gets its exclusion proof, the declarations of the empty account (nonce 0, balance 0,
 *    the empty storage root, the hash of the empty code) and, for its slots, zero-node proofs against the empty root with value
 *    0.  A zero-valued or missing slot of a held account gets its exclusion proof with value 0 (an account without live slots
 *    has the empty root: a zero-node proof).
 *  - state_root_out (required): the state root, equal to phant_state_root on the same arrays.
 *  - The storage forest is proven while its tables stand, the state trie behind it; the keys are hashed on the device.  Host
 *    form only.  A call without keys returns a witness without proofs. */
PHANT_API int32_t phant_state_proofs(phant_ctx *ctx, const uint8_t *addrs, const uint64_t *nonces, const uint8_t *balances,
                                     const uint8_t *code, const uint64_t *code_off, const uint8_t *slot_keys,
                                     const uint8_t *slot_vals, const uint32_t *slot_first, uint32_t n, const uint8_t *wkeys,
                                     const uint32_t *wkey_off /* n_wkeys + 1 */, uint32_t n_wkeys, phant_witness **out,
                                     uint8_t state_root_out[32]);

/* One rank's share of a SHARDED state root (arguments as phant_state_root): the sub-tries of its accounts by the top nibble x
 * of the hashed address, in one pass -- roots[32 x] = that sub-trie's mptize root, root_enc[root_enc_cap x ..] = the RLP of its
 * root NODE (what phant_mpt_strip_first_nibble re-roots one nibble lower), root_enc_len[x] its length, 0 when the rank has no
 * account under x.  The leaves stay on the device (phant_state_trie_leaves + phant_mpt_root_nodes is the same result with a
 * round trip through host memory).  root_enc_cap <= 256; 200 bytes hold any state-trie root node. */
PHANT_API int32_t phant_state_subtrie_nodes(phant_ctx *ctx, const uint8_t *addrs, const uint64_t *nonces,
                                            const uint8_t *balances, const uint8_t *code, const uint64_t *code_off,
                                            const uint8_t *slot_keys, const uint8_t *slot_vals, const uint32_t *slot_first,
                                            uint32_t n, uint8_t *roots, uint8_t *root_enc, uint32_t root_enc_cap,
                                            uint32_t *root_enc_len);

/* The LEAVES of that state trie instead of its root -- what a rank of a multi-GPU state root (SURVEY.md
 * section 8e) computes for the accounts it owns before the top-nibble exchange of mptize_sharded: keys = n x 32,
 * keccak256(address) in ascending order; value i = vals[val_off[i] .. val_off[i+1]) =
 * rlp([nonce, balance, storageRoot, codeHash]) of the account with that key, its storage root computed here
 * (same forest pass as phant_state_root).  vals_cap: bytes available at `vals`; an account's RLP is at most
 * 110 bytes.  phant_amd/shard.py::state_root_sharded is the tested composition. */
PHANT_API int32_t phant_state_trie_leaves(phant_ctx *ctx, const uint8_t *addrs, const uint64_t *nonces,
                                          const uint8_t *balances, const uint8_t *code,
                                          const uint64_t *code_off, const uint8_t *slot_keys,
                                          const uint8_t *slot_vals, const uint32_t *slot_first, uint32_t n,
                                          uint8_t *keys, uint8_t *vals, uint64_t vals_cap, uint64_t *val_off);

#ifdef __cplusplus
}
#endif
#endif /* PHANT_GPU_H */
