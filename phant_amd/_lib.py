"""ctypes loader for libphant_gpu.so -- the C-ABI of include/phant_gpu.h.

There is no fallback: if the HIP library is missing or no gfx950 device is
usable, the calls raise.  torch is imported first on purpose: it ships its own
libamdhip64.so.7, and loading ours afterwards makes the dynamic linker reuse
that one HIP runtime (device pointers and streams are then shared between
torch tensors and this library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL below; see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libphant_gpu.so")

OK = 0
E_INVALID_ARG = -1
E_OOM = -2
E_DEVICE = -3
E_NO_DEVICE = -4
E_UNSORTED = -5
E_UNSUPPORTED = -6

PROOF_INVALID_EMPTY = 0
PROOF_PRESENT = 1
PROOF_ABSENT = 2
PROOF_BAD_HASH = 16
PROOF_BAD_RLP = 17
PROOF_BAD_NODE = 18
PROOF_EXTRA_NODES = 19
PROOF_MISSING_NODE = 20
PROOF_BAD_INPUT = 21
PROOF_MISMATCH = 22
PROOF_BAD_VALUE = 23
PROOF_MISSING_SIBLING = 24
# PHANT_RANGE_*: phant_mpt_verify_ranges (beside PROOF_MISSING_NODE and PROOF_BAD_NODE)
RANGE_VALID = 1
RANGE_EMPTY_VALUE = 32
RANGE_VALUE_TOO_LONG = 33
RANGE_BAD_ORDER = 34
RANGE_BELOW_ORIGIN = 35
RANGE_ROOT_MISMATCH = 36
RANGE_NO_LEAF = 0xFFFFFFFF
POST_KEEP, POST_SET, POST_DELETE = 0, 1, 2
PROVE_MAY_REMOVE = 1
ADVANCE_KEEP_OLD = 1
CODE_NONE = 0xFFFFFFFF
SIG_OK, SIG_BAD_RANGE, SIG_HIGH_S, SIG_BAD_RECID, SIG_NOT_ON_CURVE, SIG_INFINITY, SIG_BAD_TX, SIG_BAD_V = range(8)
RECOVER_LOW_S = 1

# every symbol include/phant_gpu.h declares: (name, restype, argtypes)
_vp, _u32, _u64, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
SYMBOLS = {
    "phant_version": (C.c_char_p, []),
    "phant_device_count": (_i32, []),
    "phant_ctx_create": (_i32, [_vp, C.POINTER(_vp)]),
    "phant_ctx_destroy": (None, [_vp]),
    "phant_last_error": (C.c_char_p, [_vp]),
    "phant_set_stream": (_i32, [_vp, _vp]),
    "phant_stream_sync": (_i32, [_vp]),
    "phant_keccak256": (_i32, [_vp, _vp, _u64, _vp]),
    "phant_keccak256_with_prefix": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "phant_keccak256_batch": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_keccak256_batch_dev": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_sha256_batch": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_sha256_batch_dev": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_keccak256_fixed_dev": (_i32, [_vp, _vp, _u32, _u64, _u32, _vp]),
    "phant_logs_bloom": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "phant_logs_bloom_dev": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "phant_sender_addresses": (_i32, [_vp, _vp, _u64, _u32, _vp]),
    "phant_sender_addresses_dev": (_i32, [_vp, _vp, _u64, _u32, _vp]),
    "phant_block_receipts": (_i32, [_vp, _vp, _vp]),
    "phant_block_receipts_dev": (_i32, [_vp, _vp, _vp]),
    "phant_header_chain": (_i32, [_vp, _vp, _vp]),
    "phant_header_chain_dev": (_i32, [_vp, _vp, _vp]),
    "phant_headers_decode_rlp": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp]),
    "phant_ecrecover_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "phant_ecrecover_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "phant_tx_senders": (_i32, [_vp, _vp, _vp, _u32, _u64, _vp, _vp]),
    "phant_block_transactions": (_i32, [_vp, _vp, _vp]),
    "phant_block_transactions_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_transactions_ex": (_i32, [_vp, _vp, _vp]),
    "phant_block_transactions_ex_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_bodies": (_i32, [_vp, _vp, _vp]),
    "phant_block_bodies_dev": (_i32, [_vp, _vp, _vp]),
    "phant_bodies_decode_rlp": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp]),
    "phant_block_receipt_segments": (_i32, [_vp, _vp, _vp]),
    "phant_block_receipt_segments_dev": (_i32, [_vp, _vp, _vp]),
    "phant_receipts_decode_rlp": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp]),
    "phant_block_requests": (_i32, [_vp, _vp, _vp]),
    "phant_block_requests_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_log_filters": (_i32, [_vp, _vp, _vp, _vp]),
    "phant_block_log_filters_dev": (_i32, [_vp, _vp, _vp, _vp]),
    "phant_log_filters_bloom": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "phant_log_filters_bloom_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp]),
    "phant_block_fee_history": (_i32, [_vp, _vp, _vp]),
    "phant_block_fee_history_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_txs_prestate": (_i32, [_vp, _vp, _vp]),
    "phant_block_txs_prestate_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_settle": (_i32, [_vp, _vp, _vp]),
    "phant_block_settle_dev": (_i32, [_vp, _vp, _vp]),
    "phant_mpt_verify_ranges": (_i32, [_vp, _vp, _vp]),
    "phant_mpt_verify_ranges_dev": (_i32, [_vp, _vp, _vp]),
    "phant_block_access_lists": (_i32, [_vp, _vp, _vp]),
    "phant_block_access_lists_dev": (_i32, [_vp, _vp, _vp]),
    "phant_diag_secp_op": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp]),
    "phant_diag_scan_u32": (_i32, [_vp, _vp, _u32]),
    "phant_diag_sort_pairs": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    "phant_diag_order_digests": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "phant_mpt_verify_batch": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp]),
    "phant_mpt_verify_batch_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _u32, _vp,
                                          _vp, _vp]),
    "phant_mpt_verify_verdict_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _u32, _vp,
                                            _vp, _vp, _vp]),
    "phant_mpt_verdict_dev": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp]),
    "phant_mpt_verify_nodeset": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp]),
    "phant_mpt_verify_nodeset_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp]),
    "phant_mpt_verify_nodeset_verdict_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp,
                                                    _vp]),
    "phant_mpt_verify_nodeset_submit": (_i32, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _u32, _vp, _vp,
                                               _vp]),
    "phant_host_alloc": (_i32, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "phant_host_free": (_i32, [_vp, _vp]),
    "phant_mpt_verify_submit": (_i32, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp]),
    "phant_wait": (_i32, [_vp, _u32]),
    "phant_witness_parse_json": (_i32, [C.c_char_p, _u64, C.POINTER(_vp), C.c_char_p, _u32]),
    "phant_witness_parse_json_mt": (_i32, [C.c_char_p, _u64, _u32, C.POINTER(_vp), C.c_char_p, _u32]),
    "phant_witness_index_json": (_i32, [C.c_char_p, _u64, _u32, C.POINTER(_vp), C.c_char_p, _u32]),
    "phant_witness_free": (None, [_vp]),
    "phant_witness_get": (_i32, [_vp, _vp]),
    "phant_witness_verify": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "phant_witness_to_json": (_i32, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "phant_exec_witness_parse_json": (_i32, [C.c_char_p, _u64, C.POINTER(_vp), C.c_char_p, _u32]),
    "phant_exec_witness_free": (None, [_vp]),
    "phant_exec_witness_get": (_i32, [_vp, _vp]),
    "phant_exec_witness_prestate": (_i32, [_vp, _vp, _vp, _vp]),
    "phant_exec_witness_poststate": (_i32, [_vp, _vp, _vp, _vp]),
    "phant_exec_witness_advance": (_i32, [_vp, _vp, _vp, _vp, _u32, C.POINTER(_vp)]),
    "phant_mpt_root": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "phant_mpt_root_nodes": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp]),
    "phant_mpt_prove_nodeset": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp]),
    "phant_mpt_prove_nodeset_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _vp, _u32, _vp]),
    "phant_mpt_prove_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "phant_mpt_prove_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _u32, _vp]),
    "phant_mpt_strip_first_nibble": (_i32, [_vp, _u32, _vp, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "phant_index_root_rlp": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_block_roots": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "phant_index_root_be32": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "phant_state_root": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "phant_state_witness": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, C.POINTER(_vp), _vp]),
    "phant_state_proofs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, C.POINTER(_vp), _vp]),
    "phant_state_trie_leaves": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp]),
    "phant_state_root_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _vp]),
    "phant_state_subtrie_nodes": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "phant_timing": (_i32, [_vp, _i32]),
    "phant_last_kernel_ms": (_i32, [_vp, C.POINTER(C.c_float)]),
    "phant_keccak_rate": (_i32, [_vp, _u32, _u32, C.POINTER(C.c_double)]),
    "phant_nodeset_tune": (_i32, [_vp, _i32, _u32, _u32, _u32]),
    "phant_diag_set": (_i32, [_vp, _u32, C.c_int64]),
    "phant_verify_kernel_ms": (_i32, [_vp, C.POINTER(C.c_float * 5)]),
    "phant_verify_form": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "phant_verify_bound_experiment": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _u32,
                                            C.POINTER(C.c_float * 3)]),
    "phant_verify_stats": (_i32, [_vp, C.POINTER(C.c_uint32 * 8)]),
    "phant_verify_path_stats": (_i32, [_vp, C.POINTER(C.c_uint32 * 2)]),
    "phant_verify_tier_stats": (_i32, [_vp, C.POINTER(C.c_uint32 * 5)]),
    "phant_trie_stats": (_i32, [_vp, C.POINTER(C.c_uint32 * 16)]),
    "phant_nodeset_stats": (_i32, [_vp, C.POINTER(C.c_uint32 * 14)]),
    "phant_mpt_root_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp]),
    "phant_comm_create": (_i32, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "phant_comm_destroy": (None, [_vp]),
    "phant_comm_size": (_u32, [_vp]),
    "phant_comm_ctx": (_vp, [_vp, _u32]),
    "phant_comm_last_error": (C.c_char_p, [_vp]),
    "phant_comm_owner": (_u32, [_vp, _vp, _u32]),
    "phant_mpt_verify_sharded": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "phant_mpt_verify_nodeset_sharded": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _vp, _vp,
                                                _vp]),
    "phant_mpt_root_sharded": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "phant_state_root_sharded": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "phant_comm_allreduce_verdict": (_i32, [_vp, _vp, _u32]),
}


class PhantOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p), ("flags", C.c_uint32)]


class PhantReceiptsIn(C.Structure):
    """phant_receipts_in (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_receipts", C.c_uint32), ("n_logs", C.c_uint32), ("n_topics", C.c_uint32),
                ("data_bytes", C.c_uint64), ("tx_type", C.c_void_p), ("status", C.c_void_p), ("cum_gas", C.c_void_p),
                ("log_first", C.c_void_p), ("address", C.c_void_p), ("topic_first", C.c_void_p), ("data_off", C.c_void_p),
                ("topics", C.c_void_p), ("data", C.c_void_p), ("lists", C.c_void_p), ("list_off", C.c_void_p),
                ("list_n", C.c_void_p), ("list_bytes", C.c_void_p), ("n_lists", C.c_uint32), ("receipts_at", C.c_uint32)]


class PhantReceiptsOut(C.Structure):
    """phant_receipts_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("encoded_off_cap", C.c_uint32), ("encoded_cap", C.c_uint64),
                ("receipts_root", C.c_void_p), ("logs_bloom", C.c_void_p), ("blooms", C.c_void_p), ("encoded", C.c_void_p),
                ("encoded_off", C.c_void_p), ("roots_out", C.c_void_p), ("encoded_len", C.c_uint64)]


HEADER_ARRAYS = ("parent_hash", "uncle_hash", "fee_recipient", "state_root", "transactions_root", "receipts_root", "logs_bloom", "difficulty",
                 "number", "gas_limit", "gas_used", "timestamp", "extra_data", "extra_off", "prev_randao", "nonce", "base_fee",
                 "withdrawals_root", "blob_gas_used", "excess_blob_gas", "parent_beacon_root", "requests_hash", "n_fields", "seg_first",
                 "expected_hash")
HEADERS_FROM_BLOCKS = 1


class PhantHeadersIn(C.Structure):
    """phant_headers_in (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_uint32), ("n_segs", C.c_uint32), ("reserved", C.c_uint32)] + \
               [(name, C.c_void_p) for name in HEADER_ARRAYS]


class PhantHeadersOut(C.Structure):
    """phant_headers_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("first_bad", C.c_uint32), ("enc_cap", C.c_uint64), ("hashes", C.c_void_p),
                ("flags", C.c_void_p), ("enc", C.c_void_p), ("enc_off", C.c_void_p), ("enc_len", C.c_uint64)]


TXS_HAVE_GAS_LIMIT, TXS_NO_RECOVERY = 1, 2
# phant_txs_out's arrays in the struct's order: (name, numpy dtype, elements per transaction)
TX_OUTPUTS = (("tx_hash", "u1", 32), ("sig_hash", "u1", 32), ("sender", "u1", 20), ("sig_status", "u1", 1), ("sig", "u1", 65), ("type", "u1", 1),
              ("chain_id", "u8", 1), ("nonce", "u8", 1), ("gas_limit", "u8", 1), ("gas_price", "u1", 32), ("priority_fee", "u1", 32),
              ("value", "u1", 32), ("to", "u1", 20), ("data_off", "u8", 1), ("data_len", "u4", 1), ("al_off", "u8", 1), ("al_len", "u4", 1),
              ("al_addresses", "u4", 1), ("al_keys", "u4", 1), ("intrinsic_gas", "u8", 1), ("effective_gas_price", "u1", 32),
              ("upfront_cost", "u1", 32), ("flags", "u4", 1))
# PHANT_TX_*: bit k of flags[i]; every bit below IsCreate is an error
TX_FLAG_NAMES = ("Undecodable", "BadV", "Signature", "ChainId", "PriorityAboveMax", "FeeBelowBase", "GasAboveBlock", "IntrinsicGas", "NonceMax",
                 "InitcodeSize", "CostOverflow", "IsCreate")
TX_ERROR_BITS = 0x7FF


class PhantTxsIn(C.Structure):
    """phant_txs_in (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("txs", C.c_void_p),
                ("tx_off", C.c_void_p), ("tx_bytes", C.c_uint64), ("chain_id", C.c_uint64), ("base_fee", C.c_void_p),
                ("block_gas_limit", C.c_uint64)]


class PhantTxsOut(C.Structure):
    """phant_txs_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("first_bad", C.c_uint32)] + [(name, C.c_void_p) for name, _, _ in TX_OUTPUTS]


TXS_FORK_LONDON, TXS_FORK_CANCUN, TXS_FORK_PRAGUE = 0, 1, 2
AUTH_CHAIN_ID, AUTH_NONCE_MAX = 8, 9  # auth_status, beside SIG_*
# phant_txs_ex_out's arrays in the struct's order: a row per transaction (auth_first: n + 1 entries) ...
TX_EX_OUTPUTS = (("max_fee_per_blob_gas", "u1", 32), ("blob_off", "u8", 1), ("blobs", "u4", 1), ("auth_first", "u4", 1), ("floor_gas", "u8", 1))
# ... and a row per authorization tuple
TX_AUTH_OUTPUTS = (("auth_chain_id", "u1", 32), ("auth_address", "u1", 20), ("auth_nonce", "u8", 1), ("auth_hash", "u1", 32), ("auth_sig", "u1", 65),
                   ("authority", "u1", 20), ("auth_status", "u1", 1))
# PHANT_TX_* of phant_block_transactions_ex: bit k of flags[i] (bits 12 .. 18 are errors too)
TX_FLAG_NAMES_EX = TX_FLAG_NAMES + ("NoTo", "BlobNone", "BlobVersion", "BlobFeeBelowBase", "AuthNone", "FloorGas")
TX_ERROR_BITS_EX = 0x7FF | 0x7F000


def tx_error_bits(fork=None):
    """the error bits of a call's flags: fork None = phant_block_transactions"""
    return TX_ERROR_BITS if fork is None else TX_ERROR_BITS_EX


class PhantTxsExIn(C.Structure):
    """phant_txs_ex_in (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("fork", C.c_uint32), ("base", PhantTxsIn), ("blob_base_fee", C.c_void_p), ("auth_cap", C.c_uint32),
                ("reserved", C.c_uint32)]


class PhantTxsExOut(C.Structure):
    """phant_txs_ex_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_auth", C.c_uint32), ("blob_gas_used", C.c_uint64), ("base", PhantTxsOut)] + \
               [(name, C.c_void_p) for name, _, _ in TX_EX_OUTPUTS + TX_AUTH_OUTPUTS]


BODY_TX, BODY_TXS_ROOT, BODY_WD_ROOT, BODY_BLOB_GAS = 1, 2, 4, 8
BODY_FLAG_NAMES = ("Transaction", "TransactionsRoot", "WithdrawalsRoot", "BlobGasUsed")
# phant_bodies_in's arrays in the struct's order (tx_bytes sits behind tx_off, wd_bytes behind wd_off)
BODIES_INPUTS = ("txs", "tx_off", "block_first", "withdrawals", "wd_off", "wd_first", "base_fee", "gas_limit", "blob_base_fee", "transactions_root",
                 "withdrawals_root", "blob_gas_used")
# phant_bodies_out's own arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow)
BODIES_OUTPUTS = (("tx_block", "u4", 1, "n"), ("block_first_bad", "u4", 1, "n_blocks"), ("block_blob_gas_used", "u8", 1, "n_blocks"),
                  ("transactions_root", "u1", 32, "n_blocks"), ("withdrawals_root", "u1", 32, "n_blocks"), ("block_flags", "u4", 1, "n_blocks"))


BODIES_NO_HEADER = 1
# phant_bodies_split's arrays in the struct's order
BODIES_SPLIT_ARRAYS = ("txs", "tx_off", "block_first", "withdrawals", "wd_off", "wd_first")


class PhantBodiesSplit(C.Structure):
    """phant_bodies_split (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "reserved", "tx_cap", "wd_cap")] + [("tx_bytes_cap", C.c_uint64), ("wd_bytes_cap", C.c_uint64)] + \
               [(name, C.c_void_p) for name in BODIES_SPLIT_ARRAYS] + [("n", C.c_uint32), ("n_wd", C.c_uint32), ("tx_bytes", C.c_uint64), ("wd_bytes", C.c_uint64)]


class PhantBodiesIn(C.Structure):
    """phant_bodies_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "fork", "flags", "n_blocks", "n", "n_wd", "auth_cap", "reserved")] + \
               [("chain_id", C.c_uint64), ("txs", C.c_void_p), ("tx_off", C.c_void_p), ("tx_bytes", C.c_uint64), ("block_first", C.c_void_p),
                ("withdrawals", C.c_void_p), ("wd_off", C.c_void_p), ("wd_bytes", C.c_uint64)] + \
               [(name, C.c_void_p) for name in BODIES_INPUTS[5:]]


class PhantBodiesOut(C.Structure):
    """phant_bodies_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("first_bad_block", C.c_uint32), ("txs", PhantTxsExOut)] + \
               [(name, C.c_void_p) for name, _, _, _ in BODIES_OUTPUTS]


RCPTS_CONSENSUS, RCPTS_ETH69 = 0, 1
RCPT_UNDECODABLE, RCPT_BLOOM, RCPT_GAS_ORDER, RCPT_POST_STATE, RCPT_ERROR_BITS = 1, 2, 4, 0x100, 7
RCPT_FLAG_NAMES = ("Undecodable", "Bloom", "GasOrder", None, None, None, None, None, "PostState")
RBLOCK_RECEIPT, RBLOCK_ROOT, RBLOCK_BLOOM, RBLOCK_GAS_USED, RBLOCK_COUNT = 1, 2, 4, 8, 16
RBLOCK_FLAG_NAMES = ("Receipt", "ReceiptsRoot", "LogsBloom", "GasUsed", "Count")
# phant_rcpt_segs_in's arrays in the struct's order (rc_bytes sits behind rc_off)
RSEG_INPUTS = ("receipts", "rc_off", "block_first", "receipts_root", "logs_bloom", "gas_used", "tx_count")
# phant_rcpt_segs_out's arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow, rows beyond that count)
RSEG_OUTPUTS = (("tx_type", "u1", 1, "n", 0), ("status", "u1", 1, "n", 0), ("cum_gas", "u8", 1, "n", 0), ("gas_used", "u8", 1, "n", 0),
                ("log_first", "u4", 1, "n", 1), ("bloom", "u1", 256, "n", 0), ("flags", "u4", 1, "n", 0),
                ("log_receipt", "u4", 1, "n_logs", 0), ("address", "u1", 20, "n_logs", 0), ("topic_first", "u4", 1, "n_logs", 1),
                ("topics", "u1", 32, "n_topics", 0), ("data_at", "u8", 1, "n_logs", 0), ("data_len", "u4", 1, "n_logs", 0),
                ("encoded", "u1", 1, "encoded_len", 0), ("encoded_off", "u8", 1, "n", 1),
                ("receipts_root", "u1", 32, "n_blocks", 0), ("logs_bloom", "u1", 256, "n_blocks", 0), ("block_gas_used", "u8", 1, "n_blocks", 0),
                ("block_first_bad", "u4", 1, "n_blocks", 0), ("block_flags", "u4", 1, "n_blocks", 0))
RCPTS_SPLIT_ETH69 = 1
SPLIT_BAD_RECEIPT = 5


class PhantRcptSegsIn(C.Structure):
    """phant_rcpt_segs_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "form", "n_blocks", "n", "log_cap", "topic_cap")] + [("reserved", C.c_uint32 * 2)] + \
               [("receipts", C.c_void_p), ("rc_off", C.c_void_p), ("rc_bytes", C.c_uint64)] + [(name, C.c_void_p) for name in RSEG_INPUTS[2:]]


class PhantRcptSegsOut(C.Structure):
    """phant_rcpt_segs_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "first_bad_block", "n_logs", "n_topics")] + \
               [("encoded_cap", C.c_uint64), ("encoded_len", C.c_uint64)] + [(name, C.c_void_p) for name, _, _, _, _ in RSEG_OUTPUTS]


class PhantReceiptsSplit(C.Structure):
    """phant_receipts_split (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "reserved", "rc_cap", "n")] + [("rc_bytes_cap", C.c_uint64)] + \
               [(name, C.c_void_p) for name in ("receipts", "rc_off", "block_first")] + [("rc_bytes", C.c_uint64)]


QBLOCK_DEPOSIT_LAYOUT, QBLOCK_ORDER, QBLOCK_HASH = 1, 2, 4
QBLOCK_FLAG_NAMES = ("DepositLayout", "RequestsOrder", "RequestsHash")
DEPOSIT_EVENT_TOPIC = bytes.fromhex("649bbc62d0e31342afea4e5cd82d4049e7e1ee912fc0889aa790803be39038c5")
EMPTY_REQUESTS_HASH = bytes.fromhex("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")
# phant_requests_in's arrays in the struct's order (rc_bytes sits behind receipts, req_total behind req_off): (name, numpy dtype)
REQUESTS_INPUTS = (("receipts", "u1"), ("block_first", "u4"), ("log_first", "u4"), ("address", "u1"), ("topic_first", "u4"), ("topics", "u1"), ("data_at", "u8"),
                   ("data_len", "u4"), ("req_block_first", "u4"), ("req_type", "u1"), ("req_bytes", "u1"), ("req_off", "u8"), ("active", "u1"), ("requests_hash", "u1"))
# phant_requests_out's arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow, rows beyond that count)
REQUESTS_OUTPUTS = (("deposit_log", "u4", 1, "n_deposits", 0), ("deposit", "u1", 192, "n_deposits", 0), ("deposit_first", "u4", 1, "n_blocks", 1),
                    ("requests_hash", "u1", 32, "n_blocks", 0), ("block_flags", "u4", 1, "n_blocks", 0))


class PhantRequestsIn(C.Structure):
    """phant_requests_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_blocks", "n", "n_logs", "n_topics", "n_req", "deposit_cap", "reserved")] + \
               [("receipts", C.c_void_p), ("rc_bytes", C.c_uint64)] + [(name, C.c_void_p) for name, _ in REQUESTS_INPUTS[1:12]] + \
               [("req_total", C.c_uint64), ("active", C.c_void_p), ("requests_hash", C.c_void_p), ("deposit_contract", C.c_uint8 * 20)]


class PhantRequestsOut(C.Structure):
    """phant_requests_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_deposits", "first_bad_block", "reserved")] + \
               [(name, C.c_void_p) for name, _, _, _, _ in REQUESTS_OUTPUTS]


LOGFILTER_LINEAR_MAX = 16  # PHANT_LOGFILTER_LINEAR_MAX (include/phant_gpu_diag.h)
# phant_log_filters' arrays in the struct's order: (name, numpy dtype)
LOG_FILTER_ARRAYS = (("addr_first", "u4"), ("addr", "u1"), ("topic_first", "u4"), ("topic", "u1"), ("block_lo", "u4"), ("block_hi", "u4"))
# phant_logmatch_in's arrays and phant_logmatch_out's in their structs' order
LOGMATCH_INPUTS = (("block_first", "u4"), ("log_first", "u4"), ("address", "u1"), ("topic_first", "u4"), ("topics", "u1"))
LOGMATCH_OUTPUTS = ("filter_first", "match_log", "filter_count")


class PhantLogFilters(C.Structure):
    """phant_log_filters (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_filters", "n_addr", "n_topic")] + \
               [(name, C.c_void_p) for name, _ in LOG_FILTER_ARRAYS] + [("reserved", C.c_uint64)]


class PhantLogMatchIn(C.Structure):
    """phant_logmatch_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_blocks", "n", "n_logs", "n_topics", "match_cap", "reserved", "reserved2")] + \
               [(name, C.c_void_p) for name, _ in LOGMATCH_INPUTS]


class PhantLogMatchOut(C.Structure):
    """phant_logmatch_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_matches", "reserved", "reserved2")] + [(name, C.c_void_p) for name in LOGMATCH_OUTPUTS]


FEE_BELOW_BASE = 1            # PHANT_FEE_BELOW_BASE (block_flags of phant_block_fee_history)
FEEHIST_BLOCK_MAX = 65536     # PHANT_FEEHIST_BLOCK_MAX
# phant_fee_history_in's arrays and phant_fee_history_out's in their structs' order: (name, numpy dtype, elements per row)
FEEHIST_INPUTS = (("block_first", "u4", 1), ("price", "u1", 32), ("base_fee", "u1", 32), ("gas_used", "u8", 1), ("percentile", "u4", 1))
FEEHIST_OUTPUTS = (("reward", "u1", 32), ("tip", "u1", 32), ("order", "u4", 1), ("block_gas_used", "u8", 1), ("block_flags", "u4", 1))


class PhantFeeHistoryIn(C.Structure):
    """phant_fee_history_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_blocks", "n", "n_percentiles")] + \
               [(name, C.c_void_p) for name, _, _ in FEEHIST_INPUTS] + [("reserved", C.c_uint64)]


class PhantFeeHistoryOut(C.Structure):
    """phant_fee_history_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "first_bad_block")] + [(name, C.c_void_p) for name, _, _ in FEEHIST_OUTPUTS] + \
               [("reserved", C.c_uint64)]


ROW_NONE = 0xFFFFFFFF
# phant_txstate_in's arrays in the struct's order (code_bytes sits between codes and probe)
TXSTATE_INPUTS = ("sender", "sig_status", "tx_flags", "nonce", "upfront_cost", "to", "auth_first", "authority", "auth_status", "addresses",
                  "account_status", "nonces", "balances", "code_hashes", "code_index", "code_off", "codes")
# phant_txstate_out's arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow)
TXSTATE_OUTPUTS = (("sender_row", "u4", 1, "n"), ("to_row", "u4", 1, "n"), ("expected_nonce", "u8", 1, "n"), ("spent_before", "u1", 32, "n"),
                   ("state_flags", "u4", 1, "n"), ("sends", "u4", 1, "n_accounts"), ("roles", "u1", 1, "n_accounts"), ("probe_row", "u4", 1, "n_probe"))
# PHANT_TXST_*: bit k of state_flags[i]; the bits below 0x80 are errors
TXST_FLAG_NAMES = ("SenderUnknown", "ToUnknown", "NonceLow", "NonceHigh", "BalanceShort", "NotEOA", "CodeMissing", None, "Skipped", "Undetermined",
                   "NeedsInflow", "SpentSaturated")
TXST_ERROR_BITS = 0x7F
TXST_SKIPPED, TXST_UNDETERMINED, TXST_NEEDS_INFLOW, TXST_SPENT_SATURATED = 0x100, 0x200, 0x400, 0x800
ROLE_SENDER, ROLE_RECIPIENT, ROLE_AUTHORITY, ROLE_PROBE = 1, 2, 4, 8


class PhantTxstateIn(C.Structure):
    """phant_txstate_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "fork", "n", "n_auth", "n_accounts", "n_codes", "n_probe", "reserved")] + \
               [(name, C.c_void_p) for name in TXSTATE_INPUTS] + [("code_bytes", C.c_uint64), ("probe", C.c_void_p)]


class PhantTxstateOut(C.Structure):
    """phant_txstate_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "first_bad", "n_undetermined", "reserved")] + \
               [(name, C.c_void_p) for name, _, _, _ in TXSTATE_OUTPUTS]


# phant_settle_in's arrays in the struct's order
SETTLE_INPUTS = ("base_fee", "type", "tx_flags", "gas_limit", "intrinsic_gas", "floor_gas", "value", "effective_gas_price", "upfront_cost", "to",
                 "sender_row", "to_row", "state_flags", "account_status", "nonces", "balances", "code_hashes", "wd_row", "wd_amount_gwei")
# phant_settle_out's arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow)
SETTLE_OUTPUTS = (("settle_flags", "u4", 1, "n"), ("cumulative_gas_used", "u8", 1, "n"), ("balance_before", "u1", 32, "n"),
                  ("account_op", "u1", 1, "n_accounts"), ("nonces_after", "u8", 1, "n_accounts"), ("balances_after", "u1", 32, "n_accounts"),
                  ("code_hashes_after", "u1", 32, "n_accounts"), ("account_flags", "u1", 1, "n_accounts"), ("wd_flags", "u1", 1, "n_wd"))
# PHANT_SETTLE_*: bit k of settle_flags[i]; the bits below 0x8 are errors
SETTLE_FLAG_NAMES = ("Upstream", "GasLimit", "BalanceShort", None, None, None, None, None, "NotPlain")
SETTLE_ERROR_BITS = 0x7
SETTLE_NOT_PLAIN = 0x100
SETTLE_COINBASE_UNKNOWN, SETTLE_WD_UNKNOWN, SETTLE_ACCT_OVERFLOW, SETTLE_ACCT_NEGATIVE = 1, 1, 1, 2


class PhantSettleIn(C.Structure):
    """phant_settle_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "fork", "n", "n_accounts", "n_wd", "coinbase_row")] + \
               [("reserved", C.c_uint32 * 2), ("block_gas_limit", C.c_uint64)] + [(name, C.c_void_p) for name in SETTLE_INPUTS]


class PhantSettleOut(C.Structure):
    """phant_settle_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "first_bad", "n_not_plain", "first_not_plain", "block_flags", "n_wd_unknown")] + \
               [("gas_used", C.c_uint64)] + [(name, C.c_void_p) for name, _, _, _ in SETTLE_OUTPUTS]


AL_MALFORMED, AL_DUPLICATES = 1, 2
# phant_access_out's arrays in the struct's order: (name, numpy dtype, elements per row, the count its rows follow, rows beyond that count)
ACCESS_OUTPUTS = (("tuple_first", "u4", 1, "n", 1), ("al_flags", "u4", 1, "n", 0), ("warm_addresses", "u4", 1, "n", 0), ("warm_keys", "u4", 1, "n", 0),
                  ("address", "u1", 20, "n_tuples", 0), ("key_first", "u4", 1, "n_tuples", 1), ("account_row", "u4", 1, "n_tuples", 0),
                  ("tuple_same", "u4", 1, "n_tuples", 0), ("key", "u1", 32, "n_keys", 0), ("slot_row", "u4", 1, "n_keys", 0), ("key_same", "u4", 1, "n_keys", 0))


class PhantAccessIn(C.Structure):
    """phant_access_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n", "n_accounts", "n_slots")] + \
               [("txs", C.c_void_p), ("tx_bytes", C.c_uint64), ("al_off", C.c_void_p), ("al_len", C.c_void_p), ("addresses", C.c_void_p),
                ("slot_first", C.c_void_p), ("slots", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class PhantAccessOut(C.Structure):
    """phant_access_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_tuples", "n_keys", "n_missing_accounts", "n_missing_slots", "first_malformed",
                                                "tuple_cap", "key_cap")] + [(name, C.c_void_p) for name, _, _, _, _ in ACCESS_OUTPUTS]


# phant_ranges_in's arrays in the struct's order
RANGES_INPUTS = ("roots", "origins", "leaf_first", "has_proof", "keys", "vals", "val_off", "nodes", "node_off")
# phant_ranges_out's arrays in the struct's order: (name, numpy dtype, elements per range)
RANGES_OUTPUTS = (("status", "u1", 1), ("has_more", "u1", 1), ("computed_root", "u1", 32), ("bad_leaf", "u4", 1))


class PhantRangesIn(C.Structure):
    """phant_ranges_in (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_ranges", "n_leaves", "n_nodes")] + \
               [("reserved", C.c_uint32 * 2), ("vals_len", C.c_uint64), ("nodes_len", C.c_uint64)] + [(name, C.c_void_p) for name in RANGES_INPUTS]


class PhantRangesOut(C.Structure):
    """phant_ranges_out (include/phant_gpu.h)"""
    _fields_ = [(name, C.c_uint32) for name in ("struct_size", "n_failed", "first_failed")] + [("reserved", C.c_uint32 * 2)] + \
               [(name, C.c_void_p) for name, _, _ in RANGES_OUTPUTS]


class PhantProveOut(C.Structure):
    """phant_prove_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("max_nodes", C.c_uint32), ("nodes_cap", C.c_uint64), ("nodes", C.c_void_p),
                ("node_off", C.c_void_p), ("trie_first_node", C.c_void_p), ("roots", C.c_void_p), ("q_status", C.c_void_p),
                ("nodes_len", C.c_uint64), ("total_nodes", C.c_uint32), ("reserved", C.c_uint32)]


class PhantProveBatchOut(C.Structure):
    """phant_prove_batch_out (include/phant_gpu.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("max_nodes", C.c_uint32), ("nodes_cap", C.c_uint64), ("nodes", C.c_void_p),
                ("node_off", C.c_void_p), ("proof_first_node", C.c_void_p), ("roots", C.c_void_p), ("q_status", C.c_void_p),
                ("nodes_len", C.c_uint64), ("total_nodes", C.c_uint32), ("reserved", C.c_uint32)]


class PhantError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libphant_gpu error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libphant_gpu.so (no CPU fallback: raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP library first (python -m phant_amd.build). "
                "phant_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib
