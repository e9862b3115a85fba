"""Block headers <-> src/types/block.zig:15-69 (`BlockHeader`, `encodeToRLP`) and src/blockchain/blockchain.zig:100-145
(`validateBlockHeader`): encodings, hashes and the header rules of whole chain segments in ONE call (phant_header_chain), strict
decoding of raw headers on the host (phant_headers_decode_rlp).  And the bodies those headers commit to, for whole segments in ONE call
as well (phant_block_bodies; raw blocks split on the host by phant_bodies_decode_rlp): `split_blocks`, `block_bodies`,
`validate_segment`.  Through the C-ABI; no CPU fallback.

Two deviations from the reference, both where it would panic: a header pair of which exactly one has a base fee, and a parent
whose gas target is zero while it used gas, set the InvalidBaseFee flag instead."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields as _dc_fields

import numpy as np

from .. import _lib as L
from ..context import Context, default_context

EMPTY_UNCLE_HASH = bytes.fromhex("1dcc4de8dec75d7aab85b567b6ccd41ad312451b948a7413f0a142fd40d49347")  # block.zig:13


class Flags:
    """flags[i] of validate_chain: bit k = the k-th check of validateBlockHeader failed"""
    GasLimitTooHigh = 1 << 0
    GasLimitTooLow = 1 << 1
    GasLimitLessThanMinimum = 1 << 2
    GasLimitExceeded = 1 << 3
    InvalidBaseFee = 1 << 4
    InvalidTimestamp = 1 << 5
    InvalidBlockNumber = 1 << 6
    ExtraDataTooLong = 1 << 7
    InvalidDifficulty = 1 << 8
    InvalidNonce = 1 << 9
    InvalidUnclesHash = 1 << 10
    InvalidParentHash = 1 << 11
    ExpectedHashMismatch = 1 << 12  # not one of the reference's: the caller's expected hash (a payload's blockHash) differs
    NAMES = ("GasLimitTooHigh", "GasLimitTooLow", "GasLimitLessThanMinimum", "GasLimitExceeded", "InvalidBaseFee", "InvalidTimestamp",
             "InvalidBlockNumber", "ExtraDataTooLong", "InvalidDifficulty", "InvalidNonce", "InvalidUnclesHash", "InvalidParentHash",
             "ExpectedHashMismatch")


def first_error(flags: int):
    """the error validateBlockHeader would return for this flag word (its lowest set bit), or None"""
    flags = int(flags)
    return None if not flags else Flags.NAMES[(flags & -flags).bit_length() - 1]


@dataclass
class BlockHeader:
    """block.zig:15-36 `BlockHeader`"""
    parent_hash: bytes
    uncle_hash: bytes
    fee_recipient: bytes
    state_root: bytes
    transactions_root: bytes
    receipts_root: bytes
    logs_bloom: bytes
    difficulty: int
    block_number: int
    gas_limit: int
    gas_used: int
    timestamp: int
    extra_data: bytes
    prev_randao: bytes
    nonce: bytes
    base_fee_per_gas: int | None = None
    withdrawals_root: bytes | None = None
    blob_gas_used: int | None = None
    excess_blob_gas: int | None = None
    parent_beacon_root: bytes | None = None
    request_hash: bytes | None = None

    @property
    def n_fields(self) -> int:
        """block.zig:51-68: the last field that is set decides how many items are encoded"""
        if self.request_hash is not None:
            n = 21
        elif self.parent_beacon_root is not None:
            n = 20
        elif self.blob_gas_used is not None or self.excess_blob_gas is not None:
            n = 19
        elif self.withdrawals_root is not None:
            n = 17
        elif self.base_fee_per_gas is not None:
            n = 16
        else:
            n = 15
        if any(getattr(self, f.name) is None for f in _dc_fields(self)[:n]):
            raise ValueError("a field in front of the header's last one is None")
        return n

    def encode(self, ctx: Context | None = None) -> bytes:
        """block.zig:51 `encodeToRLP`"""
        return header_chain([self], want_encodings=True, ctx=ctx).encoded[0]

    def hash(self, ctx: Context | None = None) -> bytes:
        """common.encodeToRLPAndHash(BlockHeader, ...)"""
        return header_chain([self], ctx=ctx).hashes[0]

    @classmethod
    def decode(cls, raw: bytes) -> "BlockHeader":
        """strict; ValueError for anything encode() would not have produced"""
        return decode_headers([raw])[0]


_ROWS = (("parent_hash", 32), ("uncle_hash", 32), ("fee_recipient", 20), ("state_root", 32), ("transactions_root", 32), ("receipts_root", 32),
         ("logs_bloom", 256), ("prev_randao", 32), ("nonce", 8), ("withdrawals_root", 32), ("parent_beacon_root", 32), ("requests_hash", 32))
_INTS = ("difficulty", "number", "gas_limit", "gas_used", "timestamp", "blob_gas_used", "excess_blob_gas")
_ATTR = {"number": "block_number", "requests_hash": "request_hash"}  # C-ABI array -> the reference's field name


def _empty_arrays(n, extra_bytes):
    m = max(n, 1)
    a = {name: np.zeros((m, w), np.uint8) for name, w in _ROWS}
    a.update({name: np.zeros(m, np.uint64) for name in _INTS})
    a["base_fee"] = np.zeros((m, 32), np.uint8)
    a["extra_data"] = np.zeros(max(extra_bytes, 1), np.uint8)
    a["extra_off"] = np.zeros(n + 1, np.uint32)
    a["n_fields"] = np.zeros(m, np.uint8)
    return a


def pack_headers(headers):
    """-> the struct-of-arrays of phant_headers_in as numpy arrays (never empty: a zero count gets one spare element)"""
    headers = list(headers)
    n = len(headers)
    a = _empty_arrays(n, sum(len(h.extra_data) for h in headers))
    at = 0
    for i, h in enumerate(headers):
        a["n_fields"][i] = h.n_fields
        for name, w in _ROWS:
            v = getattr(h, _ATTR.get(name, name))
            if v is not None:
                if len(v) != w:
                    raise ValueError(f"{name} is {w} bytes")
                a[name][i] = np.frombuffer(bytes(v), np.uint8)
        for name in _INTS:
            v = getattr(h, _ATTR.get(name, name))
            if v is not None:
                if not 0 <= v < 1 << 64:
                    raise ValueError(f"{name} does not fit 64 bits")
                a[name][i] = v
        if h.base_fee_per_gas is not None:
            a["base_fee"][i] = np.frombuffer(int(h.base_fee_per_gas).to_bytes(32, "big"), np.uint8)
        x = bytes(h.extra_data)
        a["extra_data"][at:at + len(x)] = np.frombuffer(x, np.uint8)
        at += len(x)
        a["extra_off"][i + 1] = at
    return a


def _struct(a, n, seg_first=None, expected=None):
    ptr = {k: v.ctypes.data for k, v in a.items()}
    return L.PhantHeadersIn(C.sizeof(L.PhantHeadersIn), n, 0 if seg_first is None else len(seg_first) - 1, 0,
                            *[ptr.get(k) for k in L.HEADER_ARRAYS[:-2]], None if seg_first is None else seg_first.ctypes.data,
                            None if expected is None else expected.ctypes.data)


@dataclass
class HeaderChain:
    hashes: list          # n 32-byte hashes
    flags: np.ndarray     # n uint32 (Flags)
    first_bad: int        # the least index with a flag, n if none
    encoded: list | None  # n byte strings where asked for


def header_chain(headers, seg_first=None, expected_hashes=None, want_encodings=False, ctx: Context | None = None, arrays=None) -> HeaderChain:
    """phant_header_chain over BlockHeader objects (or over `arrays` as pack_headers / decode_arrays made them)."""
    ctx = ctx or default_context()
    a = pack_headers(headers) if arrays is None else arrays
    n = len(a["extra_off"]) - 1
    seg = None if seg_first is None else np.asarray(seg_first, np.uint32)
    exp = None
    if expected_hashes is not None:
        exp = np.frombuffer(b"".join(bytes(x) for x in expected_hashes) or bytes(32), np.uint8).copy()
        if exp.size != 32 * max(n, 1):
            raise ValueError("one 32-byte expected hash per header")
    arg = _struct(a, n, seg, exp)
    hashes = np.zeros((max(n, 1), 32), np.uint8)
    flags = np.zeros(max(n, 1), np.uint32)
    cap = (700 * n + int(a["extra_off"][-1]) + 16) if want_encodings else 0
    enc = np.zeros(max(cap, 1), np.uint8)
    enc_off = np.zeros(n + 1, np.uint64)
    out = L.PhantHeadersOut(C.sizeof(L.PhantHeadersOut), 0, cap, hashes.ctypes.data, flags.ctypes.data,
                            enc.ctypes.data if want_encodings else None, enc_off.ctypes.data if want_encodings else None, 0)
    ctx.check(ctx._lib.phant_header_chain(ctx.handle, C.byref(arg), C.byref(out)))
    if want_encodings and out.enc_len > cap:
        raise RuntimeError("header_chain: the encodings exceed their bound (internal)")
    encoded = [enc[int(enc_off[i]):int(enc_off[i + 1])].tobytes() for i in range(n)] if want_encodings else None
    return HeaderChain([hashes[i].tobytes() for i in range(n)], flags[:n], int(out.first_bad), encoded)


def validate_chain(headers, seg_first=None, expected_hashes=None, ctx: Context | None = None):
    """validateBlockHeader of every header against the one before it, for whole segments: seg_first (None: one segment) are the
    n_segs + 1 increasing indices of the segments' first headers, from 0 to n; the first header of a segment is the trusted
    prev_block and only hashed.  expected_hashes: one per header, compared with its hash.  -> (hashes, flags, first_bad)"""
    r = header_chain(headers, seg_first, expected_hashes, ctx=ctx)
    return r.hashes, r.flags, r.first_bad


def decode_arrays(raws, from_blocks=False):
    """phant_headers_decode_rlp -> (arrays as pack_headers makes them, status uint8[n]); host only"""
    raws = [bytes(r) for r in raws]
    n = len(raws)
    blob = np.frombuffer(b"".join(raws) or b"\x00", np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in raws]).astype(np.uint64)
    a = _empty_arrays(n, int(off[-1]))
    status = np.zeros(max(n, 1), np.uint8)
    arg = _struct(a, n)
    rc = L.lib().phant_headers_decode_rlp(blob.ctypes.data, off.ctypes.data, n, L.HEADERS_FROM_BLOCKS if from_blocks else 0, C.byref(arg),
                                          status.ctypes.data)
    if rc != L.OK:
        raise L.PhantError(rc, "phant_headers_decode_rlp")
    return a, status[:n]


def unpack_headers(a):
    """arrays -> BlockHeader objects"""
    out = []
    for i in range(len(a["extra_off"]) - 1):
        k = int(a["n_fields"][i])
        row = lambda name: a[name][i].tobytes()  # noqa: E731
        out.append(BlockHeader(
            row("parent_hash"), row("uncle_hash"), row("fee_recipient"), row("state_root"), row("transactions_root"), row("receipts_root"),
            row("logs_bloom"), int(a["difficulty"][i]), int(a["number"][i]), int(a["gas_limit"][i]), int(a["gas_used"][i]), int(a["timestamp"][i]),
            a["extra_data"][int(a["extra_off"][i]):int(a["extra_off"][i + 1])].tobytes(), row("prev_randao"), row("nonce"),
            int.from_bytes(row("base_fee"), "big") if k >= 16 else None, row("withdrawals_root") if k >= 17 else None,
            int(a["blob_gas_used"][i]) if k >= 19 else None, int(a["excess_blob_gas"][i]) if k >= 19 else None,
            row("parent_beacon_root") if k >= 20 else None, row("requests_hash") if k >= 21 else None))
    return out


def decode_headers(raws, from_blocks=False):
    """strict decoding of raw headers (from_blocks: of the first item of raw blocks); ValueError names the first refused one"""
    a, status = decode_arrays(raws, from_blocks)
    if status.any():
        raise ValueError(f"header {int(np.flatnonzero(status)[0])} is not a canonical header encoding")
    return unpack_headers(a)


def payload_block_hash(payload_fields: dict, raw_txs, withdrawals, ctx: Context | None = None, keys: str = "be32"):
    """The check newPayloadV2Handler leaves out (execution_payload.zig:115,175-181): the header ExecutionPayload.toBlock builds
    (:125-166) from the payload's fields and the two roots it computes, hashed and compared with the payload's `blockHash`.
    payload_fields: parentHash, feeRecipient, stateRoot, receiptsRoot, logsBloom, prevRandao, blockNumber, gasLimit, gasUsed,
    timestamp, extraData, baseFeePerGas, blockHash (bytes / ints) and optionally blobGasUsed, excessBlobGas; raw_txs / withdrawals:
    the encoded items.  keys: "be32" = 32-byte big-endian index keys as toBlock has them, "rlp" = rlp(index) as a block's header
    commits to.  Two calls: the roots, then one header.  -> (matches, hash, header)"""
    from .. import mpt
    p = payload_fields
    if keys == "be32":
        tx_root, wd_root = mpt.index_root_be32(raw_txs, ctx), mpt.index_root_be32(withdrawals, ctx)
    elif keys == "rlp":
        tx_root, wd_root = mpt.block_roots([raw_txs, withdrawals], ctx)
    else:
        raise ValueError("keys is 'be32' or 'rlp'")
    blob = p.get("blobGasUsed")
    h = BlockHeader(bytes(p["parentHash"]), EMPTY_UNCLE_HASH, bytes(p["feeRecipient"]), bytes(p["stateRoot"]), tx_root, bytes(p["receiptsRoot"]),
                    bytes(p["logsBloom"]), 0, int(p["blockNumber"]), int(p["gasLimit"]), int(p["gasUsed"]), int(p["timestamp"]),
                    bytes(p["extraData"]), bytes(p["prevRandao"]), bytes(8), int(p["baseFeePerGas"]), wd_root,
                    None if blob is None else int(blob), None if blob is None else int(p["excessBlobGas"]))
    r = header_chain([h], expected_hashes=[bytes(p["blockHash"])], ctx=ctx)
    return r.first_bad == 1, r.hashes[0], h


# ---------------------------------------------------------------------------------------------------- bodies of chain segments
class BodyFlags:
    """block_flags[b] of block_bodies"""
    Transaction = L.BODY_TX
    TransactionsRoot = L.BODY_TXS_ROOT
    WithdrawalsRoot = L.BODY_WD_ROOT
    BlobGasUsed = L.BODY_BLOB_GAS
    NAMES = L.BODY_FLAG_NAMES


def _pack_lists(lists):
    """lists of byte strings -> (bytes back to back, n + 1 offsets, n_lists + 1 firsts); never empty arrays"""
    items = [bytes(x) for l in lists for x in l]
    blob = np.frombuffer(b"".join(items) or b"\x00", np.uint8).copy()
    off = np.cumsum([0] + [len(x) for x in items]).astype(np.uint64)
    first = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
    return blob, off, first


def pack_bodies(block_txs, block_withdrawals=None):
    """per block its raw transactions (and, from Shanghai on, its withdrawals, each its RLP list as it stands in the block) -> the packed
    arrays phant_block_bodies takes: txs, tx_off, block_first, withdrawals, wd_off, wd_first (the last three None without withdrawals)"""
    block_txs = [list(b) for b in block_txs]
    txs, tx_off, block_first = _pack_lists(block_txs)
    a = {"txs": txs, "tx_off": tx_off, "block_first": block_first, "withdrawals": None, "wd_off": None, "wd_first": None}
    if block_withdrawals is not None:
        block_withdrawals = [list(b) for b in block_withdrawals]
        if len(block_withdrawals) != len(block_txs):
            raise ValueError("one list of withdrawals per block")
        a["withdrawals"], a["wd_off"], a["wd_first"] = _pack_lists(block_withdrawals)
    return a


SPLIT_OK, SPLIT_BAD_RLP, SPLIT_BAD_TX, SPLIT_UNCLES, SPLIT_BAD_WITHDRAWAL = range(5)


def split_blocks(raws, bodies_only=False):
    """phant_bodies_decode_rlp: raw blocks [header, txs, uncles, withdrawals?] (bodies_only: [txs, uncles, withdrawals?]) -> (the packed
    arrays of pack_bodies, always with the withdrawals' three, status uint8[n]); a refused block (status != 0: SPLIT_*) has no rows.
    Host only."""
    raws = [bytes(r) for r in raws]
    n = len(raws)
    blob = np.frombuffer(b"".join(raws) or b"\x00", np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in raws]).astype(np.uint64)
    status = np.zeros(max(n, 1), np.uint8)
    flags = L.BODIES_NO_HEADER if bodies_only else 0
    arg = L.PhantBodiesSplit(C.sizeof(L.PhantBodiesSplit))
    fn = L.lib().phant_bodies_decode_rlp
    rc = fn(blob.ctypes.data, off.ctypes.data, n, flags, C.byref(arg), status.ctypes.data)  # the totals
    if rc != L.OK:
        raise L.PhantError(rc, "phant_bodies_decode_rlp")
    a = {"txs": np.zeros(max(int(arg.tx_bytes), 1), np.uint8), "tx_off": np.zeros(int(arg.n) + 1, np.uint64), "block_first": np.zeros(n + 1, np.uint32),
         "withdrawals": np.zeros(max(int(arg.wd_bytes), 1), np.uint8), "wd_off": np.zeros(int(arg.n_wd) + 1, np.uint64), "wd_first": np.zeros(n + 1, np.uint32)}
    arg.tx_cap, arg.wd_cap, arg.tx_bytes_cap, arg.wd_bytes_cap = int(arg.n), int(arg.n_wd), int(arg.tx_bytes), int(arg.wd_bytes)
    for k in L.BODIES_SPLIT_ARRAYS:
        setattr(arg, k, a[k].ctypes.data)
    rc = fn(blob.ctypes.data, off.ctypes.data, n, flags, C.byref(arg), status.ctypes.data)
    if rc != L.OK:
        raise L.PhantError(rc, "phant_bodies_decode_rlp")
    return a, status[:n]


class BlockBodies:
    """What phant_block_bodies answers: the per-transaction and per-authorization arrays of block_transactions(fork=) over the whole
    segment (auth_first global), `tx_block`, and per block `block_first_bad`, `block_blob_gas_used`, `transactions_root`,
    `withdrawals_root` (where computed), `block_flags`; the scalars `first_bad_block`, `first_bad`, `n_auth`, `blob_gas_used`."""
    FLAG_NAMES = L.BODY_FLAG_NAMES

    def __init__(self, arrays, first_bad_block, first_bad, n_auth, blob_gas_used):
        self.first_bad_block, self.first_bad, self.n_auth, self.blob_gas_used = first_bad_block, first_bad, n_auth, blob_gas_used
        self.__dict__.update(arrays)
        self.n, self.n_blocks = len(self.flags), len(self.block_flags)

    def errors(self, b):
        """the names of block b's flags"""
        return [name for k, name in enumerate(self.FLAG_NAMES) if int(self.block_flags[b]) >> k & 1]


def _rows32(v, n, what):
    """None, n integers or n x 32 bytes -> (n, 32) uint8 big-endian, or None"""
    if v is None:
        return None
    if isinstance(v, np.ndarray) and v.dtype == np.uint8:
        a = np.ascontiguousarray(v).reshape(-1, 32)
    else:
        v = list(v)
        a = np.frombuffer(b"".join(x if isinstance(x, (bytes, bytearray)) else int(x).to_bytes(32, "big") for x in v) or bytes(32), np.uint8).reshape(-1, 32).copy()
    if len(a) < max(n, 1) and n:
        raise ValueError(f"{what}: one row per block")
    return a


def block_bodies(bodies, chain_id, fork, base_fee=None, gas_limit=None, blob_base_fee=None, transactions_root=None, withdrawals_root=None,
                 blob_gas_used=None, recover=True, roots=True, ctx: Context | None = None) -> BlockBodies:
    """phant_block_bodies over the packed arrays of pack_bodies / split_blocks.  Per block (None: the rule or comparison is skipped):
    base_fee, blob_base_fee (integers, or (n_blocks, 32) uint8 rows such as a header segment's own array), gas_limit (integers); the
    expected transactions_root / withdrawals_root (32-byte strings or rows) and blob_gas_used.  roots=False: no root is computed unless
    one is expected."""
    ctx = ctx or default_context()
    a = bodies
    nb, n = len(a["block_first"]) - 1, len(a["tx_off"]) - 1
    has_wd = a.get("wd_first") is not None
    n_wd = len(a["wd_off"]) - 1 if has_wd else 0
    ins = {k: (None if a.get(k) is None else np.ascontiguousarray(a[k])) for k in ("txs", "tx_off", "block_first", "withdrawals", "wd_off", "wd_first")}
    ins["base_fee"], ins["blob_base_fee"] = _rows32(base_fee, nb, "base_fee"), _rows32(blob_base_fee, nb, "blob_base_fee")
    ins["gas_limit"] = None if gas_limit is None else np.ascontiguousarray(gas_limit, np.uint64)
    ins["transactions_root"] = _rows32(transactions_root, nb, "transactions_root")
    ins["withdrawals_root"] = _rows32(withdrawals_root, nb, "withdrawals_root") if has_wd else None
    ins["blob_gas_used"] = None if blob_gas_used is None else np.ascontiguousarray(blob_gas_used, np.uint64)
    for k in ("gas_limit", "blob_gas_used"):
        if ins[k] is not None and len(ins[k]) < nb:
            raise ValueError(f"{k}: one value per block")
    blob = ins["txs"]
    flags = (L.TXS_HAVE_GAS_LIMIT if gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
    tx_off = ins["tx_off"]
    cap = sum(int(tx_off[i + 1] - tx_off[i]) for i in range(n) if tx_off[i + 1] > tx_off[i] and blob[int(tx_off[i])] == 4) // 27 if fork >= L.TXS_FORK_PRAGUE else 0
    arrays = {name: np.zeros((n, k) if k > 1 else n, dtype) for name, dtype, k in L.TX_OUTPUTS if recover or name not in ("sender", "sig_status")}
    for name, dtype, k in L.TX_EX_OUTPUTS:
        arrays[name] = np.zeros((n, k) if k > 1 else n + (name == "auth_first"), dtype)
    auth = {name: np.zeros((cap, k) if k > 1 else cap, dtype) for name, dtype, k in L.TX_AUTH_OUTPUTS if recover or name not in ("authority", "auth_status")}
    rows = {"n": n, "n_blocks": nb}
    own = {name: np.zeros((rows[r], k) if k > 1 else rows[r], dtype) for name, dtype, k, r in L.BODIES_OUTPUTS}
    if not roots:
        own.pop("transactions_root"), own.pop("withdrawals_root")
    elif not has_wd:
        own.pop("withdrawals_root")
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None  # noqa: E731
    arg = L.PhantBodiesIn(C.sizeof(L.PhantBodiesIn), int(fork), flags, nb, n, n_wd, cap, 0, int(chain_id), ptr(blob) if n else None, ptr(tx_off) if n else None,
                          int(tx_off[-1]), ins["block_first"].ctypes.data, ptr(ins["withdrawals"]) if n_wd else None, ptr(ins["wd_off"]) if n_wd else None,
                          int(ins["wd_off"][-1]) if has_wd else 0, *[ptr(ins[k]) for k in L.BODIES_INPUTS[5:]])
    out_base = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[ptr(arrays.get(name)) for name, _, _ in L.TX_OUTPUTS])
    xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0, 0, out_base, *[arrays[name].ctypes.data for name, _, _ in L.TX_EX_OUTPUTS],
                           *[ptr(auth.get(name)) for name, _, _ in L.TX_AUTH_OUTPUTS])
    out = L.PhantBodiesOut(C.sizeof(L.PhantBodiesOut), 0, xout, *[ptr(own.get(name)) for name, _, _, _ in L.BODIES_OUTPUTS])
    ctx.check(ctx._lib.phant_block_bodies(ctx.handle, C.byref(arg), C.byref(out)))
    arrays.update({name: x[:int(out.txs.n_auth)] for name, x in auth.items()})
    arrays.update(own)
    arrays["blob"], arrays["block_first"] = blob, ins["block_first"]  # (block_first: what fee_history joins the receipts' rows by)
    return BlockBodies(arrays, int(out.first_bad_block), int(out.txs.base.first_bad), int(out.txs.n_auth), int(out.txs.blob_gas_used))


class SegmentVerdict:
    """validate_segment's answer: per block `header_flags` (Flags) and `body_flags` (BodyFlags; 0 for a segment's anchor, whose body is
    not checked, and PHANT_BODY_* otherwise), `split_status` (SPLIT_*), `hashes`, `first_bad` (the least block with any of the three, n
    if none), and the two calls' results `headers` and `bodies`."""

    def __init__(self, header_flags, body_flags, split_status, hashes, headers, bodies):
        self.header_flags, self.body_flags, self.split_status, self.hashes, self.headers, self.bodies = header_flags, body_flags, split_status, hashes, headers, bodies
        bad = np.flatnonzero((header_flags != 0) | (body_flags != 0) | (split_status != 0))
        self.first_bad = int(bad[0]) if len(bad) else len(header_flags)


def validate_segment(raw_blocks, seg_first=None, chain_id=1, fork=L.TXS_FORK_PRAGUE, recover=True, ctx: Context | None = None) -> SegmentVerdict:
    """Headers and bodies of raw blocks [header, txs, uncles, withdrawals?] in two calls: phant_header_chain over the decoded headers
    (seg_first as there; a segment's first block is its anchor), phant_block_bodies over the split bodies with the headers' own arrays
    as parameters and expectations: base fee, gas limit, transactions root, withdrawals root (where the headers have one), blob gas used
    (where they have it), and each block's blob base fee from its parent's excess blob gas.  An anchor's body is not checked (its
    parent's excess blob gas is unknown): its transactions do not enter the call."""
    from .transaction import blob_base_fee as _blob_base_fee
    ctx = ctx or default_context()
    raws = [bytes(r) for r in raw_blocks]
    n = len(raws)
    ha, hstatus = decode_arrays(raws, from_blocks=True)
    if hstatus.any():
        raise ValueError(f"block {int(np.flatnonzero(hstatus)[0])} does not begin with a canonical header")
    chain = header_chain(None, seg_first, ctx=ctx, arrays=ha)
    seg = np.asarray([0, n] if seg_first is None else seg_first, np.int64)
    anchor = np.zeros(n, bool)
    anchor[seg[:-1][seg[:-1] < n]] = True
    body = np.flatnonzero(~anchor)
    a, status = split_blocks([raws[i] for i in body])
    split_status = np.zeros(n, np.uint8)
    split_status[body] = status
    nf = ha["n_fields"][:n]
    with_wd, with_blob = bool(len(body)) and bool((nf[body] >= 17).all()), bool(len(body)) and bool((nf[body] >= 19).all())
    if not with_wd:
        if int(a["wd_first"][-1]):
            raise ValueError("a block carries withdrawals although a header of the segment has no withdrawals root")
        a = dict(a, withdrawals=None, wd_off=None, wd_first=None)
    blob_fee = None
    if with_blob and fork >= L.TXS_FORK_CANCUN:
        blob_fee = [_blob_base_fee(int(ha["excess_blob_gas"][i - 1]), fork) for i in body]
    pick = lambda name: np.ascontiguousarray(ha[name][body])  # noqa: E731
    bodies = block_bodies(a, chain_id, fork, base_fee=pick("base_fee") if bool(len(body)) and bool((nf[body] >= 16).all()) else None, gas_limit=pick("gas_limit"),
                          blob_base_fee=blob_fee, transactions_root=pick("transactions_root"), withdrawals_root=pick("withdrawals_root") if with_wd else None,
                          blob_gas_used=pick("blob_gas_used") if with_blob else None, recover=recover, ctx=ctx) if len(body) else None
    body_flags = np.zeros(n, np.uint32)
    if bodies is not None:
        body_flags[body] = bodies.block_flags
    return SegmentVerdict(np.asarray(chain.flags, np.uint32).copy(), body_flags, split_status, chain.hashes, chain, bodies)


# -------------------------------------------------------------------------------------------- receipts of chain segments
class ReceiptsVerdict:
    """validate_receipts' answer: per block `block_flags` (receipt.ReceiptBlockFlags) and `split_status` (SPLIT_OK, SPLIT_BAD_RLP,
    SPLIT_BAD_RECEIPT), `first_bad` (the least block with either, n if none), `reason` (the names of that block's flags, or its split
    status; [] when every block is good), and the call's result `receipts`."""

    def __init__(self, block_flags, split_status, receipts):
        self.block_flags, self.split_status, self.receipts = block_flags, split_status, receipts
        bad = np.flatnonzero((block_flags != 0) | (split_status != 0))
        self.first_bad = int(bad[0]) if len(bad) else len(block_flags)
        self.reason = []
        if len(bad):
            b = self.first_bad
            self.reason = ["BadRlp" if split_status[b] == SPLIT_BAD_RLP else "BadReceipt"] if split_status[b] else receipts.errors(b)


def validate_receipts(headers, raw_receipts, eth69=False, tx_counts=None, ctx: Context | None = None, logs=False) -> ReceiptsVerdict:
    """The receipts of a chain segment against its headers in one call: `headers` are decoded headers (BlockHeader objects, or the arrays
    of decode_arrays), `raw_receipts` the per-block elements of a peer's Receipts answer, one per header, in the eth/69 form (no blooms
    on the wire) or the earlier one.  phant_receipts_decode_rlp splits them; phant_block_receipt_segments decodes every receipt,
    computes the blooms, (eth/69) rebuilds the consensus encodings and compares each block's receipts root, logs bloom and gas used
    with its header, and its receipt count with tx_counts[b] where the caller has the transaction counts.  logs=True: the result keeps
    the per-log arrays, which validate_requests reads."""
    from .receipt import receipt_segments, split_receipts
    n = len(raw_receipts)
    if isinstance(headers, dict):
        expect = {"receipts_root": np.ascontiguousarray(headers["receipts_root"]).reshape(-1, 32)[:n], "logs_bloom": np.ascontiguousarray(headers["logs_bloom"]).reshape(-1, 256)[:n],
                  "gas_used": np.ascontiguousarray(headers["gas_used"][:n], np.uint64)}
    else:
        headers = list(headers)
        expect = {"receipts_root": [h.receipts_root for h in headers], "logs_bloom": [h.logs_bloom for h in headers], "gas_used": [h.gas_used for h in headers]}
    if len(expect["gas_used"]) != n:
        raise ValueError("one header per block of receipts")
    if tx_counts is not None:
        expect["tx_count"] = tx_counts
    a, status = split_receipts(raw_receipts, eth69)
    res = receipt_segments(a, form=L.RCPTS_ETH69 if eth69 else L.RCPTS_CONSENSUS, expect=expect, logs=logs, ctx=ctx)
    return ReceiptsVerdict(np.asarray(res.block_flags, np.uint32).copy(), status.copy(), res)


# ---------------------------------------------------------------------------------- execution requests of chain segments
class RequestsVerdict:
    """validate_requests' answer: per block `block_flags` (receipt.RequestsFlags), `first_bad` (the least flagged block, n if none),
    `reason` (the names of that block's flags; [] when every block is good), and the call's result `requests`."""

    def __init__(self, block_flags, requests):
        self.block_flags, self.requests = block_flags, requests
        bad = np.flatnonzero(block_flags != 0)
        self.first_bad = int(bad[0]) if len(bad) else len(block_flags)
        self.reason = requests.errors(self.first_bad) if len(bad) else []


def validate_requests(headers, segs, deposit_contract, other_requests=None, ctx: Context | None = None) -> RequestsVerdict:
    """The execution requests of a chain segment against its headers in one call (EIP-7685): `headers` are decoded headers (BlockHeader
    objects, or the arrays of decode_arrays), `segs` the result of receipt_segments over the same blocks with its per-log arrays (what
    validate_receipts returns as `.receipts` when it is asked for the logs), `other_requests` per block the (type, data) rows the EVM's
    system calls produced.  A block is active when its header has the 21st field; its requests_hash is the expected value.  The flags
    stand beside those of validate_receipts: phant_block_requests rebuilds the deposit requests from the logs of `deposit_contract`
    (EIP-6110), hashes each block's requests with SHA-256 and compares."""
    from .receipt import block_requests
    nb = segs.n_blocks
    if isinstance(headers, dict):
        nf = np.asarray(headers["n_fields"][:nb])
        want = np.ascontiguousarray(headers["requests_hash"]).reshape(-1, 32)[:nb]
    else:
        headers = list(headers)
        nf = np.asarray([h.n_fields for h in headers])
        want = np.frombuffer(b"".join(h.request_hash or bytes(32) for h in headers) or bytes(32), np.uint8).reshape(-1, 32)
    if len(nf) != nb:
        raise ValueError("one header per block of receipts")
    res = block_requests(segs, deposit_contract, other_requests, active=(nf >= 21).tolist(), expect=np.ascontiguousarray(want), ctx=ctx)
    return RequestsVerdict(np.asarray(res.block_flags, np.uint32).copy(), res)


# ---------------------------------------------------------------------------------- log filters over the headers of a segment
def candidate_blocks(headers, filters, ctx: Context | None = None):
    """Which blocks of a chain segment can hold a log that a filter selects, from the headers alone (phant_log_filters_bloom over their
    logs_bloom): `headers` are decoded headers (BlockHeader objects, or the arrays of decode_arrays), `filters` receipt.LogFilter objects
    whose from_block / to_block index the headers.  -> per filter the ascending indices of its candidate blocks -- the blocks whose
    receipts are worth fetching; a block that holds a match is always among them."""
    from .receipt import bloom_candidates
    if isinstance(headers, dict):
        blooms = np.ascontiguousarray(headers["logs_bloom"], np.uint8).reshape(-1, 256)
    else:
        blooms = np.frombuffer(b"".join(bytes(h.logs_bloom) for h in headers), np.uint8).reshape(-1, 256)
    may, _ = bloom_candidates(blooms, filters, ctx=ctx)
    return [np.flatnonzero(row) for row in may]


# ------------------------------------------------------------------------------------- fee history over a chain segment
class RewardPercentiles:
    """reward_percentiles' answer: `reward` ((n_blocks, n_percentiles, 32) uint8, big-endian), `tip` ((n, 32) uint8), `order` (n: the
    global row with each rank, block by block), `block_gas_used`, `flags` (FEE_BELOW_BASE per block) and `first_bad_block`; host arrays,
    or device tensors when the rows were.  rewards() = the rewards as Python integers (host arrays only)."""

    def __init__(self, reward, tip, order, block_gas_used, flags, first_bad_block):
        self.reward, self.tip, self.order, self.block_gas_used, self.flags, self.first_bad_block = reward, tip, order, block_gas_used, flags, first_bad_block

    def rewards(self):
        return [[int.from_bytes(bytes(r), "big") for r in row] for row in np.asarray(self.reward)]


def reward_percentiles(block_first, price, gas_used, percentiles_bp, base_fee=None, ctx: Context | None = None) -> RewardPercentiles:
    """phant_block_fee_history: per block the priority fee at the percentiles (basis points, at most 10000 each) of its gas used.
    block_first (n_blocks + 1), price (n x 32 bytes big-endian: block_bodies' effective_gas_price), gas_used (n: receipt_segments'),
    base_fee (n_blocks x 32 bytes big-endian, or None: zero) as numpy arrays, or as torch tensors on the device -- then the device form
    runs on them without a copy, and the answer's arrays are device tensors."""
    ctx = ctx or default_context()
    dev = hasattr(price, "data_ptr")
    pct = np.ascontiguousarray(percentiles_bp, np.uint32).reshape(-1)
    rows = {"block_first": block_first, "price": price, "base_fee": base_fee, "gas_used": gas_used}
    if dev:
        import torch
        device = price.device
        kind = {"u4": torch.int32, "u1": torch.uint8, "u8": torch.int64}
        rows = {k: None if v is None else v.contiguous().view(torch.uint8).view(kind[dt]) for (k, dt, _), v in ((f, rows[f[0]]) for f in L.FEEHIST_INPUTS[:4])}
        count = lambda x: x.numel()  # noqa: E731
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        new = lambda shape, dt: torch.zeros(shape, dtype=kind[dt], device=device)  # noqa: E731
        fn = ctx._lib.phant_block_fee_history_dev
    else:
        rows = {k: None if v is None else np.ascontiguousarray(v, dt) for (k, dt, _), v in ((f, rows[f[0]]) for f in L.FEEHIST_INPUTS[:4])}
        count = lambda x: x.size  # noqa: E731
        ptr = lambda x: x.ctypes.data if x is not None and x.size else None  # noqa: E731
        new = lambda shape, dt: np.zeros(shape, dt)  # noqa: E731
        fn = ctx._lib.phant_block_fee_history
    nb, n = count(rows["block_first"]) - 1, count(rows["gas_used"])
    if count(rows["price"]) != 32 * n or (rows["base_fee"] is not None and count(rows["base_fee"]) != 32 * nb):
        raise ValueError("price is n x 32 bytes, base_fee n_blocks x 32 bytes")
    outs = {"reward": new((nb, len(pct), 32), "u1"), "tip": new((n, 32), "u1"), "order": new(n, "u4"), "block_gas_used": new(nb, "u8"), "block_flags": new(nb, "u4")}
    arg = L.PhantFeeHistoryIn(C.sizeof(L.PhantFeeHistoryIn), nb, n, len(pct), rows["block_first"].data_ptr() if dev else rows["block_first"].ctypes.data,
                              ptr(rows["price"]), ptr(rows["base_fee"]), ptr(rows["gas_used"]), pct.ctypes.data if len(pct) else None, 0)
    out = L.PhantFeeHistoryOut(C.sizeof(L.PhantFeeHistoryOut), 0, *[ptr(outs[name]) for name, _, _ in L.FEEHIST_OUTPUTS], 0)
    ctx.check(fn(ctx.handle, C.byref(arg), C.byref(out)))
    if dev:
        torch.cuda.synchronize(device)
    return RewardPercentiles(outs["reward"], outs["tip"], outs["order"], outs["block_gas_used"], outs["block_flags"], int(out.first_bad_block))


def next_base_fee(base_fee: int, gas_used: int, gas_limit: int) -> int:
    """The base fee of the block after one with these fields: the EIP-1559 rule as include/phant_gpu.h states it for PHANT_HDR_BASE_FEE
    (t = gas_limit / 2, all divisions floor).  A zero gas target with gas used has no answer (the header rule flags it): ValueError."""
    t = gas_limit // 2
    if gas_used == t:
        return base_fee
    if t == 0:
        raise ValueError("a gas target of zero with gas used")
    if gas_used > t:
        return base_fee + max(base_fee * (gas_used - t) // t // 8, 1)
    return base_fee - base_fee * (t - gas_used) // t // 8


_BLOB_GAS = {L.TXS_FORK_CANCUN: (3 * 131072, 6 * 131072), L.TXS_FORK_PRAGUE: (6 * 131072, 9 * 131072)}  # (target, maximum) per block: EIP-4844, EIP-7691


def _bp(percentiles):
    """eth_feeHistory's rewardPercentiles, floats of at most two decimals in [0, 100] -> basis points"""
    out = []
    for p in percentiles:
        bp = round(float(p) * 100)
        if not 0 <= bp <= 10000 or abs(float(p) * 100 - bp) > 1e-6:
            raise ValueError(f"a percentile is a number from 0 to 100 with at most two decimals, not {p!r}")
        out.append(bp)
    return out


def fee_history(headers, bodies, receipts, percentiles, fork, ctx: Context | None = None) -> dict:
    """The eth_feeHistory answer for a chain segment: `headers` are the segment's decoded headers (BlockHeader objects), `bodies` what
    block_bodies answered for them (or a dict of its block_first and effective_gas_price), `receipts` what receipt_segments answered
    (or a dict of its block_first and gas_used).  -> a dict of
    oldestBlock, baseFeePerGas and baseFeePerBlobGas (n + 1 entries: the last is the next block's), gasUsedRatio, blobGasUsedRatio and
    reward (per block, per percentile; phant_block_fee_history).  Everything but reward is host arithmetic on n + 1 numbers.  A
    transaction i of a block must be its receipt i: a block_first that differs between bodies and receipts is a ValueError."""
    from .transaction import blob_base_fee as _blob_base_fee
    get = lambda src, k: src[k] if isinstance(src, dict) else getattr(src, k)  # noqa: E731
    headers = list(headers)
    n = len(headers)
    bp = _bp(percentiles)
    first = np.ascontiguousarray(get(bodies, "block_first"), np.uint32)
    if first.tobytes() != np.ascontiguousarray(get(receipts, "block_first"), np.uint32).tobytes():
        raise ValueError("the bodies' block_first differs from the receipts': transaction i of a block is not its receipt i")
    if len(first) != n + 1:
        raise ValueError("one header per block")
    london = all(h.base_fee_per_gas is not None for h in headers)
    base = [int(h.base_fee_per_gas) if london else 0 for h in headers]
    res = reward_percentiles(first, get(bodies, "effective_gas_price"), get(receipts, "gas_used"), bp, base_fee=_rows32(base, n, "base_fee") if london and n else None, ctx=ctx)
    out = {"oldestBlock": int(headers[0].block_number) if n else 0, "reward": res.rewards(),
           "gasUsedRatio": [h.gas_used / h.gas_limit if h.gas_limit else 0.0 for h in headers]}
    out["baseFeePerGas"] = base + ([next_base_fee(base[-1], int(headers[-1].gas_used), int(headers[-1].gas_limit))] if london and n else [0])
    blob = fork >= L.TXS_FORK_CANCUN and all(h.excess_blob_gas is not None and h.blob_gas_used is not None for h in headers)
    if blob and n:
        target, most = _BLOB_GAS[fork]
        last = headers[-1]
        excess = [int(h.excess_blob_gas) for h in headers] + [max(int(last.excess_blob_gas) + int(last.blob_gas_used) - target, 0)]
        out["baseFeePerBlobGas"] = [_blob_base_fee(x, fork) for x in excess]
        out["blobGasUsedRatio"] = [h.blob_gas_used / most for h in headers]
    else:
        out["baseFeePerBlobGas"], out["blobGasUsedRatio"] = [0] * (n + 1), [0.0] * n
    return out
