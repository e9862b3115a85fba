"""Logs blooms of a whole block in one launch <-> src/types/receipt.zig:37-63 (`calculateLogsBloom`, `addToBloom`).

A log is (address: 20 bytes, topics: list of 32-byte values) as in receipt.zig:66-70 (`Log`); its data does not
enter the bloom.  Through the C-ABI (phant_logs_bloom); no CPU fallback.

`Log`, `Receipt` and `block_receipts` <-> receipt.zig:13-35,66-70 and the receipts side of blockchain.zig:76-90: a block's
receipts from their fields to blooms, encodings, the receipts root and the block's bloom in ONE call (phant_block_receipts).
One deviation from the reference: its Receipt.encode has no EIP-2718 type prefix yet, the fixtures' receiptTrie values
commit to one -- hence `tx_type`, and tx_type 0 reproduces the reference."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from .. import _lib as L
from ..context import Context, default_context, _np_ptr


def _flatten(receipts_logs):
    items, owner = [], []
    for r, logs in enumerate(receipts_logs):
        for address, topics in logs:
            items.append(bytes(address))
            owner.append(r)
            for t in topics:
                items.append(bytes(t))
                owner.append(r)
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(x) for x in items])
    blob = np.frombuffer(b"".join(items), np.uint8).copy() if off[-1] else np.zeros(1, np.uint8)
    return blob, off, np.asarray(owner if owner else [0], np.uint32), len(items)


def logs_blooms(receipts_logs, ctx: Context | None = None) -> np.ndarray:
    """receipts_logs: one list of logs per receipt -> (n_receipts, 256) uint8, row r = calculateLogsBloom of
    receipt r's logs (receipt.zig:37-48)."""
    ctx = ctx or default_context()
    blob, off, owner, n_items = _flatten(receipts_logs)
    out = np.zeros((len(receipts_logs), 256), np.uint8)
    if len(receipts_logs):
        ctx.check(ctx._lib.phant_logs_bloom(ctx.handle, _np_ptr(blob), _np_ptr(off), _np_ptr(owner), n_items,
                                            len(receipts_logs), _np_ptr(out)))
    return out


def calculate_logs_bloom(logs, ctx: Context | None = None) -> bytes:
    """receipt.zig:37 `calculateLogsBloom(logs: []Log) LogsBloom` for one receipt."""
    return logs_blooms([logs], ctx)[0].tobytes()


@dataclass
class Log:
    """receipt.zig:66-70 `Log`"""
    address: bytes
    topics: list = field(default_factory=list)
    data: bytes = b""


@dataclass
class Receipt:
    """receipt.zig:7-11 `Receipt` (its bloom is computed, not stored) plus the transaction's EIP-2718 type."""
    succeeded: bool
    cumulative_gas_used: int
    logs: list = field(default_factory=list)
    tx_type: int = 0

    @classmethod
    def init(cls, succeeded, cumulative_gas_used, logs, tx_type=0) -> "Receipt":
        """receipt.zig:13 `init`"""
        return cls(bool(succeeded), int(cumulative_gas_used), [lg if isinstance(lg, Log) else Log(*lg) for lg in logs], int(tx_type))

    @property
    def bloom(self) -> bytes:
        """receipt.zig:37 `calculateLogsBloom` of this receipt's logs"""
        return block_receipts([self]).blooms[0].tobytes()

    def encode(self) -> bytes:
        """receipt.zig:24 `encode`, behind the type byte when tx_type != 0"""
        return block_receipts([self]).encoded[0]


@dataclass
class BlockReceipts:
    roots: list            # one 32-byte root per trie: the riding lists with the receipts at `receipts_at`
    receipts_root: bytes
    logs_bloom: bytes      # the block's
    blooms: np.ndarray     # (n, 256) uint8
    encoded: list          # n byte strings, index order


def pack_receipts(receipts):
    """-> the struct-of-arrays of phant_receipts_in as numpy arrays (never empty: a zero count gets one spare element)."""
    n = len(receipts)
    logs = [lg for r in receipts for lg in r.logs]
    u8 = lambda b, width: np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(width, np.uint8)  # noqa: E731
    a = {
        "tx_type": np.array([r.tx_type for r in receipts] or [0], np.uint8),
        "status": np.array([1 if r.succeeded else 0 for r in receipts] or [0], np.uint8),
        "cum_gas": np.array([r.cumulative_gas_used for r in receipts] or [0], np.uint64),
        "log_first": np.cumsum([0] + [len(r.logs) for r in receipts]).astype(np.uint32),
        "address": u8(b"".join(bytes(lg.address) for lg in logs), 20),
        "topic_first": np.cumsum([0] + [len(lg.topics) for lg in logs]).astype(np.uint32),
        "data_off": np.cumsum([0] + [len(lg.data) for lg in logs]).astype(np.uint64),
        "topics": u8(b"".join(bytes(t) for lg in logs for t in lg.topics), 32),
        "data": u8(b"".join(bytes(lg.data) for lg in logs), 1),
    }
    for lg in logs:
        if len(lg.address) != 20 or any(len(t) != 32 for t in lg.topics):
            raise ValueError("a log's address is 20 bytes, a topic 32")
    return a, n, len(logs), int(a["topic_first"][-1]), int(a["data_off"][-1])


def block_receipts(receipts, ctx: Context | None = None, other_lists=(), receipts_at: int = 0) -> BlockReceipts:
    """The receipts side of blockchain.zig:76-90 in one call and one synchronisation: blooms, encodings, receipts root and
    the block's bloom of `receipts` (Receipt objects); `other_lists` (lists of already encoded items: transactions,
    withdrawals) are hashed in the same forest pass, `receipts_at` is the receipts' place among them in `.roots`."""
    ctx = ctx or default_context()
    receipts = list(receipts)
    a, n, n_logs, n_topics, data_bytes = pack_receipts(receipts)
    others = [[bytes(x) for x in lst] for lst in other_lists]
    nl = len(others)
    blobs = [np.frombuffer(b"".join(lst), np.uint8).copy() if sum(map(len, lst)) else np.zeros(1, np.uint8) for lst in others]
    offs = [np.cumsum([0] + [len(x) for x in lst]).astype(np.uint64) for lst in others]
    list_n = np.array([len(lst) for lst in others] or [0], np.uint32)
    lists_p = (C.c_void_p * max(nl, 1))(*[b.ctypes.data for b in blobs])
    offs_p = (C.c_void_p * max(nl, 1))(*[o.ctypes.data for o in offs])
    p = lambda x: x.ctypes.data  # noqa: E731
    arg = L.PhantReceiptsIn(C.sizeof(L.PhantReceiptsIn), n, n_logs, n_topics, data_bytes, p(a["tx_type"]), p(a["status"]),
                            p(a["cum_gas"]), p(a["log_first"]), p(a["address"]), p(a["topic_first"]), p(a["data_off"]),
                            p(a["topics"]), p(a["data"]), C.cast(lists_p, C.c_void_p) if nl else None,
                            C.cast(offs_p, C.c_void_p) if nl else None, p(list_n) if nl else None, None, nl, receipts_at)
    roots = np.zeros((nl + 1, 32), np.uint8)
    bloom = np.zeros(256, np.uint8)
    rows = np.zeros((max(n, 1), 256), np.uint8)
    enc_off = np.zeros(n + 1, np.uint64)
    # the encodings' size is the call's to say: room for a block of ordinary receipts first, the reported size if that was short
    cap = 320 * n + 64 * n_logs + 33 * n_topics + data_bytes + 16
    for _ in range(2):
        enc = np.zeros(max(cap, 1), np.uint8)
        out = L.PhantReceiptsOut(C.sizeof(L.PhantReceiptsOut), n + 1, cap, None, p(bloom), p(rows), p(enc), p(enc_off), p(roots), 0)
        ctx.check(ctx._lib.phant_block_receipts(ctx.handle, C.byref(arg), C.byref(out)))
        if out.encoded_len <= cap:
            break
        cap = int(out.encoded_len)
    encoded = [enc[int(enc_off[i]):int(enc_off[i + 1])].tobytes() for i in range(n)]
    return BlockReceipts([r.tobytes() for r in roots], roots[receipts_at].tobytes(), bloom.tobytes(), rows[:n], encoded)


# ------------------------------------------------------------------------------------ receipts of chain segments from raw messages
class ReceiptFlags:
    """flags[i] of receipt_segments"""
    Undecodable = L.RCPT_UNDECODABLE
    Bloom = L.RCPT_BLOOM
    GasOrder = L.RCPT_GAS_ORDER
    PostState = L.RCPT_POST_STATE
    ERROR_BITS = L.RCPT_ERROR_BITS


class ReceiptBlockFlags:
    """block_flags[b] of receipt_segments"""
    Receipt = L.RBLOCK_RECEIPT
    ReceiptsRoot = L.RBLOCK_ROOT
    LogsBloom = L.RBLOCK_BLOOM
    GasUsed = L.RBLOCK_GAS_USED
    Count = L.RBLOCK_COUNT
    NAMES = L.RBLOCK_FLAG_NAMES


def pack_receipt_segments(blocks):
    """per block its raw receipt values (one wire form for all) -> the packed arrays phant_block_receipt_segments takes: receipts, rc_off,
    block_first; never empty arrays.  (pack_receipts above packs the FIELDS of one block for phant_block_receipts.)"""
    blocks = [[bytes(x) for x in b] for b in blocks]
    items = [x for b in blocks for x in b]
    return {"receipts": np.frombuffer(b"".join(items) or b"\x00", np.uint8).copy(), "rc_off": np.cumsum([0] + [len(x) for x in items]).astype(np.uint64),
            "block_first": np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)}


def split_receipts(raw_blocks, eth69=False):
    """phant_receipts_decode_rlp: the per-block elements of a Receipts message (each the RLP list of a block's receipts) -> (the packed
    arrays of pack_receipt_segments, status uint8[n]); a refused block (status != 0: SPLIT_BAD_RLP, SPLIT_BAD_RECEIPT) has no rows.  Host only."""
    raws = [bytes(r) for r in raw_blocks]
    n = len(raws)
    blob = np.frombuffer(b"".join(raws) or b"\x00", np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in raws]).astype(np.uint64)
    status = np.zeros(max(n, 1), np.uint8)
    flags = L.RCPTS_SPLIT_ETH69 if eth69 else 0
    arg = L.PhantReceiptsSplit(C.sizeof(L.PhantReceiptsSplit))
    fn = L.lib().phant_receipts_decode_rlp
    a = None
    for _ in range(2):  # the totals, then the arrays
        rc = fn(blob.ctypes.data, off.ctypes.data, n, flags, C.byref(arg), status.ctypes.data)
        if rc != L.OK:
            raise L.PhantError(rc, "phant_receipts_decode_rlp")
        if a is None:
            a = {"receipts": np.zeros(max(int(arg.rc_bytes), 1), np.uint8), "rc_off": np.zeros(int(arg.n) + 1, np.uint64), "block_first": np.zeros(n + 1, np.uint32)}
            arg.rc_cap, arg.rc_bytes_cap = int(arg.n), int(arg.rc_bytes)
            arg.receipts, arg.rc_off, arg.block_first = (a[k].ctypes.data for k in ("receipts", "rc_off", "block_first"))
    return a, status[:n]


class ReceiptSegments:
    """What phant_block_receipt_segments answers: per receipt `tx_type`, `status`, `cum_gas`, `gas_used`, `log_first`, `bloom`, `flags`; per
    log `log_receipt`, `address`, `topic_first`, `topics`, `data_at`, `data_len`; `encoded` (n byte strings: the consensus encodings) where
    asked for; per block `receipts_root` (where computed), `logs_bloom`, `block_gas_used`, `block_first_bad`, `block_flags`; the scalars
    `first_bad_block`, `n_logs`, `n_topics`."""
    FLAG_NAMES = L.RBLOCK_FLAG_NAMES

    def __init__(self, arrays, first_bad_block, n_logs, n_topics):
        self.first_bad_block, self.n_logs, self.n_topics = first_bad_block, n_logs, n_topics
        self.__dict__.update(arrays)
        self.n, self.n_blocks = len(self.flags), len(self.block_flags)

    def errors(self, b):
        """the names of block b's flags"""
        return [name for k, name in enumerate(self.FLAG_NAMES) if int(self.block_flags[b]) >> k & 1]


def receipt_segments(packed, form=L.RCPTS_CONSENSUS, expect=None, roots=True, logs=True, encoded=False, ctx: Context | None = None) -> ReceiptSegments:
    """phant_block_receipt_segments over the packed arrays of pack_receipt_segments / split_receipts.  expect: a dict with any of
    receipts_root ((n_blocks, 32) uint8 or 32-byte strings), logs_bloom ((n_blocks, 256) or 256-byte strings), gas_used, tx_count (integers);
    a missing key skips its comparison.  roots=False: no root is computed unless one is expected; logs=False: no per-log array;
    encoded=True: the consensus encodings, which an ETH69 caller stores."""
    ctx = ctx or default_context()
    expect = expect or {}
    a = {k: np.ascontiguousarray(packed[k]) for k in ("receipts", "rc_off", "block_first")}
    nb, n = len(a["block_first"]) - 1, len(a["rc_off"]) - 1
    nbytes = int(a["rc_off"][-1])

    def rows(v, width):
        if v is None:
            return None
        if isinstance(v, np.ndarray) and v.dtype == np.uint8:
            r = np.ascontiguousarray(v).reshape(-1, width)
        else:
            r = np.frombuffer(b"".join(bytes(x) for x in v) or bytes(width), np.uint8).reshape(-1, width).copy()
        if len(r) < nb:
            raise ValueError("an expected value per block")
        return r

    ins = dict(a, receipts_root=rows(expect.get("receipts_root"), 32), logs_bloom=rows(expect.get("logs_bloom"), 256),
               gas_used=None if expect.get("gas_used") is None else np.ascontiguousarray(expect["gas_used"], np.uint64),
               tx_count=None if expect.get("tx_count") is None else np.ascontiguousarray(expect["tx_count"], np.uint32))
    for k in ("gas_used", "tx_count"):
        if ins[k] is not None and len(ins[k]) < nb:
            raise ValueError(f"{k}: one value per block")
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None  # noqa: E731
    # the rows of the logs and the bytes of the encodings are the call's to say: room for what the bytes can hold at most first
    count = {"n": n, "n_blocks": nb, "n_logs": nbytes // 24 if logs else 0, "n_topics": nbytes // 33 if logs else 0, "encoded_len": nbytes + 268 * n if encoded else 0}
    skip = set() if roots else {"receipts_root"}
    skip |= set() if logs else {"log_receipt", "address", "topic_first", "topics", "data_at", "data_len"}
    skip |= set() if encoded else {"encoded", "encoded_off"}
    out_arrays = {name: np.zeros((count[r] + extra, k) if k > 1 else count[r] + extra, dtype) for name, dtype, k, r, extra in L.RSEG_OUTPUTS if name not in skip}
    arg = L.PhantRcptSegsIn(C.sizeof(L.PhantRcptSegsIn), int(form), nb, n, count["n_logs"], count["n_topics"], (C.c_uint32 * 2)(0, 0), ptr(a["receipts"]) if n else None,
                            ptr(a["rc_off"]) if n else None, nbytes, a["block_first"].ctypes.data, *[ptr(ins[k]) for k in L.RSEG_INPUTS[3:]])
    out = L.PhantRcptSegsOut(C.sizeof(L.PhantRcptSegsOut), 0, 0, 0, count["encoded_len"], 0, *[ptr(out_arrays.get(name)) for name, _, _, _, _ in L.RSEG_OUTPUTS])
    ctx.check(ctx._lib.phant_block_receipt_segments(ctx.handle, C.byref(arg), C.byref(out)))
    nl, nt = int(out.n_logs), int(out.n_topics)
    for name, _, _, r, extra in L.RSEG_OUTPUTS:
        if name in out_arrays and r in ("n_logs", "n_topics"):
            out_arrays[name] = out_arrays[name][:(nl if r == "n_logs" else nt) + extra]
    if encoded:
        off, blob = out_arrays.pop("encoded_off"), out_arrays["encoded"]
        out_arrays["encoded"] = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    out_arrays["receipts"], out_arrays["block_first"] = a["receipts"][:nbytes], a["block_first"]  # (what block_requests reads the logs' data from)
    return ReceiptSegments(out_arrays, int(out.first_bad_block), nl, nt)


# --------------------------------------------------------------------------------- execution requests of chain segments
class RequestsFlags:
    """block_flags[b] of block_requests"""
    DepositLayout = L.QBLOCK_DEPOSIT_LAYOUT
    RequestsOrder = L.QBLOCK_ORDER
    RequestsHash = L.QBLOCK_HASH
    NAMES = L.QBLOCK_FLAG_NAMES


class BlockRequests:
    """What phant_block_requests answers: per deposit `deposit_log` (its log's index) and `deposit` ((n_deposits, 192) uint8: pubkey,
    credentials, amount, signature, index); per block `deposit_first`, `requests_hash`, `block_flags`; the scalars `n_deposits` and
    `first_bad_block`."""
    FLAG_NAMES = L.QBLOCK_FLAG_NAMES

    def __init__(self, arrays, n_deposits, first_bad_block):
        self.n_deposits, self.first_bad_block = n_deposits, first_bad_block
        self.__dict__.update(arrays)
        self.n_blocks = len(self.block_flags)

    def errors(self, b):
        """the names of block b's flags"""
        return [name for k, name in enumerate(self.FLAG_NAMES) if int(self.block_flags[b]) >> k & 1]

    def requests(self, b):
        """block b's deposit request data: its rows back to back (b"" without one)"""
        return self.deposit[int(self.deposit_first[b]):int(self.deposit_first[b + 1])].tobytes()


def block_requests(segs, deposit_contract, other_requests=None, active=None, expect=None, ctx: Context | None = None) -> BlockRequests:
    """phant_block_requests over the result of receipt_segments (with its per-log arrays): the deposit requests (EIP-6110) rebuilt from
    the logs of `deposit_contract` (20 bytes) and every block's requests_hash (EIP-7685).  other_requests: per block a list of
    (type, data) -- the requests the EVM's system calls produced (types 1 and 2 today), ascending by type; active: per block, False before
    the fork (None: every block); expect: the headers' requests_hash per block ((n_blocks, 32) uint8 or 32-byte strings), or None."""
    ctx = ctx or default_context()
    if not hasattr(segs, "data_at"):
        raise ValueError("block_requests reads the per-log arrays: receipt_segments(..., logs=True)")
    nb, n, nl, nt = segs.n_blocks, segs.n, segs.n_logs, segs.n_topics
    if len(bytes(deposit_contract)) != 20:
        raise ValueError("deposit_contract: 20 bytes")
    other = [list(b) for b in other_requests] if other_requests is not None else [[] for _ in range(nb)]
    if len(other) != nb:
        raise ValueError("other_requests: one list per block")
    rows = [(int(t), bytes(d)) for b in other for t, d in b]
    ins = {"receipts": np.ascontiguousarray(segs.receipts, np.uint8), "block_first": np.ascontiguousarray(segs.block_first, np.uint32),
           "log_first": np.ascontiguousarray(segs.log_first, np.uint32), "address": np.ascontiguousarray(segs.address, np.uint8),
           "topic_first": np.ascontiguousarray(segs.topic_first, np.uint32), "topics": np.ascontiguousarray(segs.topics, np.uint8),
           "data_at": np.ascontiguousarray(segs.data_at, np.uint64), "data_len": np.ascontiguousarray(segs.data_len, np.uint32),
           "req_block_first": np.cumsum([0] + [len(b) for b in other]).astype(np.uint32), "req_type": np.asarray([t for t, _ in rows], np.uint8),
           "req_bytes": np.frombuffer(b"".join(d for _, d in rows), np.uint8), "req_off": np.cumsum([0] + [len(d) for _, d in rows]).astype(np.uint64),
           "active": None if active is None else np.asarray([1 if x else 0 for x in active], np.uint8), "requests_hash": None}
    if ins["active"] is not None and len(ins["active"]) != nb:
        raise ValueError("active: one value per block")
    if expect is not None:
        e = expect if isinstance(expect, np.ndarray) else np.frombuffer(b"".join(bytes(x) for x in expect), np.uint8)
        ins["requests_hash"] = np.ascontiguousarray(e, np.uint8).reshape(-1, 32)
        if len(ins["requests_hash"]) < nb:
            raise ValueError("expect: one hash per block")
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None  # noqa: E731
    count = {"n_blocks": nb, "n_deposits": nl}
    outs = {name: np.zeros((count[r] + extra, k) if k > 1 else count[r] + extra, dtype) for name, dtype, k, r, extra in L.REQUESTS_OUTPUTS}
    arg = L.PhantRequestsIn(C.sizeof(L.PhantRequestsIn), nb, n, nl, nt, len(rows) if nb else 0, nl, 0, ptr(ins["receipts"]), ins["receipts"].size,
                            *[ins[name].ctypes.data if name in ("block_first", "log_first", "topic_first") else ptr(ins[name]) for name, _ in L.REQUESTS_INPUTS[1:12]],
                            int(ins["req_off"][-1]), ptr(ins["active"]), ptr(ins["requests_hash"]), (C.c_uint8 * 20)(*bytes(deposit_contract)))
    out = L.PhantRequestsOut(C.sizeof(L.PhantRequestsOut), 0, 0, 0, *[ptr(outs[name]) for name, _, _, _, _ in L.REQUESTS_OUTPUTS])
    ctx.check(ctx._lib.phant_block_requests(ctx.handle, C.byref(arg), C.byref(out)))
    nd = int(out.n_deposits)
    outs["deposit_log"], outs["deposit"] = outs["deposit_log"][:nd], outs["deposit"][:nd]
    return BlockRequests(outs, nd, int(out.first_bad_block))


# ------------------------------------------------------------------------------------------ log filters over chain segments
@dataclass
class LogFilter:
    """One eth_getLogs filter: `addresses` (20-byte strings; none: any address), `topics` (up to four lists of 32-byte strings, list p
    the values topic p may take; an empty list or None: anything, or no topic at all), the blocks [from_block, to_block) of the segment
    (None: from its first / to its last)."""
    addresses: list = field(default_factory=list)
    topics: list = field(default_factory=list)
    from_block: int | None = None
    to_block: int | None = None


class _PackedFilters:
    """phant_log_filters over numpy arrays (or their copies on the device)"""

    def __init__(self, filters, n_range, device=None):
        filters = list(filters)
        sets = [[bytes(a) for a in f.addresses] for f in filters]
        tsets = [([[bytes(t) for t in (ts or ())] for ts in f.topics] + [[], [], [], []])[:4] for f in filters]
        if any(len(a) != 20 for s in sets for a in s) or any(len(t) != 32 for f in tsets for s in f for t in s) or any(len(list(f.topics)) > 4 for f in filters):
            raise ValueError("a filter's addresses are 20 bytes, its topics 32 bytes in at most four positions")
        addr, topic = [a for s in sets for a in s], [t for f in tsets for s in f for t in s]
        a = {"addr_first": np.cumsum([0] + [len(s) for s in sets]).astype(np.uint32), "addr": np.frombuffer(b"".join(addr), np.uint8),
             "topic_first": np.cumsum([0] + [len(s) for f in tsets for s in f]).astype(np.uint32), "topic": np.frombuffer(b"".join(topic), np.uint8),
             "block_lo": np.asarray([f.from_block or 0 for f in filters], np.uint32),
             "block_hi": np.asarray([n_range if f.to_block is None else f.to_block for f in filters], np.uint32)}
        if device is not None:
            import torch
            a = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).to(device) for k, v in a.items()}
            ptr = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
        else:
            ptr = lambda x: x.ctypes.data if x.size else None  # noqa: E731
        self.keep, self.n = a, len(filters)
        self.struct = L.PhantLogFilters(C.sizeof(L.PhantLogFilters), len(filters), len(addr), len(topic), *[ptr(a[name]) for name, _ in L.LOG_FILTER_ARRAYS], 0)


class LogMatches:
    """filter_logs' answer: `match_log` (the indices of the selected logs, ordered by filter and then by log), `filter_first`
    (n_filters + 1) and `filter_count`; logs(f) = the logs filter f selects, in chain order."""

    def __init__(self, filter_first, match_log, filter_count):
        self.filter_first, self.match_log, self.filter_count = filter_first, match_log, filter_count
        self.n_matches = len(match_log)

    def logs(self, f):
        return self.match_log[int(self.filter_first[f]):int(self.filter_first[f + 1])]


def filter_logs(segment_rows, filters, ctx: Context | None = None) -> LogMatches:
    """phant_block_log_filters: which logs of a chain segment each filter selects.  segment_rows: what receipt_segments(..., logs=True)
    returns (or a dict of its block_first, log_first, address, topic_first, topics), as host arrays or as torch tensors on the device --
    then the device form runs on them without a copy, and the answer's arrays are device tensors."""
    ctx = ctx or default_context()
    get = (lambda k: segment_rows[k]) if isinstance(segment_rows, dict) else (lambda k: getattr(segment_rows, k))
    try:
        rows = {name: get(name) for name, _ in L.LOGMATCH_INPUTS}
    except (KeyError, AttributeError):
        raise ValueError("filter_logs reads the per-log arrays: receipt_segments(..., logs=True)") from None
    dev = hasattr(rows["address"], "data_ptr")
    filters = list(filters)
    if dev:
        import torch
        device = rows["address"].device
        rows = {name: rows[name].contiguous().view(torch.uint8).view({"u4": torch.int32, "u1": torch.uint8}[dt]) for name, dt in L.LOGMATCH_INPUTS}
        count = lambda x: x.numel()  # noqa: E731
        ptr = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
        fn = ctx._lib.phant_block_log_filters_dev
    else:
        device = None
        rows = {name: np.ascontiguousarray(rows[name], dt) for name, dt in L.LOGMATCH_INPUTS}
        count = lambda x: x.size  # noqa: E731
        ptr = lambda x: x.ctypes.data if x.size else None  # noqa: E731
        fn = ctx._lib.phant_block_log_filters
    nb, n, nl, nt = count(rows["block_first"]) - 1, count(rows["log_first"]) - 1, count(rows["address"]) // 20, count(rows["topics"]) // 32
    nf = len(filters)
    packed = _PackedFilters(filters, nb, device)
    cap = min(nf * nl, max(1024, 4 * nl))
    while True:
        if dev:
            outs = {"filter_first": torch.zeros(nf + 1, dtype=torch.int32, device=device), "match_log": torch.zeros(cap, dtype=torch.int32, device=device),
                    "filter_count": torch.zeros(nf, dtype=torch.int32, device=device)}
        else:
            outs = {"filter_first": np.zeros(nf + 1, np.uint32), "match_log": np.zeros(cap, np.uint32), "filter_count": np.zeros(nf, np.uint32)}
        arg = L.PhantLogMatchIn(C.sizeof(L.PhantLogMatchIn), nb, n, nl, nt, cap, 0, 0,
                                *[rows[name].data_ptr() if dev else rows[name].ctypes.data for name in ("block_first", "log_first")], ptr(rows["address"]),
                                rows["topic_first"].data_ptr() if dev else rows["topic_first"].ctypes.data, ptr(rows["topics"]))
        if nb == 0:
            arg.block_first = arg.log_first = arg.topic_first = None
        out = L.PhantLogMatchOut(C.sizeof(L.PhantLogMatchOut), 0, 0, 0, *[ptr(outs[name]) for name in L.LOGMATCH_OUTPUTS])
        ctx.check(fn(ctx.handle, C.byref(arg), C.byref(packed.struct), C.byref(out)))
        nm = int(out.n_matches)
        if nm <= cap:
            break
        cap = nm  # (the counts were complete: once more with room for every row)
    if dev:
        torch.cuda.synchronize(device)
    return LogMatches(outs["filter_first"], outs["match_log"][:nm], outs["filter_count"])


def bloom_candidates(blooms, filters, ctx: Context | None = None):
    """phant_log_filters_bloom: which of the 2048-bit blooms (an (n, 256) uint8 array, 256-byte strings, or a uint8 tensor on the device)
    can hold a match of each filter; a filter's from_block / to_block index the blooms.  -> (may, may_count): may[f, b] a boolean
    (host form) or the packed words (n_filters, ceil(n / 64)) as an int64 tensor (device form); no false negatives."""
    ctx = ctx or default_context()
    filters = list(filters)
    nf = len(filters)
    if hasattr(blooms, "data_ptr"):
        import torch
        blooms = blooms.contiguous().view(torch.uint8).reshape(-1, 256)
        n, words = blooms.shape[0], (blooms.shape[0] + 63) // 64
        packed = _PackedFilters(filters, n, blooms.device)
        may = torch.zeros((nf, words), dtype=torch.int64, device=blooms.device)
        may_count = torch.zeros(nf, dtype=torch.int32, device=blooms.device)
        ctx.check(ctx._lib.phant_log_filters_bloom_dev(ctx.handle, blooms.data_ptr() if n else None, n, C.byref(packed.struct), may.data_ptr() if may.numel() else None,
                                                       may_count.data_ptr() if nf else None))
        return may, may_count
    b = blooms if isinstance(blooms, np.ndarray) else np.frombuffer(b"".join(bytes(x) for x in blooms), np.uint8)
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 256)
    n, words = len(b), (len(b) + 63) // 64
    packed = _PackedFilters(filters, n)
    may, may_count = np.zeros((nf, words), np.uint64), np.zeros(nf, np.uint32)
    ctx.check(ctx._lib.phant_log_filters_bloom(ctx.handle, b.ctypes.data if n else None, n, C.byref(packed.struct), may.ctypes.data if may.size else None,
                                               may_count.ctypes.data if nf else None))
    bits = np.unpackbits(may.view(np.uint8).reshape(nf, -1), axis=1, bitorder="little")[:, :n].astype(bool) if may.size else np.zeros((nf, n), bool)
    return bits, may_count
