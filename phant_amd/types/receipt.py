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
