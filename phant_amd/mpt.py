"""Mirror of phant's src/mpt/mpt.zig over the C-ABI, plus the batched proof
verifier the reference only has as a TODO
(src/engine_api/execution_payload.zig:177-178).

    KeyVal.init(key, value)            mpt.zig:13-34
    mptize(list[KeyVal]) -> Hash32     mpt.zig:38-45   (list must be sorted)
    empty_mpt_root                     mpt.zig:10
    index_root_rlp / index_root_be32   blockchain.zig:209-235 /
                                       execution_payload.zig:125-158
    verify_batch / verify_batch_dev    DESIGN.md section 3
    prove_nodeset / _packed / _dev     DESIGN.md section 7d (witness generation)
    prove_batch / _packed / _dev       DESIGN.md section 7d (per-proof form: eth_getProof)
    verify_ranges / prove_range        DESIGN.md section 7p (range proofs: snap sync's AccountRange / StorageRanges)
"""
from __future__ import annotations

from dataclasses import dataclass

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .context import Context, default_context, _np_ptr

empty_mpt_root = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")

PROOF_INVALID_EMPTY = L.PROOF_INVALID_EMPTY
PROOF_PRESENT = L.PROOF_PRESENT
PROOF_ABSENT = L.PROOF_ABSENT
PROOF_BAD_HASH = L.PROOF_BAD_HASH
PROOF_BAD_RLP = L.PROOF_BAD_RLP
PROOF_BAD_NODE = L.PROOF_BAD_NODE
PROOF_EXTRA_NODES = L.PROOF_EXTRA_NODES
PROOF_MISSING_NODE = L.PROOF_MISSING_NODE
PROOF_BAD_INPUT = L.PROOF_BAD_INPUT
PROVE_MAY_REMOVE = L.PROVE_MAY_REMOVE


class UnsortedError(ValueError):
    """mptize precondition (mpt.zig:39): keys strictly increasing."""


@dataclass(frozen=True)
class KeyVal:
    """mpt.zig:13-34.  `nibbles` is what KeyVal.init derives from the key bytes."""
    key: bytes
    value: bytes

    @staticmethod
    def init(key: bytes, value: bytes) -> "KeyVal":
        return KeyVal(bytes(key), bytes(value))

    @property
    def nibbles(self) -> bytes:
        out = bytearray()
        for b in self.key:
            out.append(b >> 4)
            out.append(b & 0x0F)
        return bytes(out)

    @staticmethod
    def less_than(a: "KeyVal", b: "KeyVal") -> bool:
        return a.nibbles < b.nibbles


def _pack(items, off_dtype):
    off = np.zeros(len(items) + 1, off_dtype)
    if items:
        off[1:] = np.cumsum([len(x) for x in items])
    blob = np.frombuffer(b"".join(items), np.uint8).copy() if items else np.zeros(0, np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, np.uint8)
    return blob, off


def mptize_packed(keys: np.ndarray, key_off: np.ndarray, vals: np.ndarray, val_off: np.ndarray,
                  ctx: Context | None = None) -> bytes:
    ctx = ctx or default_context()
    keys = np.ascontiguousarray(keys, np.uint8)
    key_off = np.ascontiguousarray(key_off, np.uint32)
    vals = np.ascontiguousarray(vals, np.uint8)
    val_off = np.ascontiguousarray(val_off, np.uint64)
    n = len(key_off) - 1
    out = np.zeros(32, np.uint8)
    rc = ctx._lib.phant_mpt_root(ctx.handle, _np_ptr(keys), _np_ptr(key_off), _np_ptr(vals), _np_ptr(val_off), n,
                                 _np_ptr(out))
    if rc == L.E_UNSORTED:
        raise UnsortedError("mptize: keys must be strictly increasing")
    ctx.check(rc)
    return out.tobytes()


def mptize(keyvals, ctx: Context | None = None) -> bytes:
    """Root hash of the MPT holding exactly `keyvals` (sorted by key)."""
    kb, ko = _pack([kv.key for kv in keyvals], np.uint32)
    vb, vo = _pack([kv.value for kv in keyvals], np.uint64)
    return mptize_packed(kb, ko, vb, vo, ctx)


def mptize_dev(keys: torch.Tensor, key_off: torch.Tensor, vals: torch.Tensor, val_off: torch.Tensor,
               out: torch.Tensor | None = None, ctx: Context | None = None) -> torch.Tensor:
    """mptize over device-resident packed arrays (phant_mpt_root_dev): keys u8[], key_off i32[n + 1], vals u8[],
    val_off i64[n + 1] -> root u8[32] on the device.  Keys strictly increasing (mpt.zig:39) else PHANT_E_UNSORTED."""
    ctx = ctx or default_context(keys.device.index)
    n = key_off.numel() - 1
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=keys.device)
    ctx.check(ctx._lib.phant_mpt_root_dev(ctx.handle, keys.data_ptr(), key_off.data_ptr(), keys.numel(), vals.data_ptr(),
                                          val_off.data_ptr(), vals.numel(), n, out.data_ptr()))
    return out


def pack_items(items):
    """-> (blob u8[], off u64[n + 1]): a list's encoded items back to back, the form phant_index_root_rlp / phant_block_roots take
    (and a compiled caller holds them in: src/blockchain/blockchain.zig:213-232 encodes every item into one buffer)."""
    return _pack([bytes(x) for x in items], np.uint64)


def index_root_rlp_packed(blob: np.ndarray, off: np.ndarray, ctx: Context | None = None) -> bytes:
    ctx = ctx or default_context()
    out = np.zeros(32, np.uint8)
    ctx.check(ctx._lib.phant_index_root_rlp(ctx.handle, _np_ptr(blob), _np_ptr(off), len(off) - 1, _np_ptr(out)))
    return out.tobytes()


def index_root_rlp(items, ctx: Context | None = None) -> bytes:
    """calculateMPTRoot (blockchain.zig:209-235): item i under key rlp(i)."""
    return index_root_rlp_packed(*pack_items(items), ctx)


def block_roots(lists, ctx: Context | None = None) -> list[bytes]:
    """Blockchain.validateBlock's roots (blockchain.zig:198-204: transactionsRoot, receiptsRoot, withdrawalsRoot) in ONE
    call: `lists` = the encoded items of every index-keyed trie of the block (key rlp(index), as index_root_rlp); all of
    them go through the trie hasher as one forest, so its level-by-level latency is paid once (phant_block_roots).
    -> one 32-byte root per list (empty_mpt_root for an empty one)."""
    return block_roots_packed([pack_items(items) for items in lists], ctx)


def block_roots_packed(packed, ctx: Context | None = None) -> list[bytes]:
    """block_roots over lists that are packed already: [(blob, off), ...] as pack_items returns them."""
    ctx = ctx or default_context()
    k = len(packed)
    item_p = (C.c_void_p * max(k, 1))(*[_np_ptr(b).value if b.size else None for b, _ in packed])
    off_p = (C.c_void_p * max(k, 1))(*[_np_ptr(o).value for _, o in packed])
    n = (C.c_uint32 * max(k, 1))(*[len(o) - 1 for _, o in packed])
    out = np.zeros(32 * max(k, 1), np.uint8)
    ctx.check(ctx._lib.phant_block_roots(ctx.handle, item_p, off_p, n, k, _np_ptr(out), None, None, None, 0, 0, None))
    return [out[32 * i:32 * i + 32].tobytes() for i in range(k)]


def index_root_be32(items, ctx: Context | None = None) -> bytes:
    """ExecutionPayload.toBlock (execution_payload.zig:125-158): 32-byte BE index keys."""
    ctx = ctx or default_context()
    blob, off = _pack([bytes(x) for x in items], np.uint64)
    out = np.zeros(32, np.uint8)
    ctx.check(ctx._lib.phant_index_root_be32(ctx.handle, _np_ptr(blob), _np_ptr(off), len(items), _np_ptr(out)))
    return out.tobytes()


def verify_batch(roots, root_idx, keys, key_len, nodes, node_off, proof_first_node, ctx: Context | None = None):
    """Host form.  numpy in -> (status u8[n], value_off u64[n], value_len u32[n])."""
    ctx = ctx or default_context()
    roots = np.ascontiguousarray(roots, np.uint8).reshape(-1)
    n_roots = roots.size // 32
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1)
    nodes_len = nodes.size
    if nodes.size == 0:
        nodes = np.zeros(1, np.uint8)
    if keys.size == 0:
        keys = np.zeros(1, np.uint8)
    node_off = np.ascontiguousarray(node_off, np.uint64)
    pfn = np.ascontiguousarray(proof_first_node, np.uint32)
    n = len(pfn) - 1
    ri = None if root_idx is None else np.ascontiguousarray(root_idx, np.uint32)
    status = np.zeros(max(n, 1), np.uint8)
    voff = np.zeros(max(n, 1), np.uint64)
    vlen = np.zeros(max(n, 1), np.uint32)
    ctx.check(ctx._lib.phant_mpt_verify_batch(
        ctx.handle, _np_ptr(roots), n_roots, None if ri is None else _np_ptr(ri), _np_ptr(keys), key_len,
        _np_ptr(nodes), nodes_len, _np_ptr(node_off), _np_ptr(pfn), n, _np_ptr(status), _np_ptr(voff),
        _np_ptr(vlen)))
    return status[:n], voff[:n], vlen[:n]


@dataclass
class ProofBatch:
    """A witness resident in HBM (all tensors on one device).

    roots (n_roots, 32) u8 | root_idx (n,) i32 or None | keys (n, key_len) u8 |
    nodes (nodes_len,) u8 | node_off (total_nodes+1,) i64 | proof_first_node (n+1,) i32
    """
    roots: torch.Tensor
    root_idx: torch.Tensor | None
    keys: torch.Tensor
    nodes: torch.Tensor
    node_off: torch.Tensor
    proof_first_node: torch.Tensor

    @property
    def n(self) -> int:
        return self.proof_first_node.numel() - 1

    @property
    def key_len(self) -> int:
        return self.keys.shape[1] if self.keys.dim() == 2 else 0

    @property
    def n_roots(self) -> int:
        return self.roots.numel() // 32

    def algorithmic_bytes(self) -> int:
        """node bytes + key bytes read, 1 status byte written per proof."""
        return int(self.nodes.numel() + self.keys.numel() + self.n)


def verify_batch_dev(b: ProofBatch, status: torch.Tensor | None = None, value_off: torch.Tensor | None = None,
                     value_len: torch.Tensor | None = None, ctx: Context | None = None,
                     fail_count: torch.Tensor | None = None) -> torch.Tensor:
    """Device form, asynchronous on the ctx stream.  Returns the status tensor.  With `fail_count`
    (int32[n_roots], device) the per-root verdict is produced in the same launch
    (phant_mpt_verify_verdict_dev)."""
    ctx = ctx or default_context(b.nodes.device.index)
    n = b.n
    dev = b.nodes.device
    assert b.nodes.dtype == torch.uint8 and b.node_off.dtype == torch.int64
    assert b.proof_first_node.dtype == torch.int32 and b.keys.dtype == torch.uint8 and b.roots.dtype == torch.uint8
    if b.root_idx is not None:
        assert b.root_idx.dtype == torch.int32
    if status is None:
        status = torch.empty(n, dtype=torch.uint8, device=dev)
    args = (ctx.handle, b.roots.data_ptr(), b.n_roots, None if b.root_idx is None else b.root_idx.data_ptr(),
            b.keys.data_ptr(), b.key_len, b.nodes.data_ptr(), b.nodes.numel(), b.node_off.data_ptr(),
            b.node_off.numel() - 1, b.proof_first_node.data_ptr(), n, status.data_ptr(),
            None if value_off is None else value_off.data_ptr(), None if value_len is None else value_len.data_ptr())
    if fail_count is None:
        ctx.check(ctx._lib.phant_mpt_verify_batch_dev(*args))
    else:
        assert fail_count.dtype == torch.int32 and fail_count.numel() >= b.n_roots
        ctx.check(ctx._lib.phant_mpt_verify_verdict_dev(*args, fail_count.data_ptr()))
    return status


def verdict_dev(status: torch.Tensor, root_idx: torch.Tensor | None, n_roots: int,
                out: torch.Tensor | None = None, ctx: Context | None = None) -> torch.Tensor:
    """fail_count[r] = number of proofs against root r that are not PRESENT/ABSENT (int32, device)."""
    ctx = ctx or default_context(status.device.index)
    if out is None:
        out = torch.empty(n_roots, dtype=torch.int32, device=status.device)
    ctx.check(ctx._lib.phant_mpt_verdict_dev(ctx.handle, status.data_ptr(),
                                             None if root_idx is None else root_idx.data_ptr(), status.numel(),
                                             n_roots, out.data_ptr()))
    return out


# ---------------------------------------------------------------------------- streaming (BASELINE config 5)
@dataclass
class HostWitness:
    """A witness in pinned host memory (what a block-processing loop holds after parsing the wire format),
    plus pinned result buffers.  All tensors are CPU tensors with pin_memory=True."""
    roots: torch.Tensor
    root_idx: torch.Tensor | None
    keys: torch.Tensor
    nodes: torch.Tensor
    node_off: torch.Tensor
    proof_first_node: torch.Tensor
    status: torch.Tensor
    value_off: torch.Tensor
    value_len: torch.Tensor

    @property
    def n(self) -> int:
        return self.proof_first_node.numel() - 1

    def h2d_bytes(self) -> int:
        t = [self.roots, self.keys, self.nodes, self.node_off, self.proof_first_node]
        if self.root_idx is not None:
            t.append(self.root_idx)
        return int(sum(x.numel() * x.element_size() for x in t))


def to_host(b: ProofBatch) -> HostWitness:
    """Copy a device-resident ProofBatch into pinned host buffers."""
    def pin(t):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t)
        return h

    n = b.n
    return HostWitness(pin(b.roots), None if b.root_idx is None else pin(b.root_idx), pin(b.keys), pin(b.nodes),
                       pin(b.node_off), pin(b.proof_first_node),
                       torch.empty(n, dtype=torch.uint8, pin_memory=True),
                       torch.empty(n, dtype=torch.int64, pin_memory=True),
                       torch.empty(n, dtype=torch.int32, pin_memory=True))


def verify_submit(hw: HostWitness, slot: int, ctx: Context | None = None) -> None:
    """phant_mpt_verify_submit: queue copy-in, verification and copy-out of `hw` on slot `slot`; returns at
    once.  hw.status / value_off / value_len are valid after wait(slot)."""
    ctx = ctx or default_context()
    key_len = hw.keys.shape[1] if hw.keys.dim() == 2 else 0
    ctx.check(ctx._lib.phant_mpt_verify_submit(
        ctx.handle, slot, hw.roots.data_ptr(), hw.roots.numel() // 32,
        None if hw.root_idx is None else hw.root_idx.data_ptr(), hw.keys.data_ptr(), key_len, hw.nodes.data_ptr(),
        hw.nodes.numel(), hw.node_off.data_ptr(), hw.proof_first_node.data_ptr(), hw.n, hw.status.data_ptr(),
        hw.value_off.data_ptr(), hw.value_len.data_ptr()))


def wait(slot: int, ctx: Context | None = None) -> None:
    ctx = ctx or default_context()
    ctx.check(ctx._lib.phant_wait(ctx.handle, slot))


# ---------------------------------------------------------------------------- node-set witnesses
def verify_nodeset(roots, root_idx, keys, key_len, nodes, node_off, ctx: Context | None = None):
    """Host form of phant_mpt_verify_nodeset: `nodes` / `node_off` are an unordered SET of trie nodes, every
    key is walked from its root with references resolved by hash.
    numpy in -> (status u8[n], value_off u64[n], value_len u32[n])."""
    ctx = ctx or default_context()
    roots = np.ascontiguousarray(roots, np.uint8).reshape(-1)
    n_roots = roots.size // 32
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1)
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1)
    nodes_len = nodes.size
    node_off = np.ascontiguousarray(node_off, np.uint64)
    total_nodes = len(node_off) - 1
    ri = None if root_idx is None else np.ascontiguousarray(root_idx, np.uint32)
    n = len(ri) if ri is not None else (keys.size // key_len if key_len else 0)
    if nodes.size == 0:
        nodes = np.zeros(1, np.uint8)
    if keys.size == 0:
        keys = np.zeros(1, np.uint8)
    status = np.zeros(max(n, 1), np.uint8)
    voff = np.zeros(max(n, 1), np.uint64)
    vlen = np.zeros(max(n, 1), np.uint32)
    ctx.check(ctx._lib.phant_mpt_verify_nodeset(
        ctx.handle, _np_ptr(roots), n_roots, None if ri is None else _np_ptr(ri), _np_ptr(keys), key_len,
        _np_ptr(nodes), nodes_len, _np_ptr(node_off), total_nodes, n, _np_ptr(status), _np_ptr(voff), _np_ptr(vlen)))
    return status[:n], voff[:n], vlen[:n]


def verify_nodeset_dev(roots: torch.Tensor, root_idx: torch.Tensor | None, keys: torch.Tensor, nodes: torch.Tensor,
                       node_off: torch.Tensor, status: torch.Tensor | None = None, ctx: Context | None = None,
                       value_off: torch.Tensor | None = None, value_len: torch.Tensor | None = None,
                       fail_count: torch.Tensor | None = None) -> torch.Tensor:
    """Device form, asynchronous on the ctx stream.  keys (n, key_len) u8, node_off (m + 1,) i64; value_off (n,) i64 and
    value_len (n,) i32 (optional outputs): where in `nodes` the proven value of a PRESENT key lies.  With `fail_count`
    (int32[n_roots], device) the per-root verdict comes out of the same launch (phant_mpt_verify_nodeset_verdict_dev)."""
    ctx = ctx or default_context(nodes.device.index)
    n = keys.shape[0]
    if status is None:
        status = torch.empty(n, dtype=torch.uint8, device=nodes.device)
    args = (ctx.handle, roots.data_ptr(), roots.numel() // 32, None if root_idx is None else root_idx.data_ptr(),
            keys.data_ptr(), keys.shape[1], nodes.data_ptr(), nodes.numel(), node_off.data_ptr(), node_off.numel() - 1, n,
            status.data_ptr(), None if value_off is None else value_off.data_ptr(),
            None if value_len is None else value_len.data_ptr())
    if fail_count is None:
        ctx.check(ctx._lib.phant_mpt_verify_nodeset_dev(*args))
    else:
        assert fail_count.dtype == torch.int32 and fail_count.numel() >= roots.numel() // 32
        ctx.check(ctx._lib.phant_mpt_verify_nodeset_verdict_dev(*args, fail_count.data_ptr()))
    return status


@dataclass
class NodeSet:
    """A node-set witness resident in HBM: what a block's execution witness is (src/engine_api/execution_payload.zig:121) --
    every trie node once, in any order, next to the keys it proves.

    roots (n_roots, 32) u8 | root_idx (n,) i32 or None | keys (n, key_len) u8 | nodes (nodes_len,) u8 | node_off (m + 1,) i64
    """
    roots: torch.Tensor
    root_idx: torch.Tensor | None
    keys: torch.Tensor
    nodes: torch.Tensor
    node_off: torch.Tensor

    @property
    def n(self) -> int:
        return self.keys.shape[0]

    @property
    def n_roots(self) -> int:
        return self.roots.numel() // 32

    @property
    def total_nodes(self) -> int:
        return self.node_off.numel() - 1

    def algorithmic_bytes(self) -> int:
        """node bytes + key bytes read, 1 status byte written per key"""
        return int(self.nodes.numel() + self.keys.numel() + self.n)


@dataclass
class HostNodeSet:
    """A NodeSet in pinned host memory, plus pinned result buffers (phant_mpt_verify_nodeset_submit)."""
    roots: torch.Tensor
    root_idx: torch.Tensor | None
    keys: torch.Tensor
    nodes: torch.Tensor
    node_off: torch.Tensor
    status: torch.Tensor
    value_off: torch.Tensor
    value_len: torch.Tensor

    @property
    def n(self) -> int:
        return self.keys.shape[0]

    def h2d_bytes(self) -> int:
        t = [self.roots, self.keys, self.nodes, self.node_off]
        if self.root_idx is not None:
            t.append(self.root_idx)
        return int(sum(x.numel() * x.element_size() for x in t))


def nodeset_to_host(s: NodeSet) -> HostNodeSet:
    def pin(t):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t)
        return h

    n = s.n
    return HostNodeSet(pin(s.roots), None if s.root_idx is None else pin(s.root_idx), pin(s.keys), pin(s.nodes), pin(s.node_off),
                       torch.empty(n, dtype=torch.uint8, pin_memory=True), torch.empty(n, dtype=torch.int64, pin_memory=True),
                       torch.empty(n, dtype=torch.int32, pin_memory=True))


def verify_nodeset_submit(hw: HostNodeSet, slot: int, ctx: Context | None = None) -> None:
    """phant_mpt_verify_nodeset_submit: queue copy-in, verification and copy-out of the node set on slot `slot`; returns at
    once.  hw.status / value_off / value_len are valid after wait(slot)."""
    ctx = ctx or default_context()
    key_len = hw.keys.shape[1] if hw.keys.dim() == 2 else 0
    ctx.check(ctx._lib.phant_mpt_verify_nodeset_submit(
        ctx.handle, slot, hw.roots.data_ptr(), hw.roots.numel() // 32,
        None if hw.root_idx is None else hw.root_idx.data_ptr(), hw.keys.data_ptr(), key_len, hw.nodes.data_ptr(),
        hw.nodes.numel(), hw.node_off.data_ptr(), hw.node_off.numel() - 1, hw.n, hw.status.data_ptr(),
        hw.value_off.data_ptr(), hw.value_len.data_ptr()))


# ---------------------------------------------------------------------------- witness generation
@dataclass
class ProvenNodeSet:
    """What phant_mpt_prove_nodeset emits (numpy, host): the hashed nodes on the paths of the queried keys, every position once,
    grouped by trie.  roots / nodes / node_off are what verify_nodeset takes; with root_idx = q_trie the queries verify against it.

    roots (n_tries, 32) u8 | nodes u8[nodes_len] | node_off u64[total_nodes + 1] | trie_first_node u32[n_tries + 1] |
    q_status u8[n_queries] (PROOF_PRESENT / PROOF_ABSENT)
    """
    roots: np.ndarray
    nodes: np.ndarray
    node_off: np.ndarray
    trie_first_node: np.ndarray
    q_status: np.ndarray

    @property
    def total_nodes(self) -> int:
        return len(self.node_off) - 1

    def node(self, j: int) -> bytes:
        return self.nodes[int(self.node_off[j]):int(self.node_off[j + 1])].tobytes()

    def trie_nodes(self, t: int) -> list[bytes]:
        """the nodes of trie t, in the order they were emitted"""
        return [self.node(j) for j in range(int(self.trie_first_node[t]), int(self.trie_first_node[t + 1]))]


def prove_nodeset_packed(keys, key_off, vals, val_off, seg_first, qkeys, qkey_off, q_trie=None, q_flags=None,
                         ctx: Context | None = None) -> ProvenNodeSet:
    """phant_mpt_prove_nodeset over packed arrays: the forest as mptize_packed takes a trie plus seg_first (u32[n_tries + 1], or
    None: one trie), the queries as a blob with offsets, q_trie (u32 per query, None with one trie) and q_flags (u8 per query,
    PROVE_MAY_REMOVE).  The first call guesses the capacities; if the set is larger the call is made once more with the sizes the
    first one reported."""
    ctx = ctx or default_context()
    keys = np.ascontiguousarray(keys, np.uint8)
    key_off = np.ascontiguousarray(key_off, np.uint32)
    vals = np.ascontiguousarray(vals, np.uint8)
    val_off = np.ascontiguousarray(val_off, np.uint64)
    n = len(key_off) - 1
    seg = None if seg_first is None else np.ascontiguousarray(seg_first, np.uint32)
    n_tries = 1 if seg is None else len(seg) - 1
    qkeys = np.ascontiguousarray(qkeys, np.uint8)
    qkey_off = np.ascontiguousarray(qkey_off, np.uint32)
    nq = len(qkey_off) - 1
    qt = None if q_trie is None else np.ascontiguousarray(q_trie, np.uint32)
    qf = None if q_flags is None else np.ascontiguousarray(q_flags, np.uint8)
    roots = np.zeros((max(n_tries, 1), 32), np.uint8)
    first = np.zeros(n_tries + 1, np.uint32)
    status = np.zeros(max(nq, 1), np.uint8)
    max_nodes, nodes_cap = 8 * nq + 64, (8 * nq + 64) * 256
    for attempt in (0, 1):
        nodes = np.zeros(max(nodes_cap, 1), np.uint8)
        node_off = np.zeros(max_nodes + 1, np.uint64)
        o = L.PhantProveOut(C.sizeof(L.PhantProveOut), max_nodes, nodes_cap, _np_ptr(nodes), _np_ptr(node_off), _np_ptr(first),
                            _np_ptr(roots), _np_ptr(status), 0, 0, 0)
        rc = ctx._lib.phant_mpt_prove_nodeset(ctx.handle, _np_ptr(keys), _np_ptr(key_off), _np_ptr(vals), _np_ptr(val_off), n,
                                              None if seg is None else _np_ptr(seg), n_tries, _np_ptr(qkeys), _np_ptr(qkey_off),
                                              None if qt is None else _np_ptr(qt), None if qf is None else _np_ptr(qf), nq, C.byref(o))
        if rc == L.E_UNSORTED:
            raise UnsortedError("prove_nodeset: keys must be strictly increasing inside every trie")
        ctx.check(rc)
        if o.total_nodes <= max_nodes and o.nodes_len <= nodes_cap:
            return ProvenNodeSet(roots[:n_tries], nodes[:o.nodes_len], node_off[:o.total_nodes + 1], first, status[:nq])
        max_nodes, nodes_cap = int(o.total_nodes), int(o.nodes_len)
    raise RuntimeError("prove_nodeset: the reported sizes did not hold on the second call")


def prove_nodeset(keyvals, queries, q_trie=None, q_flags=None, seg_first=None, ctx: Context | None = None) -> ProvenNodeSet:
    """The node set that proves `queries` (an iterable of key bytes) against the trie holding `keyvals` (sorted KeyVals) -- or, with
    seg_first, against a forest of tries laid end to end (q_trie says which).  -> ProvenNodeSet."""
    kb, ko = _pack([kv.key for kv in keyvals], np.uint32)
    vb, vo = _pack([kv.value for kv in keyvals], np.uint64)
    qb, qo = _pack([bytes(q) for q in queries], np.uint32)
    return prove_nodeset_packed(kb, ko, vb, vo, seg_first, qb, qo, q_trie, q_flags, ctx)


def prove_nodeset_dev(keys: torch.Tensor, key_off: torch.Tensor, vals: torch.Tensor, val_off: torch.Tensor,
                      seg_first: torch.Tensor | None, qkeys: torch.Tensor, qkey_off: torch.Tensor, q_trie: torch.Tensor | None,
                      q_flags: torch.Tensor | None, nodes: torch.Tensor | None, node_off: torch.Tensor | None,
                      trie_first_node: torch.Tensor | None = None, roots: torch.Tensor | None = None,
                      q_status: torch.Tensor | None = None, ctx: Context | None = None) -> tuple[int, int]:
    """phant_mpt_prove_nodeset_dev: every tensor device-resident (keys u8, key_off i32[n + 1], vals u8, val_off i64[n + 1],
    seg_first i32[n_tries + 1] or None, qkeys u8, qkey_off i32[nq + 1], q_trie i32[nq] or None, q_flags u8[nq] or None; outputs
    nodes u8[cap], node_off i64[max_nodes + 1], trie_first_node i32, roots u8, q_status u8, each optional).
    -> (total_nodes, nodes_len); nodes / node_off are valid only if both fit."""
    ctx = ctx or default_context(keys.device.index)
    n, nq = key_off.numel() - 1, qkey_off.numel() - 1
    n_tries = 1 if seg_first is None else seg_first.numel() - 1
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    o = L.PhantProveOut(C.sizeof(L.PhantProveOut), 0 if node_off is None else node_off.numel() - 1,
                        0 if nodes is None else nodes.numel(), ptr(nodes), ptr(node_off), ptr(trie_first_node), ptr(roots),
                        ptr(q_status), 0, 0, 0)
    ctx.check(ctx._lib.phant_mpt_prove_nodeset_dev(ctx.handle, keys.data_ptr(), key_off.data_ptr(), keys.numel(), vals.data_ptr(),
                                                   val_off.data_ptr(), vals.numel(), n, ptr(seg_first), n_tries, qkeys.data_ptr(),
                                                   qkey_off.data_ptr(), qkeys.numel(), ptr(q_trie), ptr(q_flags), nq, C.byref(o)))
    return int(o.total_nodes), int(o.nodes_len)


@dataclass
class ProvenBatch:
    """What phant_mpt_prove_batch emits (numpy, host): an ordered node list per query, root first, the lists back to back in query
    order.  (roots, root_idx = q_trie, nodes, node_off, proof_first_node) are what verify_batch takes.

    roots (n_tries, 32) u8 | nodes u8[nodes_len] | node_off u64[total_nodes + 1] | proof_first_node u32[n_queries + 1] |
    q_status u8[n_queries] (PROOF_PRESENT / PROOF_ABSENT)
    """
    roots: np.ndarray
    nodes: np.ndarray
    node_off: np.ndarray
    proof_first_node: np.ndarray
    q_status: np.ndarray

    @property
    def total_nodes(self) -> int:
        return len(self.node_off) - 1

    @property
    def n_queries(self) -> int:
        return len(self.proof_first_node) - 1

    def node(self, k: int) -> bytes:
        return self.nodes[int(self.node_off[k]):int(self.node_off[k + 1])].tobytes()

    def proof(self, j: int) -> list[bytes]:
        """the proof of query j: its nodes, root first"""
        return [self.node(k) for k in range(int(self.proof_first_node[j]), int(self.proof_first_node[j + 1]))]


def prove_batch_packed(keys, key_off, vals, val_off, seg_first, qkeys, qkey_off, q_trie=None, ctx: Context | None = None) -> ProvenBatch:
    """phant_mpt_prove_batch over packed arrays: the forest and the queries as prove_nodeset_packed takes them (no q_flags).  The
    first call guesses the capacities; if the proofs are larger the call is made once more with the sizes the first one reported."""
    ctx = ctx or default_context()
    keys = np.ascontiguousarray(keys, np.uint8)
    key_off = np.ascontiguousarray(key_off, np.uint32)
    vals = np.ascontiguousarray(vals, np.uint8)
    val_off = np.ascontiguousarray(val_off, np.uint64)
    n = len(key_off) - 1
    seg = None if seg_first is None else np.ascontiguousarray(seg_first, np.uint32)
    n_tries = 1 if seg is None else len(seg) - 1
    qkeys = np.ascontiguousarray(qkeys, np.uint8)
    qkey_off = np.ascontiguousarray(qkey_off, np.uint32)
    nq = len(qkey_off) - 1
    qt = None if q_trie is None else np.ascontiguousarray(q_trie, np.uint32)
    roots = np.zeros((max(n_tries, 1), 32), np.uint8)
    first = np.zeros(nq + 1, np.uint32)
    status = np.zeros(max(nq, 1), np.uint8)
    max_nodes, nodes_cap = 8 * nq + 64, (8 * nq + 64) * 256
    for attempt in (0, 1):
        nodes = np.zeros(max(nodes_cap, 1), np.uint8)
        node_off = np.zeros(max_nodes + 1, np.uint64)
        o = L.PhantProveBatchOut(C.sizeof(L.PhantProveBatchOut), max_nodes, nodes_cap, _np_ptr(nodes), _np_ptr(node_off), _np_ptr(first),
                                 _np_ptr(roots), _np_ptr(status), 0, 0, 0)
        rc = ctx._lib.phant_mpt_prove_batch(ctx.handle, _np_ptr(keys), _np_ptr(key_off), _np_ptr(vals), _np_ptr(val_off), n,
                                            None if seg is None else _np_ptr(seg), n_tries, _np_ptr(qkeys), _np_ptr(qkey_off),
                                            None if qt is None else _np_ptr(qt), nq, C.byref(o))
        if rc == L.E_UNSORTED:
            raise UnsortedError("prove_batch: keys must be strictly increasing inside every trie")
        ctx.check(rc)
        if o.total_nodes <= max_nodes and o.nodes_len <= nodes_cap:
            return ProvenBatch(roots[:n_tries], nodes[:o.nodes_len], node_off[:o.total_nodes + 1], first, status[:nq])
        max_nodes, nodes_cap = int(o.total_nodes), int(o.nodes_len)
    raise RuntimeError("prove_batch: the reported sizes did not hold on the second call")


def prove_batch(keyvals, queries, q_trie=None, seg_first=None, ctx: Context | None = None) -> ProvenBatch:
    """An eth_getProof-shaped proof per query (an iterable of key bytes) against the trie holding `keyvals` (sorted KeyVals) -- or,
    with seg_first, against a forest of tries laid end to end (q_trie says which).  -> ProvenBatch."""
    kb, ko = _pack([kv.key for kv in keyvals], np.uint32)
    vb, vo = _pack([kv.value for kv in keyvals], np.uint64)
    qb, qo = _pack([bytes(q) for q in queries], np.uint32)
    return prove_batch_packed(kb, ko, vb, vo, seg_first, qb, qo, q_trie, ctx)


def prove_batch_dev(keys: torch.Tensor, key_off: torch.Tensor, vals: torch.Tensor, val_off: torch.Tensor,
                    seg_first: torch.Tensor | None, qkeys: torch.Tensor, qkey_off: torch.Tensor, q_trie: torch.Tensor | None,
                    nodes: torch.Tensor | None, node_off: torch.Tensor | None, proof_first_node: torch.Tensor | None = None,
                    roots: torch.Tensor | None = None, q_status: torch.Tensor | None = None,
                    ctx: Context | None = None) -> tuple[int, int]:
    """phant_mpt_prove_batch_dev: every tensor device-resident (the forest and the queries as prove_nodeset_dev takes them; outputs
    nodes u8[cap], node_off i64[max_nodes + 1], proof_first_node i32[nq + 1], roots u8, q_status u8, each optional).
    -> (total_nodes, nodes_len); nodes / node_off / proof_first_node are valid only if both fit."""
    ctx = ctx or default_context(keys.device.index)
    n, nq = key_off.numel() - 1, qkey_off.numel() - 1
    n_tries = 1 if seg_first is None else seg_first.numel() - 1
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    o = L.PhantProveBatchOut(C.sizeof(L.PhantProveBatchOut), 0 if node_off is None else node_off.numel() - 1,
                             0 if nodes is None else nodes.numel(), ptr(nodes), ptr(node_off), ptr(proof_first_node), ptr(roots),
                             ptr(q_status), 0, 0, 0)
    ctx.check(ctx._lib.phant_mpt_prove_batch_dev(ctx.handle, keys.data_ptr(), key_off.data_ptr(), keys.numel(), vals.data_ptr(),
                                                 val_off.data_ptr(), vals.numel(), n, ptr(seg_first), n_tries, qkeys.data_ptr(),
                                                 qkey_off.data_ptr(), qkeys.numel(), ptr(q_trie), nq, C.byref(o)))
    return int(o.total_nodes), int(o.nodes_len)


# ---------------------------------------------------------------------------- range proofs
@dataclass
class Range:
    """One range of a verify_ranges call: the trusted root, the origin (32 bytes; ignored without a proof), the sorted run of
    (key, value) leaves, and whether the call's node set holds the proofs of its two edges."""
    root: bytes
    origin: bytes
    leaves: list
    has_proof: bool = True


@dataclass
class RangesResult:
    """What phant_mpt_verify_ranges answers (numpy, host), one row per range: status u8 (RANGE_* / PROOF_MISSING_NODE /
    PROOF_BAD_NODE), has_more u8, computed_root (n, 32) u8 (zeros on failure), bad_leaf u32 (the call-wide index of the least leaf
    that breaks a rule, else RANGE_NO_LEAF); n_failed, first_failed (n: none)."""
    status: np.ndarray
    has_more: np.ndarray
    computed_root: np.ndarray
    bad_leaf: np.ndarray
    n_failed: int
    first_failed: int

    def valid(self, r: int) -> bool:
        return int(self.status[r]) == L.RANGE_VALID


def pack_ranges(ranges, nodes):
    """ranges: Range objects (or (root, origin, leaves, has_proof) tuples); nodes: the node set, a list of encodings -> the arrays of
    phant_ranges_in as numpy, in the order of L.RANGES_INPUTS"""
    rs = [r if isinstance(r, Range) else Range(*r) for r in ranges]
    n = len(rs)
    roots = np.frombuffer(b"".join(bytes(r.root) for r in rs), np.uint8).copy().reshape(n, 32) if n else np.zeros((0, 32), np.uint8)
    origins = np.frombuffer(b"".join(bytes(r.origin or bytes(32)) for r in rs), np.uint8).copy().reshape(n, 32) if n else np.zeros((0, 32), np.uint8)
    leaf_first = np.zeros(n + 1, np.uint32)
    leaf_first[1:] = np.cumsum([len(r.leaves) for r in rs]) if n else []
    has_proof = np.array([1 if r.has_proof else 0 for r in rs], np.uint8)
    leaves = [kv for r in rs for kv in r.leaves]
    for k, _ in leaves:
        if len(k) != 32:
            raise ValueError("verify_ranges: keys are 32 bytes")
    keys = np.frombuffer(b"".join(bytes(k) for k, _ in leaves), np.uint8).copy()
    vals, val_off = _pack([bytes(v) for _, v in leaves], np.uint64)
    nb, node_off = _pack([bytes(x) for x in nodes], np.uint64)
    return roots, origins, leaf_first, has_proof, keys, vals[:int(val_off[-1])], val_off, nb[:int(node_off[-1])], node_off


def verify_ranges_packed(roots, origins, leaf_first, has_proof, keys, vals, val_off, nodes, node_off, ctx: Context | None = None) -> RangesResult:
    """Host form of phant_mpt_verify_ranges over packed numpy arrays (include/phant_gpu.h has the contract)."""
    ctx = ctx or default_context()
    arrays = [np.ascontiguousarray(a, dt).reshape(-1) for a, dt in zip(
        (roots, origins, leaf_first, has_proof, keys, vals, val_off, nodes, node_off),
        (np.uint8, np.uint8, np.uint32, np.uint8, np.uint8, np.uint8, np.uint64, np.uint8, np.uint64))]
    n, n_leaves, n_nodes = len(arrays[2]) - 1, len(arrays[6]) - 1, len(arrays[8]) - 1
    i = L.PhantRangesIn(C.sizeof(L.PhantRangesIn), n, n_leaves, n_nodes, (C.c_uint32 * 2)(0, 0), arrays[5].size, arrays[7].size,
                        *[_np_ptr(a) if a.size else None for a in arrays])
    outs = {name: np.zeros((max(n, 1), w) if w > 1 else max(n, 1), dt) for name, dt, w in L.RANGES_OUTPUTS}
    o = L.PhantRangesOut(C.sizeof(L.PhantRangesOut), 0, 0, (C.c_uint32 * 2)(0, 0), *[_np_ptr(outs[name]) for name, _, _ in L.RANGES_OUTPUTS])
    ctx.check(ctx._lib.phant_mpt_verify_ranges(ctx.handle, C.byref(i), C.byref(o)))
    return RangesResult(outs["status"][:n], outs["has_more"][:n], outs["computed_root"][:n], outs["bad_leaf"][:n], int(o.n_failed), int(o.first_failed))


def verify_ranges(ranges, nodes, ctx: Context | None = None) -> RangesResult:
    """Are the leaves of every range exactly what the trie under its root holds between its origin and its last key -- and does
    anything lie to the right (has_more)?  ranges: Range objects; nodes: ONE node set for all of them (a list of node encodings, any
    order, unrelated nodes allowed).  -> RangesResult."""
    return verify_ranges_packed(*pack_ranges(ranges, nodes), ctx=ctx)


def verify_ranges_dev(roots: torch.Tensor, origins: torch.Tensor, leaf_first: torch.Tensor, has_proof: torch.Tensor, keys: torch.Tensor,
                      vals: torch.Tensor, val_off: torch.Tensor, nodes: torch.Tensor, node_off: torch.Tensor, status: torch.Tensor | None = None,
                      has_more: torch.Tensor | None = None, computed_root: torch.Tensor | None = None, bad_leaf: torch.Tensor | None = None,
                      ctx: Context | None = None):
    """Device form: every array a device tensor (u8 but leaf_first / bad_leaf: int32 storage of uint32, val_off / node_off: int64
    storage of uint64).  Outputs that are None are not asked for.  -> (n_failed, first_failed)."""
    ctx = ctx or default_context()
    n, n_leaves, n_nodes = leaf_first.numel() - 1, val_off.numel() - 1, node_off.numel() - 1
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    i = L.PhantRangesIn(C.sizeof(L.PhantRangesIn), n, n_leaves, n_nodes, (C.c_uint32 * 2)(0, 0), vals.numel(), nodes.numel(),
                        ptr(roots), ptr(origins), ptr(leaf_first), ptr(has_proof), ptr(keys), ptr(vals), ptr(val_off), ptr(nodes), ptr(node_off))
    o = L.PhantRangesOut(C.sizeof(L.PhantRangesOut), 0, 0, (C.c_uint32 * 2)(0, 0), ptr(status), ptr(has_more), ptr(computed_root), ptr(bad_leaf))
    ctx.check(ctx._lib.phant_mpt_verify_ranges_dev(ctx.handle, C.byref(i), C.byref(o)))
    return int(o.n_failed), int(o.first_failed)


@dataclass
class ProvenRange:
    """What prove_range serves: the leaves from the first key >= origin on, the node set that proves the two edges (empty without a
    proof) and the trie's root.  Range(root, origin, leaves, has_proof) + nodes is what verify_ranges takes."""
    root: bytes
    origin: bytes
    leaves: list
    nodes: list
    has_proof: bool

    def range(self) -> Range:
        return Range(self.root, self.origin, self.leaves, self.has_proof)


def prove_range(keyvals, origin: bytes, limit: bytes | None = None, max_leaves: int | None = None, ctx: Context | None = None) -> ProvenRange:
    """The serving side of a range proof over the trie holding `keyvals` (sorted KeyVals with 32-byte keys): the leaves from the first
    key >= origin on, none beyond `limit` and at most max_leaves of them; with them the node set of
    prove_nodeset over {origin, the last key served} -- over {origin} alone when nothing is served -- or no proof at all when the
    slice is the whole trie and origin is zero."""
    import bisect
    origin = bytes(origin)
    keys = [kv.key for kv in keyvals]
    lo = bisect.bisect_left(keys, origin)
    hi = len(keys)
    if limit is not None:
        hi = max(lo, bisect.bisect_right(keys, bytes(limit)))
    if max_leaves is not None:
        hi = min(hi, lo + max_leaves)
    leaves = [(kv.key, kv.value) for kv in keyvals[lo:hi]]
    if lo == 0 and hi == len(keys) and origin == bytes(32):
        return ProvenRange(mptize(keyvals, ctx) if keyvals else empty_mpt_root, origin, leaves, [], False)
    if not keyvals:
        return ProvenRange(empty_mpt_root, origin, [], [], True)
    queries = [origin] + ([leaves[-1][0]] if leaves and leaves[-1][0] != origin else [])
    s = prove_nodeset(keyvals, queries, ctx=ctx)
    return ProvenRange(s.roots[0].tobytes(), origin, leaves, [s.node(j) for j in range(s.total_nodes)], True)
