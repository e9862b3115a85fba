"""The pre-state of a block out of an execution witness as stateless clients exchange it -- the step phant's
newPayloadV2Handler (src/engine_api/execution_payload.zig:175-181) leaves open before `runBlock`, which needs
`StateDB.init(allocator, accounts)` (src/state/statedb.zig:32).

The document declares nothing; every value comes out of the proofs (include/phant_gpu.h, execution-witness section):

    { "state": ["0x<rlp node>", ...], "codes": ["0x<bytecode>", ...], "keys": ["0x<address>" | "0x<address ++ slot>", ...] }

    w = StatelessWitness.parse_json(text)                # host-only (no GPU needed)
    pre = w.prestate(ctx, parent_state_root)            # the GPU: one call, one synchronisation
    pre.ok, pre.accounts                                # -> state.AccountState list for StateDB.init
    pre = new_payload_prestate(text, parent_state_root) # the hook: raises unless every proof holds
    post = w.poststate(ctx, parent_state_root, accounts_after)         # the state root after the block's writes
    post, nxt = w.advance(ctx, parent_state_root, accounts_after)      # ... and the witness of the NEXT block (its nodes: the post-state's)
    posts = new_payload_chain(text, parent_state_root, [(accounts_after, header_state_root), ...])  # k blocks, one witness
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .context import Context, default_context
from .state import AccountState

PROOF_BAD_VALUE = L.PROOF_BAD_VALUE
PROOF_MISSING_SIBLING = L.PROOF_MISSING_SIBLING
POST_KEEP, POST_SET, POST_DELETE = L.POST_KEEP, L.POST_SET, L.POST_DELETE
CODE_NONE = L.CODE_NONE


class ExecWitnessInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_accounts", C.c_uint32), ("n_slots", C.c_uint32), ("n_codes", C.c_uint32),
                ("total_nodes", C.c_uint32), ("nodes_len", C.c_uint64), ("code_bytes", C.c_uint64),
                ("addresses", C.c_void_p), ("slot_first", C.c_void_p), ("slots", C.c_void_p), ("codes", C.c_void_p),
                ("code_off", C.c_void_p), ("nodes", C.c_void_p), ("node_off", C.c_void_p)]


class PrestateOut(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("account_status", C.c_void_p), ("nonces", C.c_void_p), ("balances", C.c_void_p),
                ("storage_roots", C.c_void_p), ("code_hashes", C.c_void_p), ("code_index", C.c_void_p),
                ("slot_status", C.c_void_p), ("slot_vals", C.c_void_p), ("n_failed", C.c_uint32),
                ("n_missing_code", C.c_uint32), ("n_unused_codes", C.c_uint32)]


class WitnessFormatError(ValueError):
    pass


class PrestateError(RuntimeError):
    def __init__(self, msg: str, prestate: "PreState"):
        super().__init__(msg)
        self.prestate = prestate


def _view(ptr, count, dtype):
    if not count or not ptr:
        return np.zeros(0, dtype)
    n = count * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=dtype, count=count)


@dataclass
class PreState:
    """What phant_exec_witness_prestate proved.  accounts: the PRESENT accounts as state.AccountState (code by code_index,
    only the non-zero slots in storage), in witness order; absent: the addresses proven absent."""
    accounts: list
    absent: list
    addresses: list
    account_status: np.ndarray
    slot_status: np.ndarray
    nonces: np.ndarray
    balances: np.ndarray
    storage_roots: np.ndarray
    code_hashes: np.ndarray
    code_index: np.ndarray
    slot_vals: np.ndarray
    n_failed: int
    n_missing_code: int
    n_unused_codes: int
    missing_code: list = field(default_factory=list)  # addresses of PRESENT accounts whose code the witness does not carry

    @property
    def ok(self) -> bool:
        return self.n_failed == 0


class StatelessWitness:
    def __init__(self, handle):
        self._h = handle
        self._lib = L.lib()

    @staticmethod
    def parse_json(text: str | bytes) -> "StatelessWitness":
        lib = L.lib()
        data = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        rc = lib.phant_exec_witness_parse_json(data, len(data), C.byref(h), err, 256)
        if rc != L.OK:
            raise WitnessFormatError(err.value.decode() or f"phant_exec_witness_parse_json rc={rc}")
        return StatelessWitness(h)

    def info(self) -> dict:
        """numpy views (valid while this object lives) of the parsed arrays + counts."""
        wi = ExecWitnessInfo()
        wi.struct_size = C.sizeof(ExecWitnessInfo)
        rc = self._lib.phant_exec_witness_get(self._h, C.byref(wi))
        if rc != L.OK:
            raise L.PhantError(rc, "phant_exec_witness_get")
        return {"n_accounts": wi.n_accounts, "n_slots": wi.n_slots, "n_codes": wi.n_codes, "total_nodes": wi.total_nodes,
                "nodes_len": wi.nodes_len, "code_bytes": wi.code_bytes,
                "addresses": _view(wi.addresses, wi.n_accounts * 20, np.uint8).reshape(-1, 20),
                "slot_first": _view(wi.slot_first, wi.n_accounts + 1, np.uint32),
                "slots": _view(wi.slots, wi.n_slots * 32, np.uint8).reshape(-1, 32),
                "codes": _view(wi.codes, wi.code_bytes, np.uint8), "code_off": _view(wi.code_off, wi.n_codes + 1, np.uint64),
                "nodes": _view(wi.nodes, wi.nodes_len, np.uint8), "node_off": _view(wi.node_off, wi.total_nodes + 1, np.uint64)}

    def prestate_arrays(self, ctx: Context | None, state_root: bytes) -> dict:
        """The raw outputs of phant_exec_witness_prestate (numpy arrays + the three counts)."""
        ctx = ctx or default_context()
        if state_root is None or len(state_root) != 32:
            raise ValueError("state_root must be the 32-byte state root the caller trusts")
        i = self.info()
        na, ns = i["n_accounts"], i["n_slots"]
        r = {"account_status": np.zeros(max(na, 1), np.uint8), "nonces": np.zeros(max(na, 1), np.uint64),
             "balances": np.zeros((max(na, 1), 32), np.uint8), "storage_roots": np.zeros((max(na, 1), 32), np.uint8),
             "code_hashes": np.zeros((max(na, 1), 32), np.uint8), "code_index": np.zeros(max(na, 1), np.uint32),
             "slot_status": np.zeros(max(ns, 1), np.uint8), "slot_vals": np.zeros((max(ns, 1), 32), np.uint8)}
        o = PrestateOut()
        o.struct_size = C.sizeof(PrestateOut)
        for k, a in r.items():
            setattr(o, k, a.ctypes.data)
        root = C.create_string_buffer(bytes(state_root), 32)
        ctx.check(self._lib.phant_exec_witness_prestate(ctx.handle, self._h, root, C.byref(o)))
        out = {k: a[:na] if k not in ("slot_status", "slot_vals") else a[:ns] for k, a in r.items()}
        out.update(n_failed=int(o.n_failed), n_missing_code=int(o.n_missing_code), n_unused_codes=int(o.n_unused_codes))
        return out

    def prestate(self, ctx: Context | None, state_root: bytes) -> PreState:
        r = self.prestate_arrays(ctx, state_root)
        i = self.info()
        addrs = [bytes(a) for a in i["addresses"]]
        first, slots = i["slot_first"], i["slots"]
        codes, code_off = i["codes"], i["code_off"]
        accounts, absent, missing = [], [], []
        for k, addr in enumerate(addrs):
            st = int(r["account_status"][k])
            if st == L.PROOF_ABSENT:
                absent.append(addr)
                continue
            if st != L.PROOF_PRESENT:
                continue
            ci = int(r["code_index"][k])
            code = b"" if ci == CODE_NONE else codes[int(code_off[ci]):int(code_off[ci + 1])].tobytes()
            if ci == CODE_NONE and r["code_hashes"][k].tobytes() != _EMPTY_CODE:
                missing.append(addr)
            storage = {}
            for j in range(int(first[k]), int(first[k + 1])):
                v = int.from_bytes(r["slot_vals"][j].tobytes(), "big")
                if r["slot_status"][j] == L.PROOF_PRESENT and v:
                    storage[int.from_bytes(slots[j].tobytes(), "big")] = v
            accounts.append(AccountState(addr=addr, nonce=int(r["nonces"][k]),
                                         balance=int.from_bytes(r["balances"][k].tobytes(), "big"), code=code, storage=storage))
        return PreState(accounts=accounts, absent=absent, addresses=addrs, account_status=r["account_status"],
                        slot_status=r["slot_status"], nonces=r["nonces"], balances=r["balances"],
                        storage_roots=r["storage_roots"], code_hashes=r["code_hashes"], code_index=r["code_index"],
                        slot_vals=r["slot_vals"], n_failed=r["n_failed"], n_missing_code=r["n_missing_code"],
                        n_unused_codes=r["n_unused_codes"], missing_code=missing)

    def to_json(self) -> str:
        """The document parse_json reads back to the same object: state / codes / keys, each account's address followed by its
        address ++ slot keys, in this object's own order."""
        import json
        i = self.info()
        nodes, off = i["nodes"].tobytes(), i["node_off"]
        codes, coff = i["codes"].tobytes(), i["code_off"]
        keys = []
        for k, addr in enumerate(bytes(a) for a in i["addresses"]):
            keys.append("0x" + addr.hex())
            keys += ["0x" + (addr + i["slots"][j].tobytes()).hex() for j in range(int(i["slot_first"][k]), int(i["slot_first"][k + 1]))]
        return json.dumps({"state": ["0x" + nodes[int(off[j]):int(off[j + 1])].hex() for j in range(i["total_nodes"])],
                           "codes": ["0x" + codes[int(coff[j]):int(coff[j + 1])].hex() for j in range(i["n_codes"])], "keys": keys})

    def close(self):
        if getattr(self, "_h", None):
            self._lib.phant_exec_witness_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_witness(accounts, keys, may_remove=(), ctx: Context | None = None) -> StatelessWitness:
    """phant_state_witness: the execution witness of `keys` (20-byte addresses, 52-byte address ++ slot) cut from the state
    `accounts` (AccountState list) on the GPU; keys also in `may_remove` carry PHANT_PROVE_MAY_REMOVE, so that the witness holds
    what phant_exec_witness_poststate needs when the block removes them.  The state root is left in `.state_root`."""
    from .context import _np_ptr
    from .state import _soa
    ctx = ctx or default_context()
    n, arrays = _soa(accounts)
    keys = [bytes(k) for k in keys]
    flagged = {bytes(k) for k in may_remove}
    blob = np.frombuffer(b"".join(keys), np.uint8).copy() if keys and sum(map(len, keys)) else np.zeros(1, np.uint8)
    off = np.zeros(len(keys) + 1, np.uint32)
    if keys:
        off[1:] = np.cumsum([len(k) for k in keys])
    flags = np.array([L.PROVE_MAY_REMOVE if k in flagged else 0 for k in keys] or [0], np.uint8)
    h = C.c_void_p()
    root = np.zeros(32, np.uint8)
    ctx.check(ctx._lib.phant_state_witness(ctx.handle, *[_np_ptr(a) for a in arrays], n, _np_ptr(blob), _np_ptr(off),
                                           _np_ptr(flags) if flagged else None, len(keys), C.byref(h), _np_ptr(root)))
    w = StatelessWitness(h)
    w.state_root = root.tobytes()
    return w


_EMPTY_CODE = bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")


def new_payload_prestate(witness_json: str | bytes, parent_state_root: bytes, ctx: Context | None = None) -> PreState:
    """The hook newPayloadV2Handler (execution_payload.zig:175-181) would call before `runBlock`: the pre-state the block runs
    on, proven against `parent_state_root` -- the parent header's state root the node already trusts.  Raises
    WitnessFormatError for a malformed document and PrestateError (carrying the PreState) when any proof fails; a code the
    witness does not carry is not a failure here (pre.missing_code: the caller decides)."""
    w = StatelessWitness.parse_json(witness_json)
    try:
        pre = w.prestate(ctx, parent_state_root)
    finally:
        w.close()
    if not pre.ok:
        raise PrestateError(f"execution witness: {pre.n_failed} account / slot proofs failed against the parent state root", pre)
    return pre


# ------------------------------------------------------------------------------------------------ the post-state root
class PoststateIO(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("account_op", C.c_void_p), ("nonces", C.c_void_p), ("balances", C.c_void_p),
                ("code_hashes", C.c_void_p), ("slot_write", C.c_void_p), ("slot_vals", C.c_void_p), ("state_root", C.c_void_p),
                ("storage_roots", C.c_void_p), ("account_status", C.c_void_p), ("slot_status", C.c_void_p),
                ("n_failed", C.c_uint32)]


class PoststateError(RuntimeError):
    def __init__(self, msg: str, poststate: "PostState"):
        super().__init__(msg)
        self.poststate = poststate


@dataclass
class PostState:
    """What phant_exec_witness_poststate computed: the state root after the block's writes (zero when a proof failed), the post
    storage roots and the statuses, in witness order."""
    root: bytes
    storage_roots: np.ndarray
    account_status: np.ndarray
    slot_status: np.ndarray
    n_failed: int

    @property
    def ok(self) -> bool:
        return self.n_failed == 0


def _poststate_arrays(self, ctx: Context | None, parent_root: bytes, writes: dict, advance: int | None = None):
    """The raw call (advance = the flags of phant_exec_witness_advance: that call instead, -> (dict, next witness or None)).  writes: account_op (n_accounts, POST_KEEP / POST_SET / POST_DELETE), nonces, balances (n x 32), code_hashes
    (n x 32) -- read where op == SET --, slot_write (n_slots, or None) and slot_vals (n_slots x 32), all in witness order."""
    ctx = ctx or default_context()
    if parent_root is None or len(parent_root) != 32:
        raise ValueError("parent_root must be the 32-byte state root the caller trusts")
    i = self.info()
    na, ns = i["n_accounts"], i["n_slots"]

    def arr(name, dtype, shape):
        a = writes.get(name)
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{name}: expected {shape}, got {a.shape}")
        return a

    ins = {"account_op": arr("account_op", np.uint8, (na,)), "nonces": arr("nonces", np.uint64, (na,)),
           "balances": arr("balances", np.uint8, (na, 32)), "code_hashes": arr("code_hashes", np.uint8, (na, 32)),
           "slot_write": arr("slot_write", np.uint8, (ns,)), "slot_vals": arr("slot_vals", np.uint8, (ns, 32))}
    outs = {"state_root": np.zeros(32, np.uint8), "storage_roots": np.zeros((max(na, 1), 32), np.uint8),
            "account_status": np.zeros(max(na, 1), np.uint8), "slot_status": np.zeros(max(ns, 1), np.uint8)}
    o = PoststateIO()
    o.struct_size = C.sizeof(PoststateIO)
    for k, a in ins.items():
        setattr(o, k, a.ctypes.data if a is not None and a.size else None)
    for k, a in outs.items():
        setattr(o, k, a.ctypes.data)
    root = C.create_string_buffer(bytes(parent_root), 32)
    nxt = None
    if advance is None:
        ctx.check(self._lib.phant_exec_witness_poststate(ctx.handle, self._h, root, C.byref(o)))
    else:
        h = C.c_void_p()
        ctx.check(self._lib.phant_exec_witness_advance(ctx.handle, self._h, root, C.byref(o), int(advance), C.byref(h)))
        nxt = StatelessWitness(h) if h.value else None
    out = {"state_root": outs["state_root"].tobytes(), "storage_roots": outs["storage_roots"][:na],
           "account_status": outs["account_status"][:na], "slot_status": outs["slot_status"][:ns], "n_failed": int(o.n_failed)}
    return out if advance is None else (out, nxt)


def writes_of(info: dict, accounts_after: dict, ctx: Context | None = None) -> dict:
    """The write arrays for a witness from address -> AccountState (the account after the block; every slot of it among the
    witness's keys is written, with zero where its storage does not hold it) or None (deleted); other addresses are kept."""
    from .state import code_hashes
    na, ns = info["n_accounts"], info["n_slots"]
    w = {"account_op": np.zeros(na, np.uint8), "nonces": np.zeros(na, np.uint64), "balances": np.zeros((na, 32), np.uint8),
         "code_hashes": np.zeros((na, 32), np.uint8), "slot_write": np.zeros(ns, np.uint8), "slot_vals": np.zeros((ns, 32), np.uint8)}
    first, slots = info["slot_first"], info["slots"]
    setters = []
    for k, addr in enumerate(bytes(a) for a in info["addresses"]):
        if addr not in accounts_after:
            continue
        a = accounts_after[addr]
        if a is None:
            w["account_op"][k] = L.POST_DELETE
            continue
        w["account_op"][k] = L.POST_SET
        w["nonces"][k] = a.nonce
        w["balances"][k] = np.frombuffer(int(a.balance).to_bytes(32, "big"), np.uint8)
        setters.append((k, a))
        for j in range(int(first[k]), int(first[k + 1])):
            v = int(a.storage.get(int.from_bytes(slots[j].tobytes(), "big"), 0))
            w["slot_write"][j] = 1
            w["slot_vals"][j] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
    if setters:
        h = code_hashes([a.code for _, a in setters], ctx)
        for (k, _), d in zip(setters, h):
            w["code_hashes"][k] = d
    return w


def _poststate(self, ctx: Context | None, parent_root: bytes, accounts_after: dict) -> PostState:
    r = self.poststate_arrays(ctx, parent_root, writes_of(self.info(), accounts_after, ctx))
    return PostState(root=r["state_root"], storage_roots=r["storage_roots"], account_status=r["account_status"],
                     slot_status=r["slot_status"], n_failed=r["n_failed"])


def _advance_arrays(self, ctx: Context | None, parent_root: bytes, writes: dict, keep_old: bool = False):
    """phant_exec_witness_advance, raw: poststate_arrays' dict and the witness of the next block (None when the call failed)."""
    return _poststate_arrays(self, ctx, parent_root, writes, L.ADVANCE_KEEP_OLD if keep_old else 0)


def _advance(self, ctx: Context | None, parent_root: bytes, accounts_after: dict, keep_old: bool = False):
    """-> (PostState, StatelessWitness | None): the post-state of the block and the witness to check the NEXT block with -- the
    same keys and codes over the nodes of the post-state (keep_old: this witness's own nodes behind them, which carries the
    siblings a producer shipped for later removals).  None when a proof failed; the caller closes the witness it gets."""
    r, nxt = self.advance_arrays(ctx, parent_root, writes_of(self.info(), accounts_after, ctx), keep_old)
    return PostState(root=r["state_root"], storage_roots=r["storage_roots"], account_status=r["account_status"],
                     slot_status=r["slot_status"], n_failed=r["n_failed"]), nxt


StatelessWitness.poststate_arrays = _poststate_arrays
StatelessWitness.poststate = _poststate
StatelessWitness.advance_arrays = _advance_arrays
StatelessWitness.advance = _advance


def new_payload_poststate(witness_json: str | bytes, parent_state_root: bytes, accounts_after: dict, header_state_root: bytes,
                          ctx: Context | None = None) -> PostState:
    """The hook behind `runBlock` (src/blockchain/blockchain.zig:83-85): the state root after the block's writes, proven from the
    witness alone, must be the header's.  accounts_after: address -> AccountState, or None for a deleted account.  Raises
    PoststateError when a proof fails, the witness is too thin to re-root, or the root is not header_state_root."""
    w = StatelessWitness.parse_json(witness_json)
    try:
        post = w.poststate(ctx, parent_state_root, accounts_after)
    finally:
        w.close()
    if not post.ok:
        raise PoststateError(f"execution witness: {post.n_failed} keys failed (proofs, or nodes missing for the new root)", post)
    if post.root != bytes(header_state_root):
        raise PoststateError(f"state root after the block is {post.root.hex()}, the header says {bytes(header_state_root).hex()}", post)
    return post


def new_payload_chain(witness_json: str | bytes, parent_state_root: bytes, blocks, ctx: Context | None = None) -> list:
    """k payloads under ONE witness: the document covers the keys of all of `blocks` -- a list of (accounts_after,
    header_state_root), as new_payload_poststate takes them -- and is proven against parent_state_root, the root before the first.
    Every block is checked against the witness the block before it left (StatelessWitness.advance with keep_old, so that siblings
    shipped for a later block's removals stay).  -> the PostState of every block; PoststateError at the first block that fails or
    whose root is not its header's."""
    w = StatelessWitness.parse_json(witness_json)
    out, root = [], bytes(parent_state_root)
    try:
        for n, (accounts_after, header_root) in enumerate(blocks):
            post, nxt = w.advance(ctx, root, accounts_after, keep_old=True)
            w.close()
            w = nxt
            if not post.ok or w is None:
                raise PoststateError(f"block {n}: {post.n_failed} keys failed (proofs, or nodes missing for the new root)", post)
            if post.root != bytes(header_root):
                raise PoststateError(f"block {n}: state root after the block is {post.root.hex()}, the header says {bytes(header_root).hex()}", post)
            out.append(post)
            root = post.root
    finally:
        if w is not None:
            w.close()
    return out
