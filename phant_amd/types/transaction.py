"""A block's transactions before execution in one call (`block_transactions` <-> phant_block_transactions: the decoded fields of
src/types/transaction.zig:152-273, both hashes, the senders, src/blockchain/blockchain.zig:355-381 `calculateIntrinsicCost` and the
state-free rules of `checkTransaction` / `validateTransaction`), the same rows against the pre-state (`against_prestate`), the access
lists decoded and joined with the witness's tables (`access_lists` <-> phant_block_access_lists, blockchain.zig:284-295), and
transaction hashes of a whole block in one launch <-> src/types/transaction.zig:79-85 `Tx.hash`
(:183-187 legacy = keccak256(rlp(tx)); :223-228 / :256-261 typed = keccak256(type || rlp(tx))): in every case
the Keccak-256 of the transaction's EIP-2718 encoding, the bytes a block body carries."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib as L
from ..context import Context, default_context
from ..crypto import hasher


def hashes(encoded_txs, ctx: Context | None = None) -> np.ndarray:
    """list of encoded transactions -> (n, 32) uint8."""
    txs = [bytes(t) for t in encoded_txs]
    if any(len(t) == 0 for t in txs):
        raise ValueError("EncodedTxCannotBeEmpty")  # transaction.zig:31-33
    off = np.zeros(len(txs) + 1, np.uint64)
    if txs:
        off[1:] = np.cumsum([len(t) for t in txs])
    blob = np.frombuffer(b"".join(txs), np.uint8).copy() if txs else np.zeros(1, np.uint8)
    return hasher.keccak256_batch(blob, off, ctx=ctx)


FLAG_NAMES = L.TX_FLAG_NAMES
ERROR_BITS = L.TX_ERROR_BITS
FLAG_NAMES_EX = L.TX_FLAG_NAMES_EX
ERROR_BITS_EX = L.TX_ERROR_BITS_EX
FORK_LONDON, FORK_CANCUN, FORK_PRAGUE = L.TXS_FORK_LONDON, L.TXS_FORK_CANCUN, L.TXS_FORK_PRAGUE
GAS_PER_BLOB = 131072
_BLOB_FEE_UPDATE_FRACTION = {FORK_CANCUN: 3338477, FORK_PRAGUE: 5007716}


def blob_base_fee(excess_blob_gas, fork=FORK_PRAGUE) -> int:
    """EIP-4844's fake_exponential(1, excess_blob_gas, BLOB_BASE_FEE_UPDATE_FRACTION) with the fork's fraction (EIP-7691 raised it for
    Prague): what `block_transactions(..., blob_base_fee=)` takes.  Computed on the host: one number a block."""
    denominator = _BLOB_FEE_UPDATE_FRACTION[fork]
    i, output, accum = 1, 0, denominator  # factor = 1
    while accum > 0:
        output += accum
        accum = accum * int(excess_blob_gas) // (denominator * i)
        i += 1
    return output // denominator


class BlockTransactions:
    """What phant_block_transactions answers: one numpy array per output of include/phant_gpu.h's phant_txs_out (rows of 32 / 20 / 65
    bytes as (n, width) uint8, big-endian), `first_bad`, and views of the calldata and the access lists inside the blob."""

    def __init__(self, blob, arrays, first_bad, fork=None, n_auth=0, blob_gas_used=0):
        self.blob, self.first_bad, self.fork, self.n_auth, self.blob_gas_used = blob, first_bad, fork, n_auth, blob_gas_used
        self.__dict__.update(arrays)
        self.n = len(self.flags)

    def data(self, i) -> np.ndarray:
        """transaction i's calldata: a view into the blob"""
        return self.blob[int(self.data_off[i]):int(self.data_off[i]) + int(self.data_len[i])]

    def access_list(self, i) -> np.ndarray:
        """the payload of transaction i's access list (RLP: [[address, [key, ...]], ...] without the outer header): a view"""
        return self.blob[int(self.al_off[i]):int(self.al_off[i]) + int(self.al_len[i])]

    def errors(self, i):
        """the names of transaction i's failed rules, the one the reference returns first in front"""
        names = FLAG_NAMES if self.fork is None else FLAG_NAMES_EX
        return [name for k, name in enumerate(names) if (int(self.flags[i]) & L.tx_error_bits(self.fork)) >> k & 1]

    def versioned_hashes(self, i) -> np.ndarray:
        """transaction i's blob versioned hashes, (blobs, 32): a view into the blob (calls with a fork)"""
        at, k = int(self.blob_off[i]), int(self.blobs[i])
        return self.blob[at:at + 33 * k].reshape(k, 33)[:, 1:]

    def authorizations(self, i) -> dict:
        """the rows of transaction i's authorization tuples: {output of phant_txs_ex_out: its slice} (calls with a fork)"""
        rows = slice(int(self.auth_first[i]), int(self.auth_first[i + 1]))
        return {name: getattr(self, name)[rows] for name, _, _ in L.TX_AUTH_OUTPUTS if hasattr(self, name)}


def pack(raw_txs):
    """list of raw transactions -> (blob uint8, offsets uint64 of n + 1)"""
    txs = [bytes(t) for t in raw_txs]
    off = np.zeros(len(txs) + 1, np.uint64)
    if txs:
        off[1:] = np.cumsum([len(t) for t in txs])
    blob = np.frombuffer(b"".join(txs), np.uint8).copy() if off[-1] else np.zeros(1, np.uint8)
    return blob, off


def block_transactions(raw_txs, chain_id, base_fee=None, block_gas_limit=None, recover=True, ctx: Context | None = None, fork=None,
                       blob_base_fee=None) -> BlockTransactions:
    """raw transactions (legacy list, 0x01 || rlp, 0x02 || rlp) -> BlockTransactions.  base_fee (int) None: the two fee rules are
    skipped; block_gas_limit None: GasAboveBlock is not evaluated; recover=False: no secp256k1 launch, no `sender` / `sig_status`.
    fork None: phant_block_transactions.  FORK_LONDON / FORK_CANCUN (+ 0x03 || rlp) / FORK_PRAGUE (+ 0x04 || rlp, the EIP-7623 floor):
    phant_block_transactions_ex, whose result also has the arrays of phant_txs_ex_out (one row per authorization tuple of the whole
    call for the auth_* ones; without `authority` / `auth_status` when recover=False), `n_auth` and `blob_gas_used`; blob_base_fee
    (int, `blob_base_fee()` of the parent's excess blob gas) None: BlobFeeBelowBase is not evaluated."""
    ctx = ctx or default_context()
    blob, off = pack(raw_txs)
    n = len(off) - 1
    flags = (L.TXS_HAVE_GAS_LIMIT if block_gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
    fee = None if base_fee is None else np.frombuffer(int(base_fee).to_bytes(32, "big"), np.uint8).copy()
    arrays = {name: np.zeros((n, k) if k > 1 else n, dtype) for name, dtype, k in L.TX_OUTPUTS if recover or name not in ("sender", "sig_status")}
    arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, blob.ctypes.data, off.ctypes.data, int(off[-1]), int(chain_id),
                       None if fee is None else fee.ctypes.data, int(block_gas_limit or 0))
    out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[arrays[name].ctypes.data if name in arrays else None for name, _, _ in L.TX_OUTPUTS])
    if fork is None:
        ctx.check(ctx._lib.phant_block_transactions(ctx.handle, C.byref(arg), C.byref(out)))
        return BlockTransactions(blob, arrays, int(out.first_bad))
    # a tuple takes at least 27 bytes: the rows that the transactions beginning with 0x04 can need
    cap = sum(int(off[i + 1] - off[i]) for i in range(n) if off[i + 1] > off[i] and blob[int(off[i])] == 4) // 27 if fork >= FORK_PRAGUE else 0
    for name, dtype, k in L.TX_EX_OUTPUTS:
        arrays[name] = np.zeros((n, k) if k > 1 else n + (name == "auth_first"), dtype)
    auth = {name: np.zeros((cap, k) if k > 1 else cap, dtype) for name, dtype, k in L.TX_AUTH_OUTPUTS if recover or name not in ("authority", "auth_status")}
    blob_fee = None if blob_base_fee is None else np.frombuffer(int(blob_base_fee).to_bytes(32, "big"), np.uint8).copy()
    xarg = L.PhantTxsExIn(C.sizeof(L.PhantTxsExIn), int(fork), arg, None if blob_fee is None else blob_fee.ctypes.data, cap, 0)
    xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0, 0, out, *[arrays[name].ctypes.data for name, _, _ in L.TX_EX_OUTPUTS],
                           *[auth[name].ctypes.data if name in auth and cap else None for name, _, _ in L.TX_AUTH_OUTPUTS])
    ctx.check(ctx._lib.phant_block_transactions_ex(ctx.handle, C.byref(xarg), C.byref(xout)))
    arrays.update({name: a[:int(xout.n_auth)] for name, a in auth.items()})
    return BlockTransactions(blob, arrays, int(xout.base.first_bad), int(fork), int(xout.n_auth), int(xout.blob_gas_used))


class TransactionsAgainstPrestate:
    """What phant_block_txs_prestate answers: one numpy array per output of include/phant_gpu.h's phant_txstate_out (spent_before as
    (n, 32) uint8, big-endian), `first_bad` and `n_undetermined`."""
    FLAG_NAMES = L.TXST_FLAG_NAMES
    ERROR_BITS = L.TXST_ERROR_BITS

    def __init__(self, arrays, first_bad, n_undetermined):
        self.first_bad, self.n_undetermined = first_bad, n_undetermined
        self.__dict__.update(arrays)
        self.n = len(self.state_flags)

    def errors(self, i):
        """the names of transaction i's failed rules"""
        return [name for k, name in enumerate(self.FLAG_NAMES) if name and (int(self.state_flags[i]) & self.ERROR_BITS) >> k & 1]

    def undetermined(self, i) -> bool:
        return bool(int(self.state_flags[i]) & L.TXST_UNDETERMINED)


def against_prestate(bt: BlockTransactions, prestate, witness_info, fork, probe=(), ctx: Context | None = None) -> TransactionsAgainstPrestate:
    """A block's transactions against the pre-state its witness proves <-> phant_block_txs_prestate: which witness row every sender,
    recipient, authority and probe is, the nonce every transaction must carry, EIP-3607, and what a sender can have spent before each of
    its transactions (blockchain.zig:270-276, for the whole block before any transaction runs).  bt: `block_transactions` of the block
    (with its senders); prestate, witness_info: `StatelessWitness.prestate()` and `.info()` of phant_amd/stateless.py (anything with
    their arrays will do); fork: FORK_*; probe: further 20-byte addresses to locate."""
    ctx = ctx or default_context()
    if not hasattr(bt, "sender"):
        raise ValueError("against_prestate needs the senders: block_transactions(..., recover=True)")
    u8 = lambda a, width: np.ascontiguousarray(np.asarray(a, np.uint8).reshape(-1, width))  # noqa: E731
    n, na, nc = bt.n, int(witness_info["n_accounts"]), int(witness_info["n_codes"])
    has_auth = hasattr(bt, "authority") and hasattr(bt, "auth_first")
    n_auth = len(bt.auth_status) if has_auth else 0
    probes = u8(np.frombuffer(b"".join(bytes(p) for p in probe), np.uint8), 20)
    ins = {"sender": u8(bt.sender, 20), "sig_status": np.ascontiguousarray(bt.sig_status, np.uint8), "tx_flags": np.ascontiguousarray(bt.flags, np.uint32),
           "nonce": np.ascontiguousarray(bt.nonce, np.uint64), "upfront_cost": u8(bt.upfront_cost, 32), "to": u8(bt.to, 20),
           "auth_first": np.ascontiguousarray(bt.auth_first, np.uint32) if has_auth else None,
           "authority": u8(bt.authority, 20) if has_auth else None, "auth_status": np.ascontiguousarray(bt.auth_status, np.uint8) if has_auth else None,
           "addresses": u8(witness_info["addresses"], 20), "account_status": np.ascontiguousarray(prestate.account_status, np.uint8),
           "nonces": np.ascontiguousarray(prestate.nonces, np.uint64), "balances": u8(prestate.balances, 32), "code_hashes": u8(prestate.code_hashes, 32),
           "code_index": np.ascontiguousarray(prestate.code_index, np.uint32), "code_off": np.ascontiguousarray(witness_info["code_off"], np.uint64),
           "codes": np.ascontiguousarray(witness_info["codes"], np.uint8)}
    if len(ins["account_status"]) < na or len(ins["addresses"]) < na:
        raise ValueError("the pre-state has fewer rows than the witness has accounts")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    rows = {"n": n, "n_accounts": na, "n_probe": len(probes)}
    arrays = {name: np.zeros((rows[r], k) if k > 1 else rows[r], dtype) for name, dtype, k, r in L.TXSTATE_OUTPUTS}
    arg = L.PhantTxstateIn(C.sizeof(L.PhantTxstateIn), int(fork), n, n_auth, na, nc, len(probes), 0, *[ptr(ins[name]) for name in L.TXSTATE_INPUTS],
                           int(witness_info["code_bytes"]), ptr(probes))
    if has_auth:
        arg.auth_first = ins["auth_first"].ctypes.data
    out = L.PhantTxstateOut(C.sizeof(L.PhantTxstateOut), 0, 0, 0, *[ptr(arrays[name]) for name, _, _, _ in L.TXSTATE_OUTPUTS])
    ctx.check(ctx._lib.phant_block_txs_prestate(ctx.handle, C.byref(arg), C.byref(out)))
    r = TransactionsAgainstPrestate(arrays, int(out.first_bad), int(out.n_undetermined))
    r.probe = [bytes(p) for p in probe]  # (probe_row's addresses, for the calls that take rows: blockchain.settle)
    return r


class AccessLists:
    """What phant_block_access_lists answers: one numpy array per output of include/phant_gpu.h's phant_access_out (address as
    (n_tuples, 20), key as (n_keys, 32) uint8), the five totals, and `lists`: per transaction the list of (address, [keys]) as bytes."""
    MALFORMED, DUPLICATES, ROW_NONE = L.AL_MALFORMED, L.AL_DUPLICATES, L.ROW_NONE

    def __init__(self, arrays, n_missing_accounts, n_missing_slots, first_malformed):
        self.n_missing_accounts, self.n_missing_slots, self.first_malformed = n_missing_accounts, n_missing_slots, first_malformed
        self.__dict__.update(arrays)
        self.n, self.n_tuples, self.n_keys = len(self.al_flags), len(self.account_row), len(self.slot_row)

    def entries(self, i):
        """transaction i's access list: [(address, [key, ...]), ...]"""
        return [(self.address[e].tobytes(), [self.key[k].tobytes() for k in range(int(self.key_first[e]), int(self.key_first[e + 1]))])
                for e in range(int(self.tuple_first[i]), int(self.tuple_first[i + 1]))]

    @property
    def lists(self):
        return [self.entries(i) for i in range(self.n)]

    def malformed(self, i) -> bool:
        return bool(int(self.al_flags[i]) & L.AL_MALFORMED)


def access_lists(bt, prestate=None, ctx: Context | None = None) -> AccessLists:
    """A block's access lists decoded and joined with the pre-state tables <-> phant_block_access_lists: every [address, [keys]] entry,
    which witness row every address and every (address, key) pair is, the first occurrences (the warm sets blockchain.zig:284-295
    builds) and what the witness lacks.  bt: `block_transactions` of the block, or anything with its `blob`, `al_off` and `al_len`
    (a dict will do); prestate: `StatelessWitness.info()` of phant_amd/stateless.py (anything with n_accounts, addresses, slot_first,
    n_slots and slots), None: nothing is joined and every row is ROW_NONE."""
    ctx = ctx or default_context()
    get = (lambda k: bt[k]) if isinstance(bt, dict) else (lambda k: getattr(bt, k))  # noqa: E731
    blob = np.ascontiguousarray(get("blob"), np.uint8).reshape(-1)
    al_off, al_len = np.ascontiguousarray(get("al_off"), np.uint64), np.ascontiguousarray(get("al_len"), np.uint32)
    n = len(al_len)
    if len(al_off) != n:
        raise ValueError("al_off and al_len differ in length")
    na = int(prestate["n_accounts"]) if prestate is not None else 0
    ns = int(prestate["n_slots"]) if na else 0
    addresses = np.ascontiguousarray(np.asarray(prestate["addresses"], np.uint8).reshape(-1, 20)) if na else None
    slot_first = np.ascontiguousarray(prestate["slot_first"], np.uint32) if na else None
    slots = np.ascontiguousarray(np.asarray(prestate["slots"], np.uint8).reshape(-1, 32)) if ns else None
    if na and (len(addresses) < na or len(slot_first) < na + 1 or (ns and len(slots) < ns)):
        raise ValueError("the pre-state tables are shorter than their counts")
    total = int(al_len.sum(dtype=np.uint64))
    rows = {"n": n, "n_tuples": total // 23, "n_keys": total // 33}  # no span has more tuples or keys than its bytes allow
    arrays = {name: np.zeros((rows[r] + extra, k) if k > 1 else rows[r] + extra, dtype) for name, dtype, k, r, extra in L.ACCESS_OUTPUTS}
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    arg = L.PhantAccessIn(C.sizeof(L.PhantAccessIn), n, na, ns, ptr(blob), blob.size, ptr(al_off), ptr(al_len), ptr(addresses), ptr(slot_first), ptr(slots))
    out = L.PhantAccessOut(C.sizeof(L.PhantAccessOut), 0, 0, 0, 0, 0, rows["n_tuples"], rows["n_keys"],
                           *[arrays[name].ctypes.data for name, _, _, _, _ in L.ACCESS_OUTPUTS])
    ctx.check(ctx._lib.phant_block_access_lists(ctx.handle, C.byref(arg), C.byref(out)))
    got = {"n": n, "n_tuples": int(out.n_tuples), "n_keys": int(out.n_keys)}
    arrays = {name: arrays[name][:got[r] + extra] for name, _, _, r, extra in L.ACCESS_OUTPUTS}
    return AccessLists(arrays, int(out.n_missing_accounts), int(out.n_missing_slots), int(out.first_malformed))
