"""The block loop of src/blockchain/blockchain.zig for the blocks that need no EVM: `settle` <-> phant_block_settle does what
`applyBody` (:155-205) and `processTransaction` (:262-343) do for transactions that meet no code -- intrinsic gas, the running
gas_available, the exact balance check, the sender's debit, the recipient's and the coinbase's credit, the withdrawals -- for the whole
block in one call, and `run_transfer_block` chains it between the calls around it: raw bytes in, the header's gas_used, receipts root
and state root out, without the host touching an account."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import _lib as L
from .context import Context, default_context


class Settlement:
    """What phant_block_settle answers: one numpy array per output of include/phant_gpu.h's phant_settle_out (rows of 32 bytes as
    (rows, 32) uint8, big-endian) and its scalars."""
    FLAG_NAMES = L.SETTLE_FLAG_NAMES
    ERROR_BITS = L.SETTLE_ERROR_BITS

    def __init__(self, arrays, scalars):
        self.__dict__.update(arrays)
        self.__dict__.update(scalars)
        self.n = len(self.settle_flags)

    @property
    def settled(self) -> bool:
        """every transaction was plain and valid, the coinbase and every withdrawal target were proven, no balance left its range: the
        outputs are what the reference's loop leaves"""
        return self.first_bad == self.n and self.n_not_plain == 0 and self.block_flags == 0 and self.n_wd_unknown == 0 and \
            not self.account_flags.any()

    def errors(self, i):
        """the names of transaction i's failed rules"""
        return [name for k, name in enumerate(self.FLAG_NAMES) if name and (int(self.settle_flags[i]) & self.ERROR_BITS) >> k & 1]

    def not_plain(self, i) -> bool:
        return bool(int(self.settle_flags[i]) & L.SETTLE_NOT_PLAIN)

    @property
    def writes(self) -> dict:
        """the dict StatelessWitness.poststate_arrays takes (no plain transfer writes a slot)"""
        return {"account_op": self.account_op, "nonces": self.nonces_after, "balances": self.balances_after, "code_hashes": self.code_hashes_after,
                "slot_write": None, "slot_vals": None}


class SettleError(RuntimeError):
    def __init__(self, msg: str, settlement: Settlement):
        super().__init__(msg)
        self.settlement = settlement


def settle(bt, against, prestate, witness_info, *, fork, block_gas_limit, base_fee, coinbase, withdrawals=(), ctx: Context | None = None) -> Settlement:
    """bt: `block_transactions(..., fork=)` of the block; against: `against_prestate(bt, prestate, witness_info, fork, probe=...)`, whose
    probes held `coinbase` and every withdrawal's address (their rows are taken from against.probe_row); prestate, witness_info: as
    against_prestate takes them; withdrawals: (20-byte address, amount in gwei) in block order."""
    ctx = ctx or default_context()
    probe_row = {bytes(p): int(r) for p, r in zip(getattr(against, "probe", ()), against.probe_row)}
    wd = [(bytes(a), int(g)) for a, g in withdrawals]
    for address in [bytes(coinbase)] + [a for a, _ in wd]:
        if address not in probe_row:
            raise ValueError("settle: " + address.hex() + " was not among against_prestate's probes")
    n, na, nw = bt.n, int(witness_info["n_accounts"]), len(wd)
    u8 = lambda a, width: np.ascontiguousarray(np.asarray(a, np.uint8).reshape(-1, width))  # noqa: E731
    ins = {"base_fee": np.frombuffer(int(base_fee).to_bytes(32, "big"), np.uint8).copy(), "type": np.ascontiguousarray(bt.type, np.uint8),
           "tx_flags": np.ascontiguousarray(bt.flags, np.uint32), "gas_limit": np.ascontiguousarray(bt.gas_limit, np.uint64),
           "intrinsic_gas": np.ascontiguousarray(bt.intrinsic_gas, np.uint64),
           "floor_gas": np.ascontiguousarray(bt.floor_gas, np.uint64) if hasattr(bt, "floor_gas") else None, "value": u8(bt.value, 32),
           "effective_gas_price": u8(bt.effective_gas_price, 32), "upfront_cost": u8(bt.upfront_cost, 32), "to": u8(bt.to, 20),
           "sender_row": np.ascontiguousarray(against.sender_row, np.uint32), "to_row": np.ascontiguousarray(against.to_row, np.uint32),
           "state_flags": np.ascontiguousarray(against.state_flags, np.uint32), "account_status": np.ascontiguousarray(prestate.account_status, np.uint8),
           "nonces": np.ascontiguousarray(prestate.nonces, np.uint64), "balances": u8(prestate.balances, 32), "code_hashes": u8(prestate.code_hashes, 32),
           "wd_row": np.asarray([probe_row[a] for a, _ in wd], np.uint32), "wd_amount_gwei": np.asarray([g for _, g in wd], np.uint64)}
    if len(ins["account_status"]) < na:
        raise ValueError("the pre-state has fewer rows than the witness has accounts")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    rows = {"n": n, "n_accounts": na, "n_wd": nw}
    arrays = {name: np.zeros((rows[r], k) if k > 1 else rows[r], dtype) for name, dtype, k, r in L.SETTLE_OUTPUTS}
    arg = L.PhantSettleIn(C.sizeof(L.PhantSettleIn), int(fork), n, na, nw, probe_row[bytes(coinbase)], (C.c_uint32 * 2)(0, 0), int(block_gas_limit),
                          *[ptr(ins[name]) for name in L.SETTLE_INPUTS])
    out = L.PhantSettleOut(C.sizeof(L.PhantSettleOut), 0, 0, 0, 0, 0, 0, *[ptr(arrays[name]) for name, _, _, _ in L.SETTLE_OUTPUTS])
    ctx.check(ctx._lib.phant_block_settle(ctx.handle, C.byref(arg), C.byref(out)))
    return Settlement(arrays, {k: int(getattr(out, k)) for k in ("first_bad", "n_not_plain", "first_not_plain", "block_flags", "n_wd_unknown", "gas_used")})


@dataclass
class TransferBlock:
    gas_used: int
    receipts_root: bytes
    state_root: bytes
    settlement: Settlement


def run_transfer_block(raw_txs, withdrawals, header_fields, witness, parent_state_root, chain_id, fork, ctx: Context | None = None) -> TransferBlock:
    """A stateless block of plain transfers and its withdrawals from raw bytes to what its header must say:
    block_transactions -> against_prestate -> settle -> block_receipts (status 1, the cumulative gas, no logs) -> poststate.
    header_fields: {"coinbase": 20 bytes, "base_fee": int, "gas_limit": int}; witness: the block's StatelessWitness, which must prove
    every sender, recipient, the coinbase and every withdrawal's address (an address the state lacks: proven absent) -- and, for an
    account the block empties (EIP-161 deletes it), the siblings a removal needs: `build_witness(..., may_remove=[that address])`.
    Raises SettleError when the block is not settled (a row needs the EVM, a rule failed, an address is not proven) and
    stateless.PoststateError when the witness is too thin for the new root.  The caller compares the result with the header."""
    from .stateless import PostState, PoststateError
    from .types import transaction as TX
    from .types.receipt import Receipt, block_receipts
    ctx = ctx or default_context()
    coinbase, base_fee, gas_limit = bytes(header_fields["coinbase"]), int(header_fields["base_fee"]), int(header_fields["gas_limit"])
    wd = [(bytes(a), int(g)) for a, g in withdrawals]
    bt = TX.block_transactions(raw_txs, chain_id, base_fee=base_fee, block_gas_limit=gas_limit, ctx=ctx, fork=fork)
    info = witness.info()
    pre = SimpleNamespace(**witness.prestate_arrays(ctx, parent_state_root))
    against = TX.against_prestate(bt, pre, info, fork, probe=[coinbase] + [a for a, _ in wd], ctx=ctx)
    s = settle(bt, against, pre, info, fork=fork, block_gas_limit=gas_limit, base_fee=base_fee, coinbase=coinbase, withdrawals=wd, ctx=ctx)
    if not s.settled:
        raise SettleError(f"the block is not settled: first_bad {s.first_bad} of {s.n}, {s.n_not_plain} rows need the EVM, block_flags {s.block_flags}, "
                          f"{s.n_wd_unknown} withdrawals unknown, {int(np.count_nonzero(s.account_flags))} balances out of range", s)
    receipts = block_receipts([Receipt(True, int(s.cumulative_gas_used[i]), [], int(bt.type[i])) for i in range(s.n)], ctx=ctx)
    r = witness.poststate_arrays(ctx, parent_state_root, s.writes)
    if r["n_failed"]:
        raise PoststateError(f"execution witness: {r['n_failed']} keys failed (proofs, or nodes missing for the new root)",
                             PostState(r["state_root"], r["storage_roots"], r["account_status"], r["slot_status"], r["n_failed"]))
    return TransferBlock(s.gas_used, receipts.receipts_root, r["state_root"], s)
