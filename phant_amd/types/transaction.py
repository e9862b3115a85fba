"""A block's transactions before execution in one call (`block_transactions` <-> phant_block_transactions: the decoded fields of
src/types/transaction.zig:152-273, both hashes, the senders, src/blockchain/blockchain.zig:355-381 `calculateIntrinsicCost` and the
state-free rules of `checkTransaction` / `validateTransaction`), and
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


class BlockTransactions:
    """What phant_block_transactions answers: one numpy array per output of include/phant_gpu.h's phant_txs_out (rows of 32 / 20 / 65
    bytes as (n, width) uint8, big-endian), `first_bad`, and views of the calldata and the access lists inside the blob."""

    def __init__(self, blob, arrays, first_bad):
        self.blob, self.first_bad = blob, first_bad
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
        return [name for k, name in enumerate(FLAG_NAMES) if (int(self.flags[i]) & ERROR_BITS) >> k & 1]


def pack(raw_txs):
    """list of raw transactions -> (blob uint8, offsets uint64 of n + 1)"""
    txs = [bytes(t) for t in raw_txs]
    off = np.zeros(len(txs) + 1, np.uint64)
    if txs:
        off[1:] = np.cumsum([len(t) for t in txs])
    blob = np.frombuffer(b"".join(txs), np.uint8).copy() if off[-1] else np.zeros(1, np.uint8)
    return blob, off


def block_transactions(raw_txs, chain_id, base_fee=None, block_gas_limit=None, recover=True, ctx: Context | None = None) -> BlockTransactions:
    """raw transactions (legacy list, 0x01 || rlp, 0x02 || rlp) -> BlockTransactions.  base_fee (int) None: the two fee rules are
    skipped; block_gas_limit None: GasAboveBlock is not evaluated; recover=False: no secp256k1 launch, no `sender` / `sig_status`."""
    ctx = ctx or default_context()
    blob, off = pack(raw_txs)
    n = len(off) - 1
    flags = (L.TXS_HAVE_GAS_LIMIT if block_gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
    fee = None if base_fee is None else np.frombuffer(int(base_fee).to_bytes(32, "big"), np.uint8).copy()
    arrays = {name: np.zeros((n, k) if k > 1 else n, dtype) for name, dtype, k in L.TX_OUTPUTS if recover or name not in ("sender", "sig_status")}
    arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, blob.ctypes.data, off.ctypes.data, int(off[-1]), int(chain_id),
                       None if fee is None else fee.ctypes.data, int(block_gas_limit or 0))
    out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[arrays[name].ctypes.data if name in arrays else None for name, _, _ in L.TX_OUTPUTS])
    ctx.check(ctx._lib.phant_block_transactions(ctx.handle, C.byref(arg), C.byref(out)))
    return BlockTransactions(blob, arrays, int(out.first_bad))
