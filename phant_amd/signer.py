"""src/signer/signer.zig:40-79 `get_sender` for a block's transactions: the secp256k1 public-key recovery
(src/crypto/ecdsa.zig:19-21) and address = keccak256(pubkey[1..])[12..] (:77-78), one lane per signature in one launch
(`recover`), from raw transactions in one call (`senders`), or only the hashing for keys recovered elsewhere
(`addresses_from_pubkeys`)."""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .context import Context, default_context, _np_ptr

STATUS_NAMES = ("OK", "BAD_RANGE", "HIGH_S", "BAD_RECID", "NOT_ON_CURVE", "INFINITY", "BAD_TX", "BAD_V")


def addresses_from_pubkeys(pubkeys, ctx: Context | None = None) -> np.ndarray:
    """(n, 64) uint8 public keys, or (n, 65) with the 0x04 tag in front -> (n, 20) uint8 addresses."""
    ctx = ctx or default_context()
    pk = np.ascontiguousarray(pubkeys, np.uint8)
    if pk.ndim != 2 or pk.shape[1] not in (64, 65):
        raise ValueError("public keys are 64 bytes (or 65 with the 0x04 tag)")
    n, stride = pk.shape
    out = np.zeros((n, 20), np.uint8)
    if n:
        base = pk.reshape(-1)[stride - 64:]  # skips the tag of the first key; the stride skips the others
        ctx.check(ctx._lib.phant_sender_addresses(ctx.handle, _np_ptr(base), stride, n, _np_ptr(out)))
    return out


def _rows(a, width, what):
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: (n, {width}) uint8 expected")
    return a


def recover(hashes, r, s, recid, low_s: bool = False, want: str = "addresses", ctx: Context | None = None):
    """phant_ecrecover_batch.  hashes, r, s: (n, 32) uint8, big-endian; recid: (n,) uint8.  low_s: PHANT_RECOVER_LOW_S.
    want = "addresses" -> (addresses (n, 20), status (n,)); "pubkeys" -> (pubkeys (n, 64), status); "both" -> (pubkeys,
    addresses, status); "status" -> status.  A failed item's outputs are zero; status values: _lib.SIG_*."""
    if want not in ("addresses", "pubkeys", "both", "status"):
        raise ValueError("want: addresses, pubkeys, both or status")
    ctx = ctx or default_context()
    h, r, s = _rows(hashes, 32, "hashes"), _rows(r, 32, "r"), _rows(s, 32, "s")
    ids = np.ascontiguousarray(recid, np.uint8).reshape(-1)
    n = h.shape[0]
    if not (r.shape[0] == s.shape[0] == ids.shape[0] == n):
        raise ValueError("hashes, r, s and recid differ in length")
    pk = np.zeros((n, 64), np.uint8) if want in ("pubkeys", "both") else None
    ad = np.zeros((n, 20), np.uint8) if want in ("addresses", "both") else None
    st = np.zeros(n, np.uint8)
    p = lambda a: None if a is None else _np_ptr(a)  # noqa: E731
    ctx.check(ctx._lib.phant_ecrecover_batch(ctx.handle, p(h), p(r), p(s), p(ids), n, L.RECOVER_LOW_S if low_s else 0, p(pk), p(ad),
                                             p(st)))
    return {"addresses": (ad, st), "pubkeys": (pk, st), "both": (pk, ad, st), "status": st}[want]


def senders(raw_txs, chain_id: int, ctx: Context | None = None):
    """phant_tx_senders: raw transactions (legacy list, 0x01 || rlp, 0x02 || rlp) -> (addresses (n, 20), status (n,)).
    Legacy v = 27 / 28 is hashed with the pre-EIP-155 preimage, 35 + 2 chain_id + {0, 1} with the EIP-155 one (what was
    signed; signer.zig:87 differs for 27 / 28, see include/phant_gpu.h)."""
    ctx = ctx or default_context()
    txs = [bytes(t) for t in raw_txs]
    n = len(txs)
    off = np.zeros(n + 1, np.uint64)
    if n:
        off[1:] = np.cumsum([len(t) for t in txs])
    blob = np.frombuffer(b"".join(txs) or b"\x00", np.uint8)
    ad, st = np.zeros((n, 20), np.uint8), np.zeros(n, np.uint8)
    ctx.check(ctx._lib.phant_tx_senders(ctx.handle, _np_ptr(blob), _np_ptr(off), n, int(chain_id), _np_ptr(ad), _np_ptr(st)))
    return ad, st


SECP_OPS = {"fe_mul": 0, "fe_sqr": 1, "fe_inv": 2, "fe_sqrt": 3, "sc_mul": 4, "sc_inv": 5, "pt_double": 6, "pt_add": 7,
            "pt_add_affine": 8}


def secp_op(op: str, a, b=None, ctx: Context | None = None) -> np.ndarray:
    """phant_diag_secp_op (include/phant_gpu_diag.h): one arithmetic primitive per lane; rows as the header lays them out."""
    ctx = ctx or default_context()
    code = SECP_OPS[op]
    width, out_width = (65, 65) if code >= 6 else (32, 33 if code == 3 else 32)
    a = _rows(a, width, "a")
    b = None if b is None else _rows(b, width, "b")
    out = np.zeros((a.shape[0], out_width), np.uint8)
    ctx.check(ctx._lib.phant_diag_secp_op(ctx.handle, code, _np_ptr(a), None if b is None else _np_ptr(b), a.shape[0], _np_ptr(out)))
    return out
