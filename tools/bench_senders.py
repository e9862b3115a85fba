#!/usr/bin/env python3
"""Sender recovery on a block's worth of signatures: one JSON line.

For n = 100, 1 000, 10 000, 100 000 reference-signed signatures (tests/secp_ref.py; random keys and nonces built as sums of two
random sets, so that the reference knows every public key after one point addition), medians over --reps calls:
  ecrecover_device_ms     phant_timing's device region of phant_ecrecover_batch_dev (addresses and status out)
  addresses_device_ms     phant_sender_addresses_dev on the same n public keys (the hashing that existed before)
  sigs_per_s              n / ecrecover_device_ms
  tx_senders_wall_ms      host-form wall time of phant_tx_senders on --txs (10 000) reference-signed EIP-1559 transactions
  cpu_one_core_us_per_sig the same recoveries on one core through the system's libcrypto (curve secp256k1), or
                          "no CPU baseline on this host" -- never a figure from the Python reference
Every output is compared with the reference before anything is timed.
Needs a GPU.  python tools/bench_senders.py [--sizes 100,1000,10000,100000] [--txs 10000] [--reps 20] [--warmup 3]
"""
import argparse
import ctypes as C
import ctypes.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def signers(S, rng, n):
    """n (d, public key, k, R): keys and nonces a_u + b_v of two random sets of ceil(sqrt(n))"""
    w = int(np.ceil(np.sqrt(n)))
    rnd = lambda: [int.from_bytes(rng.bytes(32), "big") % (S.N - 1) + 1 for _ in range(w)]  # noqa: E731
    a, b, c, e = rnd(), rnd(), rnd(), rnd()
    Ap, Bp, Cp, Ep = ([S.mul(v, S.G) for v in vs] for vs in (a, b, c, e))
    out = []
    for i in range(n):
        u, v = divmod(i, w)
        out.append(((a[u] + b[v]) % S.N, S.add(Ap[u], Bp[v]), (c[v] + e[u]) % S.N, S.add(Cp[v], Ep[u])))
    return out


def sign_with(S, signer, z):
    d, _, k, R = signer
    r = R[0] % S.N
    s = pow(k, -1, S.N) * (z + r * d) % S.N
    recid = (R[1] & 1) | (2 if R[0] >= S.N else 0)
    if s > S.N // 2:
        s, recid = S.N - s, recid ^ 1
    return r, s, recid


def cpu_baseline(S, tuples, keys):
    """us per recovery on one core through libcrypto, or None.  The steps of SEC 1 section 4.1.6 with OpenSSL's EC_POINT calls."""
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = C.CDLL(name)
        vp = C.c_void_p
        for f, res, args in (("EC_GROUP_new_by_curve_name", vp, [C.c_int]), ("OBJ_txt2nid", C.c_int, [C.c_char_p]), ("BN_CTX_new", vp, []),
                             ("BN_bin2bn", vp, [C.c_char_p, C.c_int, vp]), ("BN_new", vp, []), ("EC_POINT_new", vp, [vp]),
                             ("EC_POINT_set_compressed_coordinates", C.c_int, [vp, vp, vp, C.c_int, vp]),
                             ("BN_mod_inverse", vp, [vp, vp, vp, vp]), ("BN_mod_mul", C.c_int, [vp, vp, vp, vp, vp]),
                             ("BN_mod_sub", C.c_int, [vp, vp, vp, vp, vp]), ("EC_POINT_mul", C.c_int, [vp, vp, vp, vp, vp, vp]),
                             ("EC_POINT_point2oct", C.c_size_t, [vp, vp, C.c_int, C.c_char_p, C.c_size_t, vp]),
                             ("BN_free", None, [vp]), ("EC_POINT_free", None, [vp]), ("EC_GROUP_get0_order", vp, [vp])):
            fn = getattr(lib, f)
            fn.restype, fn.argtypes = res, args
        grp = lib.EC_GROUP_new_by_curve_name(lib.OBJ_txt2nid(b"secp256k1"))
        if not grp:
            return None
    except (OSError, AttributeError):
        return None
    bctx, order = lib.BN_CTX_new(), lib.EC_GROUP_get0_order(grp)
    zero = lib.BN_bin2bn(b"\x00", 1, None)
    ins = [(z.to_bytes(32, "big"), r.to_bytes(32, "big"), s.to_bytes(32, "big"), recid) for z, r, s, recid in tuples]
    buf = C.create_string_buffer(65)
    R, Q, ri, u1, u2 = lib.EC_POINT_new(grp), lib.EC_POINT_new(grp), lib.BN_new(), lib.BN_new(), lib.BN_new()
    t0 = time.perf_counter()
    for (zb, rb, sb, recid), key in zip(ins, keys):
        z, r, s = lib.BN_bin2bn(zb, 32, None), lib.BN_bin2bn(rb, 32, None), lib.BN_bin2bn(sb, 32, None)
        assert recid < 2 and lib.EC_POINT_set_compressed_coordinates(grp, R, r, recid & 1, bctx) == 1
        lib.BN_mod_inverse(ri, r, order, bctx)
        lib.BN_mod_mul(u1, z, ri, order, bctx)
        lib.BN_mod_sub(u1, zero, u1, order, bctx)
        lib.BN_mod_mul(u2, s, ri, order, bctx)
        assert lib.EC_POINT_mul(grp, Q, u1, R, u2, bctx) == 1
        assert lib.EC_POINT_point2oct(grp, Q, 4, buf, 65, bctx) == 65 and buf.raw[1:] == key  # (4: uncompressed)
        for x in (z, r, s):
            lib.BN_free(x)
    return (time.perf_counter() - t0) * 1e6 / len(ins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,10000,100000")
    ap.add_argument("--txs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import signer
    from phant_amd.context import default_context
    from tests import secp_ref as S

    O.build()
    rng = np.random.default_rng(2026)
    nmax = max(sizes + [args.txs])
    who = signers(S, rng, nmax)
    zs = [int.from_bytes(rng.bytes(32), "big") for _ in range(nmax)]
    tuples = [(z,) + sign_with(S, w, z) for w, z in zip(who, zs)]
    keys = [S.pubkey_bytes(w[1]) for w in who]
    key_blob = np.frombuffer(b"".join(keys), np.uint8)
    addrs = np.ascontiguousarray(O.keccak256_batch(key_blob, np.arange(nmax + 1, dtype=np.uint64) * 64)[:, 12:])
    for i in range(0, nmax, max(1, nmax // 16)):  # the construction against the reference's own recovery
        assert S.recover(*tuples[i], S.LOW_S) == (S.OK, who[i][1])
    rows = lambda k: np.frombuffer(b"".join(t[k].to_bytes(32, "big") for t in tuples), np.uint8).reshape(-1, 32)  # noqa: E731
    H, R_, S_, ids = rows(0), rows(1), rows(2), np.array([t[3] for t in tuples], np.uint8)
    ctx = default_context()
    pk, ad, st = signer.recover(H, R_, S_, ids, low_s=True, want="both", ctx=ctx)
    assert not st.any() and np.array_equal(pk.reshape(-1), key_blob) and np.array_equal(ad, addrs), "outputs differ from the reference"

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_h, d_r, d_s, d_id, d_pk = dev(H), dev(R_), dev(S_), dev(ids), dev(key_blob)
    d_ad = torch.zeros(nmax * 20, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(nmax, dtype=torch.uint8, device="cuda")

    def timed(fn):
        ctx.check(ctx._lib.phant_timing(ctx.handle, 1))
        ms = []
        try:
            for i in range(args.warmup + args.reps):
                fn()
                if i >= args.warmup:
                    ms.append(ctx.last_kernel_ms())
        finally:
            ctx.check(ctx._lib.phant_timing(ctx.handle, 0))
        return float(np.median(ms))

    out = {"tool": "bench_senders", "reps": args.reps, "sizes": {}}
    for n in sizes:
        rec = timed(lambda: ctx.check(ctx._lib.phant_ecrecover_batch_dev(ctx.handle, d_h.data_ptr(), d_r.data_ptr(), d_s.data_ptr(),
                                                                         d_id.data_ptr(), n, 1, None, d_ad.data_ptr(), d_st.data_ptr())))
        ctx.sync()
        assert np.array_equal(d_ad.cpu().numpy()[:n * 20].reshape(-1, 20), addrs[:n]) and not d_st.cpu().numpy()[:n].any()
        had = timed(lambda: ctx.check(ctx._lib.phant_sender_addresses_dev(ctx.handle, d_pk.data_ptr(), 64, n, d_ad.data_ptr())))
        out["sizes"][str(n)] = {"ecrecover_device_ms": round(rec, 4), "addresses_device_ms": round(had, 4),
                                "sigs_per_s": round(n / (rec * 1e-3))}

    # transactions: EIP-1559 transfers signed by the same signers
    txs = []
    for i in range(args.txs):
        fields = [S.rlp_int(1), S.rlp_int(i), S.rlp_int(2), S.rlp_int(10**9), S.rlp_int(21000), S.rlp_bytes(rng.bytes(20)),
                  S.rlp_int(10**15 + i), S.rlp_bytes(b""), S.rlp_list([])]
        z = int.from_bytes(O.keccak256(b"\x02" + S.rlp_list(fields)), "big")
        r, s, recid = sign_with(S, who[i], z)
        txs.append(b"\x02" + S.rlp_list(fields + [S.rlp_int(recid), S.rlp_int(r), S.rlp_int(s)]))
    for i in range(0, args.txs, max(1, args.txs // 8)):
        assert S.tx_sender(O, txs[i], 1) == (S.OK, bytes(addrs[i]))
    got, st = signer.senders(txs, 1, ctx=ctx)
    assert not st.any() and np.array_equal(got, addrs[:args.txs]), "tx senders differ from the reference"
    blob = np.frombuffer(b"".join(txs), np.uint8)
    off = np.zeros(args.txs + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in txs])
    o_ad, o_st = np.zeros((args.txs, 20), np.uint8), np.zeros(args.txs, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    wall = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        ctx.check(ctx._lib.phant_tx_senders(ctx.handle, p(blob), p(off), args.txs, 1, p(o_ad), p(o_st)))
        wall.append((time.perf_counter() - t0) * 1e3)
    out["txs"] = args.txs
    out["tx_senders_wall_ms"] = round(float(np.median(wall[args.warmup:])), 3)

    m = min(2000, nmax)
    cpu = cpu_baseline(S, tuples[:m], keys[:m])
    out["cpu_one_core_us_per_sig"] = round(cpu, 2) if cpu is not None else "no CPU baseline on this host"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
