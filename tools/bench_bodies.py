#!/usr/bin/env python3
"""Chain segments of block bodies (phant_block_bodies) beside the per-block path: one JSON line a segment.

A segment is --blocks blocks of --per-block transactions in tools/bench_transactions.py's mix (london, or prague with its blob and
set-code share) and 16 withdrawals a block.  The reference signs --unique blocks' worth of transactions (signing is the slow part
of building the input) and the segment repeats them block after block: a lane's work does not depend on what its neighbours hold.
Every output of the segment call is compared with tests/bodies_ref.py before anything is timed.  Medians and interquartile spreads
over --reps calls, with and without the recovery:
  dev_ms          phant_timing's device region of phant_block_bodies_dev, every output, both roots expected
  host_ms         host-form wall time of phant_block_bodies, the same
  per_block_ms    host-form wall time of the per-block path of THIS build over the same blocks: n_blocks calls of
                  phant_block_transactions_ex (every output) plus n_blocks calls of phant_block_roots (two lists)
  parent_ms       the same loop through another build of the library (--parent-lib: libphant_gpu.so built from the parent
                  commit's own tree), in a context of its own
Needs a GPU.  One segment a process, each under a time limit of its own:
  for b in 1 16 64 256; do timeout -k 10 600 python tools/bench_bodies.py --blocks $b --fork london || break; done
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_senders import signers  # noqa: E402
from bench_transactions import mix  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--per-block", type=int, default=200)
    ap.add_argument("--unique", type=int, default=4)
    ap.add_argument("--fork", choices=("london", "prague"), default="london")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib")
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from phant_amd.types import block as X
    from tests import bodies_ref as B
    from tests import secp_ref as S
    from tests import tx_ref_forks as F

    O.build()
    rng = np.random.default_rng(2031)
    nb, per, fork = args.blocks, args.per_block, {"london": F.LONDON, "prague": F.PRAGUE}[args.fork]
    unique = min(args.unique, nb)
    who = signers(S, rng, per)
    made = [mix(S, O, rng, who, per, fork=fork) for _ in range(unique)]
    made = [m[0] if fork else m for m in made]
    blocks = [made[b % unique] for b in range(nb)]
    wds = [[B.withdrawal(16 * b + k, validator=k, address=bytes([k + 1]) * 20, amount=10**9 + k) for k in range(16)] for b in range(nb)]
    BASE_FEE, GAS_LIMIT, BLOB_FEE = 2 * 10**9, 30_000_000, 3
    kw = dict(base_fee=[BASE_FEE] * nb, gas_limit=[GAS_LIMIT] * nb, blob_base_fee=[BLOB_FEE] * nb)
    ctx = default_context()
    lib = ctx._lib
    a = X.pack_bodies(blocks, wds)
    n, n_wd = len(a["tx_off"]) - 1, len(a["wd_off"]) - 1

    # ---- the answers, before anything is timed
    exp, first_bad_block, first_bad, n_auth, blob_gas = B.expected(O, blocks, 1, fork, recover=True, block_wds=wds, **kw)
    txr = np.frombuffer(exp["transactions_root"], np.uint8).reshape(-1, 32)
    wdr = np.frombuffer(exp["withdrawals_root"], np.uint8).reshape(-1, 32)
    blob_used = np.frombuffer(exp["block_blob_gas_used"], "<u8")
    r = X.block_bodies(a, 1, fork, transactions_root=txr, withdrawals_root=wdr, blob_gas_used=blob_used, ctx=ctx, **kw)
    for name in B.TX_NAMES + B.AUTH_NAMES + B.BLOCK_NAMES:
        assert np.ascontiguousarray(getattr(r, name)).tobytes() == exp[name], name + " differs from the definition"
    assert (r.first_bad_block, r.first_bad, r.n_auth, r.blob_gas_used) == (nb, n, n_auth, blob_gas) and not r.sig_status.any()

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    def wall(fn):
        ms = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms[args.warmup:])

    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    fees = {k: np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in kw[k]), np.uint8).copy() for k in ("base_fee", "blob_base_fee")}
    limits = np.asarray(kw["gas_limit"], np.uint64)
    tx_outputs = [x for x in L.TX_OUTPUTS + L.TX_EX_OUTPUTS + L.TX_AUTH_OUTPUTS]
    cap = max(n_auth, 1)
    rows = lambda name: n + 1 if name == "auth_first" else cap if name.startswith("auth") else n  # noqa: E731

    def structs(up, recover):
        """phant_bodies_in / _out over `up(array)` pointers; -> (arg, out, what keeps the memory alive)"""
        keep = {k: up(v) for k, v in a.items()}
        keep.update(base_fee=up(fees["base_fee"]), blob_base_fee=up(fees["blob_base_fee"]), gas_limit=up(limits), transactions_root=up(txr.reshape(-1).copy()),
                    withdrawals_root=up(wdr.reshape(-1).copy()), blob_gas_used=up(blob_used.astype(np.uint64)))
        outs = {name: up(np.zeros(rows(name) * k * np.dtype(dt).itemsize + 8, np.uint8)) for name, dt, k in tx_outputs
                if recover or name not in ("sender", "sig_status", "authority", "auth_status")}
        own = {name: up(np.zeros((n if r_ == "n" else nb) * k * np.dtype(dt).itemsize + 8, np.uint8)) for name, dt, k, r_ in L.BODIES_OUTPUTS}
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data  # noqa: E731
        flags = L.TXS_HAVE_GAS_LIMIT | (0 if recover else L.TXS_NO_RECOVERY)
        arg = L.PhantBodiesIn(C.sizeof(L.PhantBodiesIn), fork, flags, nb, n, n_wd, cap, 0, 1, ptr(keep["txs"]), ptr(keep["tx_off"]), int(a["tx_off"][-1]),
                              ptr(keep["block_first"]), ptr(keep["withdrawals"]), ptr(keep["wd_off"]), int(a["wd_off"][-1]),
                              *[ptr(keep[k]) for k in L.BODIES_INPUTS[5:]])
        base = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[ptr(outs.get(name)) for name, _, _ in L.TX_OUTPUTS])
        xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0, 0, base, *[ptr(outs.get(name)) for name, _, _ in L.TX_EX_OUTPUTS + L.TX_AUTH_OUTPUTS])
        out = L.PhantBodiesOut(C.sizeof(L.PhantBodiesOut), 0, xout, *[ptr(own[name]) for name, _, _, _ in L.BODIES_OUTPUTS])
        return arg, out, (keep, outs, own)

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    res = {"blocks": nb, "per_block": per, "n": n, "bytes": int(a["tx_off"][-1]), "fork": args.fork, "n_auth": n_auth}
    for recover, tag in ((True, ""), (False, "_no_recovery")):
        arg, out, keep = structs(to_dev, recover)
        ctx.check(lib.phant_timing(ctx.handle, 1))
        ms = []
        try:
            for i in range(args.warmup + args.reps):
                ctx.check(lib.phant_block_bodies_dev(ctx.handle, C.byref(arg), C.byref(out)))
                assert out.first_bad_block == nb and out.txs.base.first_bad == n
                if i >= args.warmup:
                    ms.append(ctx.last_kernel_ms())
        finally:
            ctx.check(lib.phant_timing(ctx.handle, 0))
        res["dev" + tag + "_ms"] = stats(ms)
        ctx.sync()
        harg, hout, hkeep = structs(lambda x: np.ascontiguousarray(x), recover)

        def host_call():
            ctx.check(lib.phant_block_bodies(ctx.handle, C.byref(harg), C.byref(hout)))
        res["host" + tag + "_ms"] = wall(host_call)
        assert hout.first_bad_block == nb and hkeep[2]["transactions_root"][:32 * nb].tobytes() == exp["transactions_root"]

    # ---- the per-block path: phant_block_transactions_ex + phant_block_roots, a call each per block
    def per_block_loop(the_lib, handle, recover):
        calls = []
        for b in range(nb):
            lo, hi = int(a["block_first"][b]), int(a["block_first"][b + 1])
            m = hi - lo
            off = (a["tx_off"][lo:hi + 1] - a["tx_off"][lo]).astype(np.uint64)
            blob = a["txs"][int(a["tx_off"][lo]):int(a["tx_off"][hi])].copy() if m else np.zeros(1, np.uint8)
            wlo, whi = int(a["wd_first"][b]), int(a["wd_first"][b + 1])
            woff = (a["wd_off"][wlo:whi + 1] - a["wd_off"][wlo]).astype(np.uint64)
            wblob = a["withdrawals"][int(a["wd_off"][wlo]):int(a["wd_off"][whi])].copy()
            outs = {name: np.zeros((m + 1 if name == "auth_first" else cap if name.startswith("auth") else m) * k * np.dtype(dt).itemsize + 8, np.uint8)
                    for name, dt, k in tx_outputs if recover or name not in ("sender", "sig_status", "authority", "auth_status")}
            flags = L.TXS_HAVE_GAS_LIMIT | (0 if recover else L.TXS_NO_RECOVERY)
            tin = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), m, flags, 0, p(blob), p(off), int(off[-1]), 1, p(fees["base_fee"]), GAS_LIMIT)
            xin = L.PhantTxsExIn(C.sizeof(L.PhantTxsExIn), fork, tin, p(fees["blob_base_fee"]), cap, 0)
            base = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[p(outs.get(name)) for name, _, _ in L.TX_OUTPUTS])
            xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0, 0, base, *[p(outs.get(name)) for name, _, _ in L.TX_EX_OUTPUTS + L.TX_AUTH_OUTPUTS])
            items = (C.c_void_p * 2)(p(blob), p(wblob))
            offs = (C.c_void_p * 2)(p(off), p(woff))
            counts = (C.c_uint32 * 2)(m, whi - wlo)
            roots = np.zeros(64, np.uint8)
            calls.append((xin, xout, items, offs, counts, roots, (blob, off, wblob, woff, outs)))

        def run():
            for xin, xout, items, offs, counts, roots, _ in calls:
                rc = the_lib.phant_block_transactions_ex(handle, C.byref(xin), C.byref(xout))
                rc = rc or the_lib.phant_block_roots(handle, items, offs, counts, 2, roots.ctypes.data, None, None, None, 0, 0, None)
                assert rc == 0, rc
        t = wall(run)
        assert b"".join(c[5].tobytes()[:32] for c in calls) == exp["transactions_root"] and b"".join(c[5].tobytes()[32:] for c in calls) == exp["withdrawals_root"]
        assert b"".join(c[6][4]["flags"][:4 * int(c[0].base.n)].tobytes() for c in calls) == exp["flags"], "the per-block path's flags differ"
        return t

    for recover, tag in ((True, ""), (False, "_no_recovery")):
        res["per_block" + tag + "_ms"] = per_block_loop(lib, ctx.handle, recover)
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("phant_ctx_create", "phant_block_transactions_ex", "phant_block_roots"):
            fn = getattr(old, name)
            fn.restype, fn.argtypes = L.SYMBOLS[name]
        old.phant_ctx_destroy.restype, old.phant_ctx_destroy.argtypes = None, [C.c_void_p]
        h = C.c_void_p()
        opts = L.PhantOpts(C.sizeof(L.PhantOpts), torch.cuda.current_device(), None, 0)
        assert old.phant_ctx_create(C.byref(opts), C.byref(h)) == 0
        try:
            for recover, tag in ((True, ""), (False, "_no_recovery")):
                res["parent" + tag + "_ms"] = per_block_loop(old, h, recover)
        finally:
            old.phant_ctx_destroy(h)
    for tag in ("", "_no_recovery"):
        res["per_block_over_segment" + tag] = round(res["per_block" + tag + "_ms"]["median"] / res["host" + tag + "_ms"]["median"], 2)
    print(json.dumps({"bench": "bodies", **res}))


if __name__ == "__main__":
    main()
