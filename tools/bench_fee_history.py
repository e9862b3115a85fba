#!/usr/bin/env python3
"""Fee history over chain segments (phant_block_fee_history) beside numpy on one core: one JSON line.

Segments of --blocks blocks of --rows rows each against --percentiles percentiles, and one extra segment of a single block of
PHANT_FEEHIST_BLOCK_MAX rows -- what the quadratic ranking costs at its cap.  Tips below 2^63 with many ties, gas below 2^24 a row, a base
fee per block.  Before anything is timed the device's outputs (reward, order, block_gas_used, in both forms) are compared with
tests/feehist_ref.py where its loops stay below a few million steps, and with the numpy implementation -- itself compared with the ref on
those sizes -- beyond that.  Medians and interquartile spreads over --reps calls:
  dev_ms     phant_timing's device region of the _dev call, inputs resident
  host_ms    host-form wall time of the call, every output
  numpy_ms   the same answer in numpy on one core: per block a stable argsort over the tips AS uint64 (a 256-bit tip has no numpy dtype:
             this favours the core), a cumsum, a searchsorted per block
Needs a GPU.  Under a time limit of its own:  timeout -k 10 900 python tools/bench_fee_history.py
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 16, 256, 1024])
    ap.add_argument("--rows", type=int, nargs="*", default=[150, 1500])
    ap.add_argument("--percentiles", type=int, nargs="*", default=[3, 100])
    ap.add_argument("--no-cap-row", action="store_true", help="skip the single block of PHANT_FEEHIST_BLOCK_MAX rows")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from tests import feehist_ref as R

    rng = np.random.default_rng(1559)
    ctx = default_context()
    lib = ctx._lib

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    def wall(fn, reps=args.reps, warmup=args.warmup):
        ms = []
        for _ in range(warmup + reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms[warmup:])

    def timed(fn, reps=args.reps, warmup=args.warmup):
        """the device region of `reps` calls (HIP events around each call's launches)"""
        ctx.check(lib.phant_timing(ctx.handle, 1))
        ms = []
        try:
            for i in range(warmup + reps):
                fn()
                if i >= warmup:
                    ms.append(ctx.last_kernel_ms())
        finally:
            ctx.check(lib.phant_timing(ctx.handle, 0))
        ctx.sync()
        return stats(ms)

    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ptr = lambda x: None if x is None or not (x.numel() if hasattr(x, "numel") else x.size) else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data  # noqa: E731

    def be32(v):
        """uint64 values -> (len, 32) uint8 big-endian"""
        out = np.zeros((len(v), 32), np.uint8)
        out[:, 24:] = np.asarray(v, ">u8").view(np.uint8).reshape(-1, 8)
        return out

    def numpy_fee_history(first, tips, gas, pct):
        nb = len(first) - 1
        reward, order, total = np.zeros((nb, len(pct)), np.uint64), np.zeros(len(tips), np.uint32), np.zeros(nb, np.uint64)
        for b in range(nb):
            s, e = int(first[b]), int(first[b + 1])
            if s == e:
                continue
            o = np.argsort(tips[s:e], kind="stable")
            cum = np.cumsum(gas[s:e][o])
            at = np.minimum(np.searchsorted(cum, cum[-1] * pct // np.uint64(10000), side="left"), e - s - 1)
            order[s:e], reward[b], total[b] = o + s, tips[s:e][o][at], cum[-1]
        return reward, order, total

    def case(nb, rows, n_pct):
        n = nb * rows
        first = (np.arange(nb + 1, dtype=np.uint64) * rows).astype(np.uint32)
        base = rng.integers(1, 1 << 40, nb).astype(np.uint64)
        tips = np.where(rng.integers(0, 4, n) == 0, rng.integers(0, 8, n), rng.integers(0, 1 << 62, n)).astype(np.uint64)
        gas = rng.integers(0, 1 << 24, n).astype(np.uint64)
        pct = np.sort(rng.integers(0, 10001, n_pct)).astype(np.uint64) if n_pct > 3 else np.asarray([1000, 5000, 9000], np.uint64)[:n_pct]
        a = {"block_first": first, "price": be32(tips + np.repeat(base, rows)), "base_fee": be32(base), "gas_used": gas}
        reward, order, total = numpy_fee_history(first, tips, gas, pct)
        exp = {"reward": be32(reward.reshape(-1)).tobytes(), "order": order.tobytes(), "block_gas_used": total.tobytes()}
        checked = "numpy"
        if n + nb * n_pct * rows // 2 <= 3_000_000:
            ref, _ = R.expected(first.tolist(), (tips + np.repeat(base, rows)).tolist(), gas.tolist(), [int(p) for p in pct], base.tolist())
            assert all(ref[k] == exp[k] for k in exp), "numpy disagrees with tests/feehist_ref.py"
            checked = "ref"
        p32 = pct.astype(np.uint32)
        res = {"blocks": nb, "rows_per_block": rows, "rows": n, "percentiles": n_pct, "checked_against": checked}
        for dev in (True, False):
            ins = {k: to_dev(v) for k, v in a.items()} if dev else a
            outs = {"reward": np.zeros(32 * nb * n_pct, np.uint8), "tip": np.zeros(32 * n, np.uint8), "order": np.zeros(n, np.uint32),
                    "block_gas_used": np.zeros(nb, np.uint64), "block_flags": np.zeros(nb, np.uint32)}
            if dev:
                outs = {k: to_dev(v) for k, v in outs.items()}
            arg = L.PhantFeeHistoryIn(C.sizeof(L.PhantFeeHistoryIn), nb, n, n_pct, *[ptr(ins[k]) for k in ("block_first", "price", "base_fee", "gas_used")], p32.ctypes.data, 0)
            out = L.PhantFeeHistoryOut(C.sizeof(L.PhantFeeHistoryOut), 0, *[ptr(outs[k]) for k, _, _ in L.FEEHIST_OUTPUTS], 0)
            fn = lib.phant_block_fee_history_dev if dev else lib.phant_block_fee_history
            call = lambda: ctx.check(fn(ctx.handle, C.byref(arg), C.byref(out)))  # noqa: E731
            call()
            ctx.sync()
            got = {k: (v.cpu().numpy() if dev else v).tobytes() for k, v in outs.items()}
            assert out.first_bad_block == nb and all(got[k] == exp[k] for k in exp), "device disagrees"
            res["dev_ms" if dev else "host_ms"] = timed(call) if dev else wall(call)
        res["numpy_ms"] = wall(lambda: numpy_fee_history(first, tips, gas, pct), reps=min(args.reps, 5), warmup=1)
        return res

    out = {"bench": "fee_history", "block_max": L.FEEHIST_BLOCK_MAX, "segments": [], "cap": None}
    for nb in args.blocks:
        for rows in args.rows:
            for n_pct in args.percentiles:
                out["segments"].append(case(nb, rows, n_pct))
    if not args.no_cap_row:
        out["cap"] = case(1, L.FEEHIST_BLOCK_MAX, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
