#!/usr/bin/env python3
"""Receipts of chain segments from raw messages (phant_block_receipt_segments) beside the per-block path: one JSON line a wire form.

A segment is --blocks blocks of --per-block receipts of --logs logs each (two topics and 64 bytes of data a log, types 0 - 4 mixed).  Every
per-receipt and per-block output of the segment call is compared with tests/receipts_seg_ref.py before anything is timed.  Medians and
interquartile spreads over --reps calls, per form (consensus, eth69), with the root, bloom, gas and count of every block expected:
  dev_ms         phant_timing's device region of phant_block_receipt_segments_dev, every per-receipt and per-block output (eth69: and
                 the built encodings)
  host_ms        host-form wall time of phant_block_receipt_segments, the same
  per_block_ms   host-form wall time of n_blocks calls of phant_block_receipts from PRE-DECODED fields (the only route before this
                 call; the host decode that route needs is NOT timed, which favours it)
  ref_ms         tests/receipts_ref.py on one core, one pass: (consensus) decode every receipt, which checks its bloom, encode it again and
                 take the roots through the oracle; (eth69) the blooms, the encodings and the roots from the receipts' fields, no decode
Needs a GPU.  One segment a process, each under a time limit of its own:
  for b in 1 16 64 256; do timeout -k 10 600 python tools/bench_receipt_segments.py --blocks $b || break; done
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
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--per-block", type=int, default=200)
    ap.add_argument("--logs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from phant_amd.types import receipt as T
    from tests import receipts_ref as R
    from tests import receipts_seg_ref as G

    O.build()
    rng = np.random.default_rng(2032)
    nb, per = args.blocks, args.per_block
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    unique = [[(int(rng.integers(0, 5)), bool(rng.integers(0, 8)), 21000 * (i + 1) + int(rng.integers(0, 20000)), [(rb(20), [rb(32), rb(32)], rb(64)) for _ in range(args.logs)])
               for i in range(per)] for _ in range(min(nb, 4))]
    blocks = [unique[b % len(unique)] for b in range(nb)]
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

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data  # noqa: E731
    for form, name in ((G.CONSENSUS, "consensus"), (G.ETH69, "eth69")):
        raws = [[G.encode(r, form) for r in b] for b in unique]
        a = T.pack_receipt_segments([raws[b % len(unique)] for b in range(nb)])
        n, nbytes = len(a["rc_off"]) - 1, int(a["rc_off"][-1])
        # ---- the answers, before anything is timed: the definition over the distinct blocks, repeated
        exp_u, *_ = G.expected(raws, form)
        rep = lambda k, w: b"".join(exp_u[k][w * (b % len(unique)):w * (b % len(unique) + 1)] for b in range(nb))  # noqa: E731
        roots, blooms = rep("receipts_root", 32), rep("logs_bloom", 256)
        gas = np.frombuffer(rep("block_gas_used", 8), "<u8").copy()
        expect = {"receipts_root": np.frombuffer(roots, np.uint8).copy(), "logs_bloom": np.frombuffer(blooms, np.uint8).copy(), "gas_used": gas, "tx_count": np.full(nb, per, np.uint32)}
        r = T.receipt_segments(a, form=form, expect=expect, encoded=True, ctx=ctx)
        assert r.first_bad_block == nb and not r.flags.any() and r.receipts_root.tobytes() == roots and r.logs_bloom.tobytes() == blooms
        assert r.n_logs == n * args.logs and r.n_topics == 2 * r.n_logs and r.encoded == [G.encode_consensus(x) for b in blocks for x in b]

        def structs(up):
            keep = {k: up(v) for k, v in a.items()}
            keep.update({k: up(v) for k, v in expect.items()})
            skip = ("log_receipt", "address", "topic_first", "topics", "data_at", "data_len") + (("encoded", "encoded_off") if form == G.CONSENSUS else ())
            count = {"n": n, "n_blocks": nb, "encoded_len": nbytes + 268 * n}
            outs = {nm: up(np.zeros((count[rr] + extra) * k * np.dtype(dt).itemsize + 8, np.uint8)) for nm, dt, k, rr, extra in L.RSEG_OUTPUTS if nm not in skip}
            arg = L.PhantRcptSegsIn(C.sizeof(L.PhantRcptSegsIn), form, nb, n, 0, 0, (C.c_uint32 * 2)(0, 0), ptr(keep["receipts"]), ptr(keep["rc_off"]), nbytes,
                                    ptr(keep["block_first"]), *[ptr(keep[k]) for k in L.RSEG_INPUTS[3:]])
            out = L.PhantRcptSegsOut(C.sizeof(L.PhantRcptSegsOut), 0, 0, 0, count["encoded_len"], 0, *[ptr(outs.get(nm)) for nm, _, _, _, _ in L.RSEG_OUTPUTS])
            return arg, out, (keep, outs)

        res = {"form": name, "blocks": nb, "per_block": per, "logs": args.logs, "n": n, "bytes": nbytes}
        arg, out, keep = structs(to_dev)
        ctx.check(lib.phant_timing(ctx.handle, 1))
        ms = []
        try:
            for i in range(args.warmup + args.reps):
                ctx.check(lib.phant_block_receipt_segments_dev(ctx.handle, C.byref(arg), C.byref(out)))
                assert out.first_bad_block == nb
                if i >= args.warmup:
                    ms.append(ctx.last_kernel_ms())
        finally:
            ctx.check(lib.phant_timing(ctx.handle, 0))
        res["dev_ms"] = stats(ms)
        ctx.sync()
        harg, hout, hkeep = structs(lambda x: np.ascontiguousarray(x))

        def host_call():
            ctx.check(lib.phant_block_receipt_segments(ctx.handle, C.byref(harg), C.byref(hout)))
        res["host_ms"] = wall(host_call)
        assert hout.first_bad_block == nb and hkeep[1]["receipts_root"][:32 * nb].tobytes() == roots

        # ---- the per-block path: phant_block_receipts from fields, a call per block (the decode into fields is not timed)
        calls = []
        for b in blocks:
            f, m, n_logs, n_topics, data_bytes = T.pack_receipts([T.Receipt.init(ok, g, [T.Log(*lg) for lg in logs], t) for t, ok, g, logs in b])
            pin = L.PhantReceiptsIn(C.sizeof(L.PhantReceiptsIn), m, n_logs, n_topics, data_bytes, *[f[k].ctypes.data for k in
                                    ("tx_type", "status", "cum_gas", "log_first", "address", "topic_first", "data_off", "topics", "data")], None, None, None, None, 0, 0)
            o = {"root": np.zeros(32, np.uint8), "bloom": np.zeros(256, np.uint8), "rows": np.zeros(256 * max(m, 1), np.uint8)}
            pout = L.PhantReceiptsOut(C.sizeof(L.PhantReceiptsOut), 0, 0, o["root"].ctypes.data, o["bloom"].ctypes.data, o["rows"].ctypes.data, None, None, None, 0)
            calls.append((pin, pout, f, o))

        def per_block():
            for pin, pout, _, _ in calls:
                assert lib.phant_block_receipts(ctx.handle, C.byref(pin), C.byref(pout)) == 0
        res["per_block_ms"] = wall(per_block)
        assert b"".join(c[3]["root"].tobytes() for c in calls) == roots

        # ---- the Python reference on one core, one pass
        flat = [[G.encode_consensus(x) for x in b] for b in blocks] if form == G.CONSENSUS else None

        def reference():
            for b, block in enumerate(blocks):
                got = [R.decode(x) for x in flat[b]] if flat else block
                assert R.receipts_root(got) == roots[32 * b:32 * b + 32]
        res["ref_ms"] = wall(reference, reps=1, warmup=0)
        res["per_block_over_segment"] = round(res["per_block_ms"]["median"] / res["host_ms"]["median"], 2)
        res["ref_over_segment"] = round(res["ref_ms"]["median"] / res["host_ms"]["median"], 1)
        print(json.dumps({"bench": "receipt_segments", **res}))


if __name__ == "__main__":
    main()
