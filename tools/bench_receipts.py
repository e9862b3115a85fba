#!/usr/bin/env python3
"""A block's receipts, fields in and header values out: one JSON line.

Block shapes: 100, 400, 1 000 and 10 000 receipts of 0-6 logs with 0-4 topics and 0-300 bytes of data each, and one block of 400
receipts in which a few logs carry 10 KB.  Per shape, medians over --reps calls of wall time (the calls synchronise), all from
arrays packed beforehand:
  new_ms             phant_block_receipts, host form: blooms, encodings, receipts root and block bloom from ONE call
  new_with_lists_ms  the same call with the block's transactions and withdrawals riding along (three roots)
  old_*_ms           the route that existed before, for the same answers: old_bloom_ms phant_logs_bloom (round trip 1), old_encode_ms
                     the receipts RLP-encoded on the host around those blooms, old_root_ms phant_index_root_rlp over the encodings
                     (round trip 2; old_roots_ms: phant_block_roots with the two lists), old_or_ms the host's OR of the rows
  old_gpu_calls_ms   old_bloom_ms + old_root_ms: what the two round trips alone cost, whatever encodes in between
The host encoder of the old route is tests/receipts_ref.py's (Python): old_encode_ms says what THAT encoder costs, not what a
native one would; compare new_ms with old_gpu_calls_ms for the round trips and add an encoder of your own.
Every output of the new call is compared with the reference before anything is timed.
Needs a GPU.  python tools/bench_receipts.py [--sizes 100,400,1000,10000] [--reps 20] [--warmup 3]
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


def make_block(rng, n, big=0):
    receipts, gas = [], 0
    for i in range(n):
        logs = []
        for _ in range(int(rng.integers(0, 7))):
            logs.append((rng.bytes(20), [rng.bytes(32) for _ in range(int(rng.integers(0, 5)))], rng.bytes(int(rng.integers(0, 301)))))
        gas += int(rng.integers(21000, 400000))
        receipts.append((int(rng.choice([0, 1, 2, 2, 2, 3])), bool(rng.random() < 0.95), gas, logs))
    for k in range(big):  # a few logs with 10 KB of data
        r = receipts[(k * 97 + 13) % n]
        r[3].append((rng.bytes(20), [rng.bytes(32)], rng.bytes(10 * 1024 + k)))
    txs = [b"\x02" + rng.bytes(int(rng.integers(110, 300))) for _ in range(n)]
    wds = [rng.bytes(int(rng.integers(40, 60))) for _ in range(16)]
    return receipts, txs, wds


def median_ms(fn, warmup, reps):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,400,1000,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import _lib as L, mpt
    from phant_amd.context import default_context
    from phant_amd.types import receipt as T
    from tests import receipts_ref as R

    O.build()
    ctx = default_context()
    lib = ctx._lib
    rng = np.random.default_rng(2027)
    shapes = [(f"{n}", n, 0) for n in (int(x) for x in args.sizes.split(","))] + [("400_with_10KB_logs", 400, 5)]
    out = {"tool": "bench_receipts", "reps": args.reps, "shapes": {}}
    p = lambda a: a.ctypes.data  # noqa: E731
    for name, n, big in shapes:
        receipts, txs, wds = make_block(rng, n, big)
        objs = [T.Receipt.init(ok, gas, [T.Log(*lg) for lg in logs], ty) for ty, ok, gas, logs in receipts]
        # ---- the answers, from the reference
        flat = [[x for a, ts, _ in r[3] for x in (a, *ts)] for r in receipts]
        want_rows = O.logs_bloom(flat)
        want_enc = [R.encode(r, want_rows[i].tobytes()) for i, r in enumerate(receipts)]
        for i in range(0, n, max(1, n // 8)):  # (the oracle's rows against the reference's own bloom, spot-checked: it hashes in Python)
            assert R.encode(receipts[i]) == want_enc[i]
        want_bloom = np.bitwise_or.reduce(want_rows, axis=0).tobytes()
        want_roots = [O.index_root_rlp(x) for x in (txs, want_enc, wds)]
        for lists, at in (((), 0), ((txs, wds), 1)):
            res = T.block_receipts(objs, ctx=ctx, other_lists=lists, receipts_at=at)
            assert res.encoded == want_enc and np.array_equal(res.blooms, want_rows) and res.logs_bloom == want_bloom, "outputs differ from the reference"
            assert res.receipts_root == want_roots[1] and (not lists or res.roots == want_roots), "roots differ from the reference"

        # ---- the new call, arrays packed beforehand
        a, n_, n_logs, n_topics, data_bytes = T.pack_receipts(objs)
        blobs = [mpt.pack_items(x) for x in (txs, wds)]
        lists_p = (C.c_void_p * 2)(*[p(b) for b, _ in blobs])
        offs_p = (C.c_void_p * 2)(*[p(o) for _, o in blobs])
        list_n = np.array([len(txs), len(wds)], np.uint32)
        total = sum(len(e) for e in want_enc)
        roots, bloom, rows = np.zeros((3, 32), np.uint8), np.zeros(256, np.uint8), np.zeros((n, 256), np.uint8)
        enc, enc_off = np.zeros(total, np.uint8), np.zeros(n + 1, np.uint64)

        def new_call(nl):
            arg = L.PhantReceiptsIn(C.sizeof(L.PhantReceiptsIn), n, n_logs, n_topics, data_bytes, *[p(a[k]) for k in (
                "tx_type", "status", "cum_gas", "log_first", "address", "topic_first", "data_off", "topics", "data")],
                C.cast(lists_p, C.c_void_p) if nl else None, C.cast(offs_p, C.c_void_p) if nl else None, p(list_n) if nl else None, None,
                nl, 1 if nl else 0)
            o = L.PhantReceiptsOut(C.sizeof(L.PhantReceiptsOut), n + 1, total, None, p(bloom), p(rows), p(enc), p(enc_off), p(roots), 0)
            ctx.check(lib.phant_block_receipts(ctx.handle, C.byref(arg), C.byref(o)))

        rec = {"receipts": n, "logs": n_logs, "topics": n_topics, "data_bytes": data_bytes, "encoded_bytes": total}
        rec["new_ms"] = median_ms(lambda: new_call(0), args.warmup, args.reps)
        assert roots[0].tobytes() == want_roots[1] and enc.tobytes() == b"".join(want_enc)
        rec["new_with_lists_ms"] = median_ms(lambda: new_call(2), args.warmup, args.reps)
        assert [r.tobytes() for r in roots] == want_roots

        # ---- the route that existed before
        fb, fo, fr, fn_items = T._flatten([[(a_, ts) for a_, ts, _ in r[3]] for r in receipts])
        old_rows = np.zeros((n, 256), np.uint8)
        rec["old_bloom_ms"] = median_ms(lambda: ctx.check(lib.phant_logs_bloom(ctx.handle, p(fb), p(fo), p(fr), fn_items, n, p(old_rows))),
                                        args.warmup, args.reps)
        assert np.array_equal(old_rows, want_rows)
        rec["old_encode_ms"] = median_ms(lambda: [R.encode(r, old_rows[i].tobytes()) for i, r in enumerate(receipts)], args.warmup, args.reps)
        eb, eo = mpt.pack_items(want_enc)
        root1 = np.zeros(32, np.uint8)
        rec["old_root_ms"] = median_ms(lambda: ctx.check(lib.phant_index_root_rlp(ctx.handle, p(eb), p(eo), n, p(root1))), args.warmup, args.reps)
        assert root1.tobytes() == want_roots[1]
        three = [blobs[0], (eb, eo), blobs[1]]
        item_p = (C.c_void_p * 3)(*[p(b) for b, _ in three])
        off_p = (C.c_void_p * 3)(*[p(o) for _, o in three])
        cnt = (C.c_uint32 * 3)(len(txs), n, len(wds))
        roots3 = np.zeros(96, np.uint8)
        rec["old_roots_ms"] = median_ms(lambda: ctx.check(lib.phant_block_roots(ctx.handle, item_p, off_p, cnt, 3, p(roots3), None, None, None, 0, 0, None)),
                                        args.warmup, args.reps)
        assert roots3.tobytes() == b"".join(want_roots)
        rec["old_or_ms"] = median_ms(lambda: np.bitwise_or.reduce(old_rows, axis=0), args.warmup, args.reps)
        rec["old_gpu_calls_ms"] = round(rec["old_bloom_ms"] + rec["old_root_ms"], 4)
        rec["old_gpu_calls_with_lists_ms"] = round(rec["old_bloom_ms"] + rec["old_roots_ms"], 4)
        rec["old_total_ms"] = round(rec["old_bloom_ms"] + rec["old_encode_ms"] + rec["old_root_ms"] + rec["old_or_ms"], 4)
        out["shapes"][name] = rec
        print(f"bench_receipts: {name} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
