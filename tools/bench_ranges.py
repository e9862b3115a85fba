#!/usr/bin/env python3
"""phant_mpt_verify_ranges on the shapes snap sync has: one JSON line per shape and per setting of the leaf pass.

  small     one range of 256 leaves with 80-byte values, cut from a trie of 2^20 keys: below what the call's launches cost, a CPU core wins
  one       one range of 4 096 such leaves
  many      64 such ranges in one call
  storage   512 whole tries of 8 leaves without a proof plus one proven range of 2 000 (StorageRanges)

Every output is compared with the definition (tests/range_ref.py), or -- `many`: the definition takes a quarter of a minute there -- every
range must be valid with the trie's root computed, before anything is timed.  Reported (medians over --reps calls, with the interquartile
spread):
  device_ms   phant_timing's region of the host-form call: the node set's hash and every range kernel
  wall_ms     the host-form call from Python, packed arrays in, results out
next to two yardsticks that are not the code under test:
  oracle_mptize_ms   oracle.mptize on one core over the same leaves, range by range: the least a CPU verifier must do
  mpt_root_ms        phant_mpt_root over the same leaves as ONE sorted trie: the floor -- as many leaf hashes and about as many branches,
                     without proofs, from the tuned hasher
Each shape runs twice: with the leaf pass (leaf_pass 1) and with PHANT_DIAG_RANGES_NO_LEAF_PASS set, the leaves then being hashed by the
lanes that build their parents, as in the post-state build.
Needs a GPU.  python tools/bench_ranges.py [--reps 20] [--warmup 3] [--keys 1048576]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(xs):
    q = np.percentile(np.array(xs, float), [25, 50, 75])
    return round(float(q[1]), 4), round(float(q[2] - q[0]), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--leaves", type=int, default=4096)
    args = ap.parse_args()

    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import mpt
    from phant_amd.context import default_context
    from tests import range_ref as R

    O.build()
    O.lib()
    ctx = default_context()
    rng = np.random.default_rng(2026)
    raw = np.unique(rng.integers(0, 256, (args.keys, 32), dtype=np.uint8), axis=0)
    keys = [k.tobytes() for k in raw]
    vals = [rng.integers(0, 256, 80, dtype=np.uint8).tobytes() for _ in keys]
    t0 = time.perf_counter()
    big = O.Trie(keys, vals)
    root = big.root()
    print(json.dumps({"trie_keys": len(keys), "oracle_trie_build_s": round(time.perf_counter() - t0, 2)}), flush=True)

    def cut(first, count):
        leaves = list(zip(keys[first:first + count], vals[first:first + count]))
        return (root, keys[first], leaves, True), big.prove(keys[first]) + big.prove(leaves[-1][0])

    shapes = {}
    r, nd = cut(len(keys) // 5, 256)
    shapes["small"] = ([r], nd, True)
    r, nd = cut(len(keys) // 3, args.leaves)
    shapes["one"] = ([r], nd, True)
    parts = [cut(1000 + i * (len(keys) // 70), args.leaves) for i in range(64)]
    shapes["many"] = ([p[0] for p in parts], [x for p in parts for x in p[1]], False)
    small, first = [], 5_000
    for i in range(512):
        ks = sorted(rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(8))
        vs = [rng.integers(1, 256, 32, dtype=np.uint8).tobytes() for _ in ks]
        small.append((O.mptize(ks, vs), bytes(32), list(zip(ks, vs)), False))
    r, nd = cut(first, 2000)
    shapes["storage"] = (small + [r], nd, True)

    for name, (ranges, nodes, by_definition) in shapes.items():
        packed = mpt.pack_ranges([mpt.Range(*x) for x in ranges], nodes)
        n_leaves = sum(len(x[2]) for x in ranges)
        # the yardsticks
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _, _, leaves, _ in ranges:
                O.mptize([k for k, _ in leaves], [v for _, v in leaves])
            ms.append(1e3 * (time.perf_counter() - t0))
        oracle_ms = round(min(ms), 3)
        both = sorted({k: v for x in ranges for k, v in x[2]}.items())
        kb, ko = mpt._pack([k for k, _ in both], np.uint32)
        vb, vo = mpt._pack([v for _, v in both], np.uint64)
        assert mpt.mptize_packed(kb, ko, vb, vo, ctx) == O.mptize([k for k, _ in both], [v for _, v in both])
        floor = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            mpt.mptize_packed(kb, ko, vb, vo, ctx)
            if i >= args.warmup:
                floor.append(1e3 * (time.perf_counter() - t0))
        for leaf_pass in (1, 0):
            ctx.diag_set("ranges_no_leaf_pass", 0 if leaf_pass else 1)
            try:
                res = mpt.verify_ranges_packed(*packed, ctx=ctx)
                if by_definition:
                    want = R.verify_call(ranges, nodes)
                    got = list(zip(res.status.tolist(), res.has_more.tolist(), [x.tobytes() for x in res.computed_root], res.bad_leaf.tolist()))
                    assert got == want, name
                else:
                    assert all(res.valid(i) and res.computed_root[i].tobytes() == ranges[i][0] for i in range(len(ranges))), name
                    assert res.n_failed == 0 and list(res.has_more) == [1] * len(ranges)
                ctx.timing(True)
                dev, wall = [], []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    mpt.verify_ranges_packed(*packed, ctx=ctx)
                    w = 1e3 * (time.perf_counter() - t0)
                    if i >= args.warmup:
                        wall.append(w)
                        dev.append(ctx.last_kernel_ms())
                ctx.timing(False)
            finally:
                ctx.diag_set("ranges_no_leaf_pass", 0)
            d, w, f = quartiles(dev), quartiles(wall), quartiles(floor)
            print(json.dumps({"shape": name, "leaf_pass": leaf_pass, "ranges": len(ranges), "leaves": n_leaves, "nodes": len(nodes),
                              "device_ms": d[0], "device_iqr_ms": d[1], "wall_ms": w[0], "wall_iqr_ms": w[1], "oracle_mptize_ms": oracle_ms,
                              "mpt_root_ms": f[0], "mpt_root_iqr_ms": f[1], "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
