#!/usr/bin/env python3
"""Wall time of the HOST form of phant_mpt_prove_nodeset (--form batch: of phant_mpt_prove_batch) on a small witness: one trie of --keys sorted 32-byte keys (values of 1 .. 80
bytes), --queries queried keys (a tenth of them absent), every output wanted.  Medians of --reps calls after --warmup calls, the
result checked against the oracle's union of proofs first.  Prints one JSON line.

    python tools/probe_prove_small.py [--keys 200] [--queries 10] [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=200)
    ap.add_argument("--queries", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--form", choices=("nodeset", "batch"), default="nodeset", help="batch: phant_mpt_prove_batch, checked against the oracle's proof lists")
    args = ap.parse_args()
    from oracle import oracle as O
    from phant_amd import mpt
    from tests.witness_util import random_kv

    O.build()
    rng = np.random.default_rng(200)
    keys, vals = random_kv(rng, args.keys, 32, 1, 80)
    absent = max(1, args.queries // 10)
    queries = [keys[i] for i in rng.choice(args.keys, args.queries - absent, replace=False)]
    queries += [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(absent)]
    kb, ko = mpt._pack(keys, np.uint32)
    vb, vo = mpt._pack(vals, np.uint64)
    qb, qo = mpt._pack(queries, np.uint32)
    trie = O.Trie(keys, vals)
    if args.form == "batch":
        call = lambda: mpt.prove_batch_packed(kb, ko, vb, vo, None, qb, qo)  # noqa: E731
        got = call()
        assert [got.proof(j) for j in range(len(queries))] == [trie.prove(q) for q in queries] and got.roots[0].tobytes() == trie.root()
    else:
        call = lambda: mpt.prove_nodeset_packed(kb, ko, vb, vo, None, qb, qo)  # noqa: E731
        got = call()
        want = set()
        for q in queries:
            want.update(trie.prove(q))
        assert set(got.trie_nodes(0)) == want and got.total_nodes == len(want) and got.roots[0].tobytes() == trie.root()
    ms = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        call()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"tool": "probe_prove_small", "form": args.form, "keys": args.keys, "queries": args.queries, "nodes": got.total_nodes, "reps": args.reps,
                      "host_form_wall_ms_median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "p90": round(float(np.percentile(ms, 90)), 4)}))


if __name__ == "__main__":
    main()
