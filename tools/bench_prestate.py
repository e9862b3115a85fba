#!/usr/bin/env python3
"""phant_exec_witness_prestate on a block-shaped execution witness: one JSON line.

The witness: a state of ~3 000 accounts, 400 of them contracts with 30 slots each (12 000 slots) and code of a length mix up to the
24 576-byte limit, every node once and shuffled, every key.  Reported (medians over --reps calls, after --warmup):
  host_ms          the call as the host sees it (copies in and out included)
  device_ms        phant_timing's region: every kernel of both streams, fork to join
  code_ms          the same region for the codes alone (a witness with the same codes and no keys)
  nodeset_ms       ... for the node-set part alone (the same witness without its codes: trie keys, set hash, two walks, decoding)
  overlap_ratio    device_ms / max(code_ms, nodeset_ms): 1.0 = the code hashing is entirely hidden beside the node-set kernels
  longest_code_ms  the 24 576-byte code alone, half wave per code (form 0) and lane per code (form 1)
Needs a GPU.  python tools/bench_prestate.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--accounts", type=int, default=3000)
    ap.add_argument("--contracts", type=int, default=400)
    ap.add_argument("--slots-per", type=int, default=30)
    args = ap.parse_args()

    import phant_amd
    from oracle import oracle as O
    from phant_amd.context import default_context
    from tests import prestate_ref as R

    O.build()
    rng = np.random.default_rng(2026)
    lens = np.where(rng.random(args.contracts) < 0.1, 24_576, rng.integers(100, 12_000, args.contracts))
    lens[0] = 24_576
    accounts = []
    for i in range(args.accounts):
        a = {"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1000)),
             "balance": int(rng.integers(0, 1 << 62)), "code": b"", "storage": {}}
        if i < args.contracts:
            a["code"] = rng.integers(0, 256, int(lens[i]), dtype=np.uint8).tobytes()
            a["storage"] = {int(rng.integers(0, 1 << 62)): int(rng.integers(1, 1 << 62)) for _ in range(args.slots_per)}
        accounts.append(a)
    doc, root = R.full_witness(O, accounts, rng)
    ctx = default_context()
    W = phant_amd.stateless.StatelessWitness

    def measure(d, form=0):
        w = W.parse_json(json.dumps(d))
        ctx.diag_set("code_hash_form", form)
        host, dev = [], []
        try:
            for r in range(args.warmup + args.reps):
                ctx.timing(True)
                t0 = time.perf_counter()
                out = w.prestate_arrays(ctx, root)
                t1 = time.perf_counter()
                ms = ctx.last_kernel_ms()
                ctx.timing(False)
                if r >= args.warmup:
                    host.append((t1 - t0) * 1e3)
                    dev.append(ms)
        finally:
            ctx.diag_set("code_hash_form", 0)
            w.close()
        return float(np.median(host)), float(np.median(dev)), out

    t0 = time.perf_counter()
    W.parse_json(json.dumps(doc)).close()
    parse_ms = (time.perf_counter() - t0) * 1e3
    host_ms, device_ms, out = measure(doc)
    assert out["n_failed"] == 0 and out["n_missing_code"] == 0, "the benchmark witness must verify"
    _, code_ms, _ = measure({"state": [], "codes": doc["codes"], "keys": []})
    _, nodeset_ms, _ = measure({"state": doc["state"], "keys": doc["keys"]})
    longest = {"state": [], "codes": [R._hex(accounts[0]["code"])], "keys": []}
    _, l0, _ = measure(longest, 0)
    _, l1, _ = measure(longest, 1)
    _, code_ms_lane, _ = measure({"state": [], "codes": doc["codes"], "keys": []}, 1)
    print(json.dumps({
        "bench": "exec_witness_prestate", "accounts": args.accounts, "slots": args.contracts * args.slots_per,
        "codes": len(doc["codes"]), "code_bytes": int(sum(len(a["code"]) for a in accounts)), "nodes": len(doc["state"]),
        "parse_ms": round(parse_ms, 3), "host_ms": round(host_ms, 3), "device_ms": round(device_ms, 4),
        "code_ms": round(code_ms, 4), "code_ms_lane_per_code": round(code_ms_lane, 4), "nodeset_ms": round(nodeset_ms, 4),
        "overlap_ratio": round(device_ms / max(code_ms, nodeset_ms), 3),
        "longest_code_ms": {"half_wave": round(l0, 4), "lane": round(l1, 4)}, "reps": args.reps}))


if __name__ == "__main__":
    main()
