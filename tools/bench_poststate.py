#!/usr/bin/env python3
"""phant_exec_witness_poststate on a block-shaped execution witness: one JSON line.

The witness of tools/bench_prestate.py (3 000 accounts, 400 contracts with 30 slots each = 12 000 slots, every node once and
shuffled, every key); the block writes 60 % of the keys, one write in ten a removal.  Reported (medians over --reps calls):
  poststate_device_ms  phant_timing's region of the call: the pre-state's node-set kernels and the post-state passes behind them
  prestate_device_ms   phant_exec_witness_prestate on the same document (without codes: the post-state call hashes none)
  oracle_state_root_ms the oracle's state_root over the FULL post-state on one core
  advance_device_ms    phant_exec_witness_advance on the same document and writes: the same kernels with the sink behind node_ref
                       (read against poststate_device_ms of the same run: advance_over_post), with the nodes and bytes it emitted
Needs a GPU.  python tools/bench_poststate.py [--reps 20] [--warmup 3]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--accounts", type=int, default=3000)
    ap.add_argument("--contracts", type=int, default=400)
    ap.add_argument("--slots-per", type=int, default=30)
    args = ap.parse_args()

    import phant_amd
    from oracle import oracle as O
    from phant_amd.context import default_context
    from tests import poststate_ref as Q
    from tests import prestate_ref as R

    O.build()
    rng = np.random.default_rng(2026)
    accounts = []
    for i in range(args.accounts):
        a = {"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1000)),
             "balance": int(rng.integers(0, 1 << 62)), "code": b"", "storage": {}}
        if i < args.contracts:
            a["code"] = rng.integers(0, 256, 200, dtype=np.uint8).tobytes()
            a["storage"] = {int(rng.integers(0, 1 << 62)): int(rng.integers(1, 1 << 62)) for _ in range(args.slots_per)}
        accounts.append(a)
    doc, root = R.full_witness(O, accounts, rng)
    doc.pop("codes", None)
    writes, n_writes, n_removed = {}, 0, 0
    for a in accounts:
        upd = {}
        for s in a["storage"]:
            if rng.random() < 0.6:
                upd[s] = 0 if rng.random() < 0.1 else int(rng.integers(1, 1 << 62))
                n_removed += upd[s] == 0
        if rng.random() < 0.6:
            if rng.random() < 0.1:
                writes[a["addr"]] = None
                n_removed += 1
            else:
                writes[a["addr"]] = {"nonce": a["nonce"] + 1, "balance": a["balance"] + 1, "code": a["code"], "storage": upd}
            n_writes += 1 + len(upd)
        elif upd:
            writes[a["addr"]] = ("keep", upd)
            n_writes += len(upd)
    ctx = default_context()
    w = phant_amd.stateless.StatelessWitness.parse_json(json.dumps(doc))
    info = w.info()
    arrays = Q.write_arrays(O, info, writes)

    def measure(call):
        dev = []
        for r in range(args.warmup + args.reps):
            ctx.timing(True)
            out = call()
            ms = ctx.last_kernel_ms()
            ctx.timing(False)
            if r >= args.warmup:
                dev.append(ms)
        return float(np.median(dev)), out

    post_ms, got = measure(lambda: w.poststate_arrays(ctx, root, arrays))
    pre_ms, pre = measure(lambda: w.prestate_arrays(ctx, root))
    emitted = {}

    def advance():
        out, nxt = w.advance_arrays(ctx, root, arrays)
        if nxt is not None:
            i = nxt.info()
            emitted.update(nodes=int(i["total_nodes"]), bytes=int(i["nodes_len"]))
            nxt.close()
        return out

    adv_ms, adv = measure(advance)
    assert adv["n_failed"] == 0 and adv["state_root"] == got["state_root"] and emitted, "the benchmark witness must advance"
    after = Q.apply_writes(accounts, writes)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = O.state_root(after)
        t.append((time.perf_counter() - t0) * 1e3)
    assert got["n_failed"] == 0 and pre["n_failed"] == 0 and got["state_root"] == want, "the benchmark witness must re-root"
    w.close()
    print(json.dumps({"bench": "exec_witness_poststate", "accounts": args.accounts, "slots": info["n_slots"], "nodes": info["total_nodes"],
                      "writes": n_writes, "removals": int(n_removed), "poststate_device_ms": round(post_ms, 4),
                      "prestate_device_ms": round(pre_ms, 4), "oracle_state_root_ms": round(float(np.median(t)), 3),
                      "post_over_pre": round(post_ms / pre_ms, 2), "advance_device_ms": round(adv_ms, 4),
                      "advance_over_post": round(adv_ms / post_ms, 3), "advance_nodes": emitted["nodes"],
                      "advance_bytes": emitted["bytes"], "reps": args.reps}))


if __name__ == "__main__":
    main()
