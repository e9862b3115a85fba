#!/usr/bin/env python3
"""phant_mpt_prove_nodeset_dev and phant_mpt_prove_batch_dev on a big trie: one JSON line.

A trie of --keys random 32-byte keys (values of 70 .. 110 bytes, a state trie's leaves), --queries random queries of which one in
ten is a key that is not stored.  Reported (medians over --reps calls, device time = phant_timing's region of the call):
  prove_device_ms     phant_mpt_prove_nodeset_dev: the build with its tables kept, locate / mark, sizes, offsets, the writing pass
  root_device_ms      phant_mpt_root_dev on the same trie (the build alone: what this feature must leave as it is)
  oracle_ms           the oracle's trie_build + one prove per query on one core (one run)
  prove_over_root     prove_device_ms / root_device_ms
The emitted set is checked against the oracle's union before anything is timed.
The per-proof leg, on the same trie, for --queries and for --more-queries queries ("batch" / "batch_more" in the line):
  batch_device_ms     phant_mpt_prove_batch_dev with every output wanted (median; _iqr: the interquartile spread)
  nodeset_device_ms   phant_mpt_prove_nodeset_dev on the same queries: the yardstick
  gather_ms           batch_device_ms minus the same call without a node blob (no gather launch): the gather kernel's share
  gather_GBps         the proof blob's bytes / gather_ms (written; as many are read from the set)
  oracle_prove_ms     the oracle's proofs of the same queries on one core (its trie built before)
Every proof list is compared with the oracle's before anything is timed.
Needs a GPU.  python tools/bench_prove.py [--keys 1000000] [--queries 3000] [--more-queries 100000] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state_witness_leg(O, ctx, args):
    """phant_state_witness on the state of tools/bench_prestate.py (3 000 accounts, 400 contracts x 30 slots, code up to 24 KiB), every
    address and slot touched: host wall time of the call (it has no device form), next to phant_state_root on the same arrays; the
    witness must resolve under its own root."""
    from phant_amd import state, stateless
    rng = np.random.default_rng(2026)
    lens = np.where(rng.random(400) < 0.1, 24_576, rng.integers(100, 12_000, 400))
    lens[0] = 24_576
    accounts, keys = [], []
    for i in range(3000):
        a = {"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1000)),
             "balance": int(rng.integers(0, 1 << 62)), "code": b"", "storage": {}}
        if i < 400:
            a["code"] = rng.integers(0, 256, int(lens[i]), dtype=np.uint8).tobytes()
            a["storage"] = {int(rng.integers(0, 1 << 62)): int(rng.integers(1, 1 << 62)) for _ in range(30)}
        accounts.append(state.AccountState(**a))
        keys.append(a["addr"])
        keys += [a["addr"] + s.to_bytes(32, "big") for s in a["storage"]]
    w = stateless.build_witness(accounts, keys, ctx=ctx)
    info = w.info()
    pre = w.prestate(ctx, w.state_root)
    assert w.state_root == O.state_root([vars(a) for a in accounts]) and pre.n_failed == 0 and len(pre.accounts) == 3000
    w.close()

    def wall(fn):
        ms = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            r = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            if hasattr(r, "close"):
                r.close()
        return float(np.median(ms[args.warmup:]))

    return {"state_witness_wall_ms": round(wall(lambda: stateless.build_witness(accounts, keys, ctx=ctx)), 3),
            "state_root_wall_ms": round(wall(lambda: state.state_root(accounts, ctx)), 3), "state_witness_keys": len(keys),
            "state_witness_nodes": int(info["total_nodes"]), "state_witness_codes": int(info["n_codes"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=3000)
    ap.add_argument("--more-queries", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import mpt
    from phant_amd.context import default_context

    O.build()
    rng = np.random.default_rng(2026)
    n, nq = args.keys, args.queries
    raw = np.unique(rng.integers(0, 256, (n + n // 50, 32), dtype=np.uint8), axis=0)[:n]  # (np.unique sorts rows lexicographically)
    n = raw.shape[0]
    vlen = rng.integers(70, 111, n)
    val_off = np.zeros(n + 1, np.uint64)
    val_off[1:] = np.cumsum(vlen)
    vals = rng.integers(0, 256, int(val_off[-1]), dtype=np.uint8)
    key_off = (np.arange(n + 1, dtype=np.uint64) * 32).astype(np.uint32)
    q = raw[rng.integers(0, n, nq)].copy()
    absent = rng.random(nq) < 0.1
    q[absent] = rng.integers(0, 256, (int(absent.sum()), 32), dtype=np.uint8)
    qkey_off = (np.arange(nq + 1, dtype=np.uint64) * 32).astype(np.uint32)

    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()  # noqa: E731
    d = [dev(raw.reshape(-1), np.uint8), dev(key_off, np.int32), dev(vals, np.uint8), dev(val_off, np.int64)]
    dq = [dev(q.reshape(-1), np.uint8), dev(qkey_off, np.int32)]
    ctx = default_context()
    tn, nl = mpt.prove_nodeset_dev(*d, None, *dq, None, None, None, None, ctx=ctx)
    nodes = torch.zeros(nl, dtype=torch.uint8, device="cuda")
    off = torch.zeros(tn + 1, dtype=torch.int64, device="cuda")
    root = torch.zeros(32, dtype=torch.uint8, device="cuda")
    status = torch.zeros(nq, dtype=torch.uint8, device="cuda")

    def prove():
        return mpt.prove_nodeset_dev(*d, None, *dq, None, None, nodes, off, None, root, status, ctx=ctx)

    assert prove() == (tn, nl)
    torch.cuda.synchronize()

    # the oracle, once: build + a proof per query; its union is what the GPU must have emitted
    keys_l = [raw[i].tobytes() for i in range(n)]
    vals_l = [vals[int(val_off[i]):int(val_off[i + 1])].tobytes() for i in range(n)]
    t0 = time.perf_counter()
    trie = O.Trie(keys_l, vals_l)
    want = set()
    for j in range(nq):
        want.update(trie.prove(q[j].tobytes()))
    oracle_ms = (time.perf_counter() - t0) * 1e3
    h_nodes, h_off = nodes.cpu().numpy(), off.cpu().numpy()
    got = {h_nodes[int(h_off[j]):int(h_off[j + 1])].tobytes() for j in range(tn)}
    assert got == want and len(want) == tn, "the emitted set differs from the oracle's union"
    assert root.cpu().numpy().tobytes() == trie.root()
    assert int((status.cpu().numpy() == mpt.PROOF_ABSENT).sum()) == int(absent.sum())

    def timed(fn, spread=False):
        ctx.check(ctx._lib.phant_timing(ctx.handle, 1))
        ms = []
        try:
            for i in range(args.warmup + args.reps):
                fn()
                if i >= args.warmup:
                    ms.append(ctx.last_kernel_ms())
        finally:
            ctx.check(ctx._lib.phant_timing(ctx.handle, 0))
        q1, med, q3 = (float(x) for x in np.percentile(ms, [25, 50, 75]))
        return (med, q3 - q1) if spread else med

    prove_ms = timed(prove)
    root_ms = timed(lambda: mpt.mptize_dev(*d, out=root, ctx=ctx))

    def batch_leg(qs, tag):
        """phant_mpt_prove_batch_dev over the queries `qs` (rows of 32 bytes) of the same trie"""
        m = qs.shape[0]
        dqs = [dev(qs.reshape(-1), np.uint8), dev((np.arange(m + 1, dtype=np.uint64) * 32).astype(np.uint32), np.int32)]
        btn, bnl = mpt.prove_batch_dev(*d, None, *dqs, None, None, None, ctx=ctx)
        b_nodes = torch.zeros(bnl, dtype=torch.uint8, device="cuda")
        b_off = torch.zeros(btn + 1, dtype=torch.int64, device="cuda")
        b_first = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        b_status = torch.zeros(m, dtype=torch.uint8, device="cuda")
        full = lambda: mpt.prove_batch_dev(*d, None, *dqs, None, b_nodes, b_off, b_first, root, b_status, ctx=ctx)  # noqa: E731
        assert full() == (btn, bnl)
        torch.cuda.synchronize()
        hn, ho, hf = b_nodes.cpu().numpy().tobytes(), b_off.cpu().numpy(), b_first.cpu().numpy()
        t0 = time.perf_counter()
        lists = [trie.prove(qs[j].tobytes()) for j in range(m)]
        oracle_prove_ms = (time.perf_counter() - t0) * 1e3
        for j in range(m):
            assert [hn[int(ho[k]):int(ho[k + 1])] for k in range(int(hf[j]), int(hf[j + 1]))] == lists[j], f"proof {j} differs from the oracle's"
        assert root.cpu().numpy().tobytes() == trie.root()
        sn, sl = mpt.prove_nodeset_dev(*d, None, *dqs, None, None, None, None, ctx=ctx)
        s_nodes, s_off = torch.zeros(sl, dtype=torch.uint8, device="cuda"), torch.zeros(sn + 1, dtype=torch.int64, device="cuda")
        b_ms, b_iqr = timed(full, True)
        nb_ms, _ = timed(lambda: mpt.prove_batch_dev(*d, None, *dqs, None, None, b_off, b_first, root, b_status, ctx=ctx), True)
        s_ms, s_iqr = timed(lambda: mpt.prove_nodeset_dev(*d, None, *dqs, None, None, s_nodes, s_off, None, root, b_status, ctx=ctx), True)
        gather_ms = b_ms - nb_ms
        return {tag: {"queries": m, "nodes": btn, "node_bytes": bnl, "batch_device_ms": round(b_ms, 4), "batch_device_ms_iqr": round(b_iqr, 4),
                      "nodeset_device_ms": round(s_ms, 4), "nodeset_device_ms_iqr": round(s_iqr, 4), "gather_ms": round(gather_ms, 4),
                      "gather_GBps": round(bnl / gather_ms / 1e6, 1) if gather_ms > 0 else None, "oracle_prove_ms": round(oracle_prove_ms, 1)}}

    legs = batch_leg(q, "batch")
    if args.more_queries:
        q2 = raw[rng.integers(0, n, args.more_queries)].copy()
        miss = rng.random(args.more_queries) < 0.1
        q2[miss] = rng.integers(0, 256, (int(miss.sum()), 32), dtype=np.uint8)
        legs.update(batch_leg(q2, "batch_more"))
    sw = state_witness_leg(O, ctx, args)
    print(json.dumps({"tool": "bench_prove", "keys": n, "queries": nq, "absent_queries": int(absent.sum()), "nodes": tn, "node_bytes": nl,
                      "prove_device_ms": round(prove_ms, 4), "root_device_ms": round(root_ms, 4), "oracle_ms": round(oracle_ms, 1),
                      "prove_over_root": round(prove_ms / root_ms, 3), "reps": args.reps, **legs, **sw}))


if __name__ == "__main__":
    main()
