#!/usr/bin/env python3
"""Execution requests of chain segments (phant_block_requests) and batched SHA-256 (phant_sha256_batch) beside hashlib on one core: one
JSON line.

requests: a segment of --blocks blocks, each with --logs ordinary logs (some of them the deposit contract's with another topic) and 0, 4
and 64 deposits among them, a withdrawal request (type 1, 76 bytes) and a consolidation request (type 2, 116 bytes) from the caller, every
header's hash expected.  The rows of the logs are packed by hand: `receipts` holds nothing but the logs' data.  Every output is compared
with tests/requests_ref.py before anything is timed.  Medians and interquartile spreads over --reps calls:
  dev_ms       phant_timing's device region of phant_block_requests_dev, every output, inputs resident
  host_ms      host-form wall time of phant_block_requests, the same
  hashlib_ms   hashlib.sha256 on one core over the SAME rows, already found and cut: the inner hashes and the outer hash of every block and
               nothing else (the scan of the logs is not timed, which favours the core)
  ref_ms       tests/requests_ref.py on one core, one pass: the scan, the layout checks, the rows and the hashes in Python
sha256: phant_sha256_batch_dev / phant_sha256_batch over 2^20 messages of 64 bytes and 2^16 of 193 bytes (a deposit request), beside
phant_keccak256_batch[_dev] over the same blobs and hashlib.sha256 in a loop on one core; rates in million messages a second from the
device region.
Needs a GPU.  Under a time limit of its own:  timeout -k 10 600 python tools/bench_requests.py
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTRACT = bytes.fromhex("00000000219ab540356cbb839cbe05303d7705fa")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--logs", type=int, default=32)
    ap.add_argument("--deposits", type=int, nargs="*", default=[0, 4, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sha", type=int, nargs="*", default=[20, 16], help="log2 of the message counts of the 64-byte and the 193-byte batch")
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from tests import requests_ref as Q

    rng = np.random.default_rng(7685)
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
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

    def to_dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data  # noqa: E731
    nb = args.blocks
    out = {"bench": "requests", "blocks": nb, "logs_per_block": args.logs, "segments": [], "sha256": []}

    # ------------------------------------------------------------------------------------------------ the segments
    for dpb in args.deposits:
        blob, address, topics, data_at, data_len, topic_first, log_first, block_first = [], [], [], [], [], [0], [0], [0]
        at = 0
        for b in range(nb):
            kinds = ["d"] * dpb + ["o"] * args.logs
            order = rng.permutation(len(kinds))
            for j in order:
                if kinds[j] == "d":
                    a, ts, d = CONTRACT, [Q.DEPOSIT_TOPIC], Q.deposit_event(rb(48), rb(32), rb(8), rb(96), rb(8))
                else:
                    a, ts, d = (CONTRACT if j % 11 == 0 else rb(20)), [rb(32), rb(32)], rb(64 + int(j) % 7)
                address.append(a), topics.extend(ts), data_at.append(at), data_len.append(len(d)), blob.append(d)
                topic_first.append(topic_first[-1] + len(ts))
                at += len(d)
            log_first.append(len(data_at))  # (a receipt a block)
            block_first.append(b + 1)
        other = [[(1, rb(76)), (2, rb(116))] for _ in range(nb)]
        rows = {"receipts": np.frombuffer(b"".join(blob), np.uint8), "block_first": np.asarray(block_first, np.uint32), "log_first": np.asarray(log_first, np.uint32),
                "address": np.frombuffer(b"".join(address), np.uint8), "topic_first": np.asarray(topic_first, np.uint32), "topics": np.frombuffer(b"".join(topics), np.uint8),
                "data_at": np.asarray(data_at, np.uint64), "data_len": np.asarray(data_len, np.uint32)}
        req, n_req = Q.pack_other(other, nb)
        t0 = time.perf_counter()
        exp, nd, first_bad = Q.expected(rows, CONTRACT, other)
        ref_ms = (time.perf_counter() - t0) * 1e3
        assert nd == nb * dpb and first_bad == nb
        ins = dict(rows, **req, active=None, requests_hash=np.frombuffer(exp["requests_hash"], np.uint8))
        nl, nt = len(data_at), len(topics)

        def structs(up):
            keep = {k: None if ins[k] is None else up(np.ascontiguousarray(ins[k], dt)) for k, dt in L.REQUESTS_INPUTS}
            count = {"n_blocks": nb, "n_deposits": max(nd, 1)}
            outs = {nm: up(np.zeros((count[r] + extra) * k * np.dtype(dt).itemsize + 8, np.uint8)) for nm, dt, k, r, extra in L.REQUESTS_OUTPUTS}
            arg = L.PhantRequestsIn(C.sizeof(L.PhantRequestsIn), nb, nb, nl, nt, n_req, nd, 0, ptr(keep["receipts"]), len(rows["receipts"]),
                                    *[ptr(keep[k]) for k, _ in L.REQUESTS_INPUTS[1:12]], int(req["req_off"][-1]), None, ptr(keep["requests_hash"]), (C.c_uint8 * 20)(*CONTRACT))
            res = L.PhantRequestsOut(C.sizeof(L.PhantRequestsOut), 0, 0, 0, *[ptr(outs[nm]) for nm, _, _, _, _ in L.REQUESTS_OUTPUTS])
            return arg, res, (keep, outs)

        def same(outs):
            got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in outs.items()}
            return all(got[k][:len(exp[k])].tobytes() == exp[k] for k in Q.OUTPUTS)

        seg = {"deposits_per_block": dpb, "n_logs": nl, "n_deposits": nd, "bytes": int(len(rows["receipts"]))}
        arg, res, keep = structs(to_dev)

        def dev_call():
            ctx.check(lib.phant_block_requests_dev(ctx.handle, C.byref(arg), C.byref(res)))
        seg["dev_ms"] = timed(dev_call)
        assert (res.n_deposits, res.first_bad_block) == (nd, nb) and same(keep[1])
        harg, hres, hkeep = structs(lambda x: np.ascontiguousarray(x))

        def host_call():
            ctx.check(lib.phant_block_requests(ctx.handle, C.byref(harg), C.byref(hres)))
        seg["host_ms"] = wall(host_call)
        assert (hres.n_deposits, hres.first_bad_block) == (nd, nb) and same(hkeep[1])

        first = np.frombuffer(exp["deposit_first"], "<u4").tolist()
        type0 = [b"\x00" + exp["deposit"][192 * first[b]:192 * first[b + 1]] for b in range(nb)]
        mine = [[bytes([t]) + d for t, d in other[b]] for b in range(nb)]

        def hashing():
            sha = hashlib.sha256
            got = [sha(b"".join(sha(m).digest() for m in ([type0[b]] if len(type0[b]) > 1 else []) + mine[b])).digest() for b in range(nb)]
            assert got[-1] == exp["requests_hash"][-32:]
        seg["hashlib_ms"] = wall(hashing, reps=5, warmup=1)
        seg["ref_ms"] = round(ref_ms, 2)
        seg["hashlib_over_host"] = round(seg["hashlib_ms"]["median"] / seg["host_ms"]["median"], 2)
        seg["hashlib_over_dev"] = round(seg["hashlib_ms"]["median"] / seg["dev_ms"]["median"], 2)
        out["segments"].append(seg)
        del keep, hkeep

    # ------------------------------------------------------------------------------------------------ the batches
    for log2n, length in zip(args.sha, (64, 193)):
        n = 1 << log2n
        blob = rng.integers(0, 256, n * length, dtype=np.uint8)
        off = (np.arange(n + 1, dtype=np.uint64) * length)
        d_blob, d_off = to_dev(blob), to_dev(off)
        d_out = torch.zeros(32 * n, dtype=torch.uint8).cuda()
        h_out = np.zeros(32 * n, np.uint8)
        t0 = time.perf_counter()
        want = b"".join(hashlib.sha256(blob[i * length:(i + 1) * length]).digest() for i in range(n))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        rec = {"n": n, "bytes": length, "hashlib_ms": round(cpu_ms, 2)}
        for name, dev_fn, host_fn in (("sha256", lib.phant_sha256_batch_dev, lib.phant_sha256_batch), ("keccak256", lib.phant_keccak256_batch_dev, lib.phant_keccak256_batch)):
            rec[name + "_dev_ms"] = timed(lambda: ctx.check(dev_fn(ctx.handle, d_blob.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr())))
            if name == "sha256":
                assert d_out.cpu().numpy().tobytes() == want
            rec[name + "_host_ms"] = wall(lambda: ctx.check(host_fn(ctx.handle, blob.ctypes.data, off.ctypes.data, n, h_out.ctypes.data)), reps=5, warmup=1)
            if name == "sha256":
                assert h_out.tobytes() == want
            rec[name + "_mmsg_per_s"] = round(n / rec[name + "_dev_ms"]["median"] / 1e3, 1)
        rec["hashlib_mmsg_per_s"] = round(n / cpu_ms / 1e3, 2)
        out["sha256"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
