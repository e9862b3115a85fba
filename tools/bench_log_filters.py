#!/usr/bin/env python3
"""Log filters over chain segments (phant_block_log_filters, phant_log_filters_bloom) beside numpy on one core: one JSON line.

exact: segments of 1, 16 and 256 blocks of --logs logs (two topics each, addresses and topics drawn from a pool so that filters select
something) against 1, 64 and 1024 filters whose sets have one entry (an address and a first topic) or 1000 addresses.  bloom: 2^10, 2^16
and 2^20 blooms of --logs logs' worth of bits against the same filter counts, single-entry sets.  crossover: 256 blocks, 64 filters, address
sets of 1 .. 64 entries with every set forced through the table and forced entry by entry (PHANT_DIAG_LOGFILTER_SETS).
Before anything is timed the device's outputs are compared with the numpy implementation, and that implementation with
tests/filters_ref.py wherever n_filters x n_logs (n_blooms) is at most 2^18 -- the Python definition takes minutes beyond that.
Medians and interquartile spreads over --reps calls:
  dev_ms     phant_timing's device region of the _dev call, inputs resident
  host_ms    host-form wall time of the call, every output
  numpy_ms   the same filters in numpy on one core over ids the logs' addresses and topics were mapped to beforehand (np.isin per set;
             the mapping is not timed, which favours the core); blooms: a byte test per bit.  Not measured beyond 2^26 filter x bloom pairs.
  GBps       (bloom) the blooms' bytes over dev_ms
Needs a GPU.  Under a time limit of its own:  timeout -k 10 900 python tools/bench_log_filters.py
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
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--logs", type=int, default=100)
    ap.add_argument("--filters", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--blooms", type=int, nargs="*", default=[10, 16, 20], help="log2 of the bloom counts")
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 2, 4, 8, 12, 16, 32, 64], help="set sizes of the crossover")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from tests import filters_ref as F

    rng = np.random.default_rng(6110)
    ctx = default_context()
    lib = ctx._lib
    POOL = 4096
    pool_addr = rng.integers(0, 256, (POOL, 20), dtype=np.uint8)
    pool_topic = rng.integers(0, 256, (POOL, 32), dtype=np.uint8)

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

    def make_filters(nf, size, with_topic):
        """-> (addr ids per filter, topic-0 ids per filter): `size` addresses each; single-entry filters also name a first topic"""
        a_ids = [rng.choice(POOL, size, replace=False) if size <= POOL else rng.integers(0, POOL, size) for _ in range(nf)]
        t_ids = [rng.integers(0, POOL, 1) if with_topic else np.zeros(0, np.int64) for _ in range(nf)]
        return a_ids, t_ids

    def pack_filters(a_ids, t_ids, n_range):
        nf = len(a_ids)
        tf = np.zeros(4 * nf + 1, np.uint32)
        tf[1:] = np.cumsum(np.asarray([[len(t), 0, 0, 0] for t in t_ids]).reshape(-1))
        return {"addr_first": np.cumsum([0] + [len(a) for a in a_ids]).astype(np.uint32), "addr": pool_addr[np.concatenate(a_ids)].reshape(-1),
                "topic_first": tf, "topic": pool_topic[np.concatenate(t_ids).astype(np.int64)].reshape(-1), "block_lo": np.zeros(nf, np.uint32),
                "block_hi": np.full(nf, n_range, np.uint32)}

    def filters_struct(fa, nf):
        return L.PhantLogFilters(C.sizeof(L.PhantLogFilters), nf, len(fa["addr"]) // 20 if not hasattr(fa["addr"], "numel") else fa["addr"].numel() // 20,
                                 (fa["topic"].numel() if hasattr(fa["topic"], "numel") else len(fa["topic"])) // 32, *[ptr(fa[k]) for k, _ in L.LOG_FILTER_ARRAYS], 0)

    def ref_filters(a_ids, t_ids):
        return [F.Filter([pool_addr[i].tobytes() for i in a], [[pool_topic[i].tobytes() for i in t]]) for a, t in zip(a_ids, t_ids)]

    # ------------------------------------------------------------------------------------------------ the exact call
    def numpy_exact(log_a, log_t0, a_ids, t_ids):
        first, match = [0], []
        for a, t in zip(a_ids, t_ids):
            m = np.isin(log_a, a)
            if len(t):
                m &= np.isin(log_t0, t)
            match.append(np.flatnonzero(m))
            first.append(first[-1] + len(match[-1]))
        return np.asarray(first, np.uint32), np.concatenate(match).astype(np.uint32)

    def exact_case(nb, nf, size, sets=0, numpy_too=True):
        nl = nb * args.logs
        log_a, log_t0, log_t1 = rng.integers(0, POOL, nl), rng.integers(0, POOL, nl), rng.integers(0, POOL, nl)
        rows = {"block_first": np.arange(nb + 1, dtype=np.uint32), "log_first": (np.arange(nb + 1) * args.logs).astype(np.uint32), "address": pool_addr[log_a].reshape(-1),
                "topic_first": (2 * np.arange(nl + 1)).astype(np.uint32), "topics": np.stack([pool_topic[log_t0], pool_topic[log_t1]], axis=1).reshape(-1)}
        a_ids, t_ids = make_filters(nf, size, with_topic=size == 1)
        fa = pack_filters(a_ids, t_ids, nb)
        first, match = numpy_exact(log_a, log_t0, a_ids, t_ids)
        if nf * nl <= 1 << 18:
            exp, _ = F.expected_matches(rows, ref_filters(a_ids, t_ids))
            assert exp["filter_first"] == first.tobytes() and exp["match_log"] == match.tobytes(), "numpy disagrees with tests/filters_ref.py"
        cap = max(len(match), 1)
        ctx.diag_set("logfilter_sets", sets)
        try:
            res = {"blocks": nb, "logs": nl, "filters": nf, "set_size": size, "matches": int(len(match))}
            for dev in (True, False):
                r, f = ({k: to_dev(v) for k, v in rows.items()}, {k: to_dev(v) for k, v in fa.items()}) if dev else (rows, fa)
                outs = {"filter_first": np.zeros(nf + 1, np.uint32), "match_log": np.zeros(cap, np.uint32), "filter_count": np.zeros(nf, np.uint32)}
                if dev:
                    outs = {k: to_dev(v).view(torch.int32) for k, v in outs.items()}
                arg = L.PhantLogMatchIn(C.sizeof(L.PhantLogMatchIn), nb, nb, nl, 2 * nl, cap, 0, 0, *[ptr(r[k]) for k, _ in L.LOGMATCH_INPUTS])
                flt = filters_struct(f, nf)
                out = L.PhantLogMatchOut(C.sizeof(L.PhantLogMatchOut), 0, 0, 0, *[ptr(outs[k]) for k in L.LOGMATCH_OUTPUTS])
                fn = lib.phant_block_log_filters_dev if dev else lib.phant_block_log_filters
                call = lambda: ctx.check(fn(ctx.handle, C.byref(arg), C.byref(flt), C.byref(out)))  # noqa: E731
                call()
                ctx.sync()
                got = {k: (v.cpu().numpy().view(np.uint32) if dev else v) for k, v in outs.items()}
                assert out.n_matches == len(match) and np.array_equal(got["filter_first"], first) and np.array_equal(got["match_log"][:len(match)], match), "device disagrees"
                res["dev_ms" if dev else "host_ms"] = timed(call) if dev else wall(call)
        finally:
            ctx.diag_set("logfilter_sets", 0)
        if numpy_too:
            res["numpy_ms"] = wall(lambda: numpy_exact(log_a, log_t0, a_ids, t_ids), reps=min(args.reps, 5), warmup=1)
        return res

    out = {"bench": "log_filters", "logs_per_block": args.logs, "linear_max": L.LOGFILTER_LINEAR_MAX, "exact": [], "bloom": [], "crossover": []}
    for nb in args.blocks:
        for nf in args.filters:
            for size in (1, 1000):
                out["exact"].append(exact_case(nb, nf, size))
    for size in args.sizes:
        for name, sets in (("table", 1), ("linear", 2)):
            r = exact_case(256, 64, size, sets=sets, numpy_too=False)
            out["crossover"].append({"set_size": size, "sets": name, "dev_ms": r["dev_ms"]})

    # ------------------------------------------------------------------------------------------------ the bloom call
    def entry_bits(entries):
        return [[F.bloom_bits(e.tobytes()) for e in s] for s in entries]

    def numpy_bloom(blooms, bits_a, bits_t):
        may = np.zeros((len(bits_a), len(blooms)), bool)
        for f, (sa, st) in enumerate(zip(bits_a, bits_t)):
            ok = np.ones(len(blooms), bool)
            for s in (sa, st):
                if s:
                    some = np.zeros(len(blooms), bool)
                    for e in s:
                        some |= ((blooms[:, e[0][0]] & e[0][1]) != 0) & ((blooms[:, e[1][0]] & e[1][1]) != 0) & ((blooms[:, e[2][0]] & e[2][1]) != 0)
                    ok &= some
            may[f] = ok
        return may

    for lg in args.blooms:
        n = 1 << lg
        # a bloom of --logs logs: 3 bits for each of their addresses and two topics, as random positions
        # (1 024 distinct ones, drawn n times)
        base = np.zeros((1024, 256), np.uint8)
        pos = rng.integers(0, 2048, (1024, 9 * args.logs))
        np.bitwise_or.at(base, (np.repeat(np.arange(1024), pos.shape[1]), (pos // 8).reshape(-1)), (1 << (pos % 8)).astype(np.uint8).reshape(-1))
        blooms = base[rng.integers(0, 1024, n)]
        d_blooms = to_dev(blooms)
        for nf in args.filters:
            a_ids, t_ids = make_filters(nf, 1, with_topic=True)
            fa = pack_filters(a_ids, t_ids, n)
            pairs = nf * n
            bits_a, bits_t = entry_bits([pool_addr[a] for a in a_ids]), entry_bits([pool_topic[t] for t in t_ids])
            exp = numpy_bloom(blooms, bits_a, bits_t) if pairs <= 1 << 26 else None
            if pairs <= 1 << 18:
                ref_may, _ = F.expected_may([b.tobytes() for b in blooms], ref_filters(a_ids, t_ids))
                assert np.packbits(exp, axis=1, bitorder="little").tobytes() == np.frombuffer(ref_may, np.uint8).reshape(nf, -1)[:, :(n + 7) // 8].tobytes(), "numpy disagrees with the ref"
            res = {"blooms": n, "filters": nf}
            words = (n + 63) // 64
            for dev in (True, False):
                if not dev and n * 256 > 1 << 26:
                    continue  # (the host form copies the blooms in: 256 MiB a call at 2^20)
                f = {k: to_dev(v) for k, v in fa.items()} if dev else fa
                may, count = np.zeros((nf, words), np.uint64), np.zeros(nf, np.uint32)
                if dev:
                    may, count = to_dev(may).view(torch.int64), to_dev(count).view(torch.int32)
                flt = filters_struct(f, nf)
                fn = lib.phant_log_filters_bloom_dev if dev else lib.phant_log_filters_bloom
                call = lambda: ctx.check(fn(ctx.handle, ptr(d_blooms if dev else blooms), n, C.byref(flt), ptr(may), ptr(count)))  # noqa: E731
                call()
                ctx.sync()
                if exp is not None:
                    got = (may.cpu().numpy() if dev else may).view(np.uint8).reshape(nf, -1)
                    assert np.array_equal(np.unpackbits(got, axis=1, bitorder="little")[:, :n].astype(bool), exp), "device disagrees"
                res["dev_ms" if dev else "host_ms"] = timed(call) if dev else wall(call, reps=min(args.reps, 10))
            res["GBps"] = round(n * 256 / (res["dev_ms"]["median"] * 1e-3) / 1e9, 1)
            if exp is not None:
                res["numpy_ms"] = wall(lambda: numpy_bloom(blooms, bits_a, bits_t), reps=3, warmup=1)
            res["candidates_per_filter"] = None if exp is None else round(float(exp.sum()) / nf, 1)
            out["bloom"].append(res)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
