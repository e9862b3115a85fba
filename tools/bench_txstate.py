#!/usr/bin/env python3
"""A block's transactions against the pre-state (phant_block_txs_prestate) beside one host core doing the same join: a JSON line per
block size and sender distribution.

For n = 200 / 2 000 / 10 000 transactions against tables of 500 / 5 000 / 25 000 pre-state rows, and three sender distributions --
`distinct` (every transaction its own sender), `skewed` (sender = row floor(n_accounts u^4): a few senders own most of the block) and
`single` (one sender owns all of it) --, medians and interquartile spreads over --reps calls:
  dev_ms        phant_timing's device region of phant_block_txs_prestate_dev, every output
  host_ms       host-form wall time, every output
  cpu_baseline  the same join, ranks, expected nonces and 320-bit sums as a plain C++ std::unordered_map loop on one core, compiled by
                this tool (g++ -O2), wall time
Every output is compared with tests/txstate_ref.py before anything is timed.  Needs a GPU.  One size a process, under a time limit:
  timeout -k 10 300 python tools/bench_txstate.py --sizes 200 && timeout -k 10 300 python tools/bench_txstate.py --sizes 2000 && \\
  timeout -k 10 300 python tools/bench_txstate.py --sizes 10000
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TABLE = {200: 500, 2000: 5000, 10000: 25000}

BASELINE = r"""
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
struct Key { uint8_t b[20]; bool operator==(const Key& o) const { return !std::memcmp(b, o.b, 20); } };
struct KeyHash { size_t operator()(const Key& k) const { uint64_t a, c; uint32_t d; std::memcpy(&a, k.b, 8); std::memcpy(&c, k.b + 8, 8);
    std::memcpy(&d, k.b + 16, 4); return (size_t)((a * 0x9E3779B97F4A7C15ull) ^ (c * 0xC2B2AE3D27D4EB4Full) ^ d); } };
// -> nanoseconds of one pass: the table, every sender and recipient located, rank, expected nonce, the sum so far (five 64-bit limbs),
// the nonce and balance verdicts
extern "C" uint64_t join_pass(uint32_t n, const uint8_t* sender, const uint8_t* to, const uint64_t* nonce, const uint8_t* cost, uint32_t na,
                              const uint8_t* addresses, const uint64_t* nonces, const uint8_t* balances, uint32_t* sender_row, uint32_t* to_row,
                              uint64_t* expected, uint32_t* flags) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<Key, uint32_t, KeyHash> row;
    row.reserve(2 * (size_t)na);
    for (uint32_t j = 0; j < na; ++j) { Key k; std::memcpy(k.b, addresses + 20ull * j, 20); row.emplace(k, j); }
    std::vector<uint32_t> sends(na, 0);
    std::vector<uint64_t> spent(5 * (size_t)na, 0);
    auto be = [](const uint8_t* p, uint64_t w[5]) { for (int q = 0; q < 4; ++q) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v = v << 8 | p[8 * (3 - q) + k]; w[q] = v; } w[4] = 0; };
    for (uint32_t i = 0; i < n; ++i) {
        Key k;
        std::memcpy(k.b, sender + 20ull * i, 20);
        auto s = row.find(k);
        std::memcpy(k.b, to + 20ull * i, 20);
        auto r = row.find(k);
        sender_row[i] = s == row.end() ? 0xffffffffu : s->second;
        to_row[i] = r == row.end() ? 0xffffffffu : r->second;
        uint32_t f = (s == row.end() ? 1u : 0u) | (r == row.end() ? 2u : 0u);
        if (s != row.end()) {
            const uint32_t j = s->second;
            expected[i] = nonces[j] + sends[j]++;
            f |= nonce[i] < expected[i] ? 4u : nonce[i] > expected[i] ? 8u : 0u;
            uint64_t c[5], b[5], *sum = &spent[5 * (size_t)j];
            be(cost + 32ull * i, c), be(balances + 32ull * j, b);
            unsigned __int128 carry = 0;
            for (int q = 0; q < 5; ++q) { carry += (unsigned __int128)sum[q] + c[q]; sum[q] = (uint64_t)carry; carry >>= 64; }
            for (int q = 4; q >= 0; --q) if (b[q] != sum[q]) { f |= b[q] < sum[q] ? 0x400u : 0u; break; }
        }
        flags[i] = f;
    }
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
"""


def baseline_lib(tmp):
    src, so = os.path.join(tmp, "join.cpp"), os.path.join(tmp, "join.so")
    with open(src, "w") as f:
        f.write(BASELINE)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.join_pass.restype = C.c_uint64
    lib.join_pass.argtypes = [C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 7
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,2000,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from tests import txstate_ref as R

    ctx = default_context()
    lib = ctx._lib
    rng = np.random.default_rng(2028)
    addr = lambda k: hashlib.sha256(b"bench" + int(k).to_bytes(8, "big")).digest()[:20]  # noqa: E731
    names = [name for name, _, _, _ in R.OUTPUTS]

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    with tempfile.TemporaryDirectory() as tmp:
        cpu = baseline_lib(tmp)
        for n in [int(x) for x in args.sizes.split(",") if x]:
            na = TABLE.get(n, 2 * n + 100)
            accounts = [R.account(addr(j), nonce=int(rng.integers(0, 10**6)), balance=((1 << 61) + int(rng.integers(1, 1 << 61))) << 40) for j in range(na)]
            for dist in ("distinct", "skewed", "single"):
                who = {"distinct": np.arange(n) % na, "skewed": (na * rng.random(n) ** 4).astype(int), "single": np.full(n, na // 3)}[dist]
                sent, txs = {}, []
                for i, j in enumerate(who.tolist()):
                    txs.append(R.tx(accounts[j]["address"], accounts[j]["nonce"] + sent.get(j, 0), int(rng.integers(1, 1 << 62)) << int(rng.integers(0, 30)),
                                    accounts[int(rng.integers(0, na))]["address"]))
                    sent[j] = sent.get(j, 0) + 1
                probes = [accounts[int(k)]["address"] for k in rng.integers(0, na, 16)]
                ins = R.inputs(txs, accounts, probes=probes)
                exp, first_bad, n_und = R.expected(R.PRAGUE, txs, accounts, probes=probes)
                counts = {"n": n, "n_accounts": na, "n_probe": len(probes)}
                width = {name: np.dtype(dt).itemsize * k * counts[rows] for name, dt, k, rows in R.OUTPUTS}

                def call(fn, ptr_in, ptr_out):
                    arg = L.PhantTxstateIn(C.sizeof(L.PhantTxstateIn), R.PRAGUE, n, 0, na, 0, len(probes), 0, *[ptr_in(k) for k in L.TXSTATE_INPUTS], 0,
                                           ptr_in("probe"))
                    out = L.PhantTxstateOut(C.sizeof(L.PhantTxstateOut), 0, 0, 0, *[ptr_out(k) for k in names])
                    ctx.check(fn(ctx.handle, C.byref(arg), C.byref(out)))
                    assert (out.first_bad, out.n_undetermined) == (first_bad, n_und)

                # ---- host form: the answers first, then the clock
                flat = {k: None if a is None or a.size == 0 else np.ascontiguousarray(a).reshape(-1).view(np.uint8) for k, a in ins.items()}
                bufs = {k: np.zeros(max(width[k], 8), np.uint8) for k in names}
                host = lambda: call(lib.phant_block_txs_prestate, lambda k: None if flat[k] is None else flat[k].ctypes.data,  # noqa: E731
                                    lambda k: bufs[k].ctypes.data)
                host()
                for k in names:
                    assert bufs[k][:width[k]].tobytes() == exp[k], k + " differs from the definition (host form)"
                ms = []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    host()
                    ms.append((time.perf_counter() - t0) * 1e3)
                res = {"n": n, "n_accounts": na, "senders": dist, "distinct_senders": len(sent), "host_ms": stats(ms[args.warmup:])}

                # ---- device form
                d_in = {k: None if a is None else torch.from_numpy(a.copy()).cuda() for k, a in flat.items()}
                d_out = {k: torch.zeros(max(width[k], 8), dtype=torch.uint8, device="cuda") for k in names}
                dev = lambda: call(lib.phant_block_txs_prestate_dev, lambda k: None if d_in[k] is None else d_in[k].data_ptr(),  # noqa: E731
                                   lambda k: d_out[k].data_ptr())
                ctx.check(lib.phant_timing(ctx.handle, 1))
                ms = []
                try:
                    for i in range(args.warmup + args.reps):
                        dev()
                        if i >= args.warmup:
                            ms.append(ctx.last_kernel_ms())
                finally:
                    ctx.check(lib.phant_timing(ctx.handle, 0))
                ctx.sync()
                for k in names:
                    assert d_out[k].cpu().numpy()[:width[k]].tobytes() == exp[k], k + " differs from the definition (device form)"
                res["dev_ms"] = stats(ms)

                # ---- one host core
                o = {"sender_row": np.zeros(n, np.uint32), "to_row": np.zeros(n, np.uint32), "expected": np.zeros(n, np.uint64), "flags": np.zeros(n, np.uint32)}
                p = lambda a: a.ctypes.data  # noqa: E731
                one = lambda: cpu.join_pass(n, p(ins["sender"]), p(ins["to"]), p(ins["nonce"]), p(ins["upfront_cost"]), na, p(ins["addresses"]),  # noqa: E731
                                            p(ins["nonces"]), p(ins["balances"]), p(o["sender_row"]), p(o["to_row"]), p(o["expected"]), p(o["flags"]))
                ns = [one() for _ in range(args.warmup + args.reps)][args.warmup:]
                assert o["sender_row"].tobytes() == exp["sender_row"] and o["to_row"].tobytes() == exp["to_row"] and o["expected"].tobytes() == exp["expected_nonce"]
                assert o["flags"].tobytes() == exp["state_flags"], "the host core's verdicts differ from the definition"
                res["cpu_baseline"] = dict(stats([x / 1e6 for x in ns]), cores=1, kind="std::unordered_map loop", unit="ms")
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
