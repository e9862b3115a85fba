#!/usr/bin/env python3
"""A block of plain transfers settled (phant_block_settle) beside one host core running the same loop: a JSON line per block size and
sender distribution.

For n = 200 / 2 000 / 10 000 transfers against tables of 500 / 5 000 / 25 000 pre-state rows, 16 withdrawals, and three sender
distributions -- `distinct` (every transaction its own sender), `skewed` (sender = row floor(n_accounts u^4): a few senders own most of
the block) and `single` (one sender owns all of it); every transaction pays the one coinbase --, medians and interquartile spreads over
--reps calls:
  dev_ms        phant_timing's device region of phant_block_settle_dev, every output
  host_ms       host-form wall time, every output
  cpu_baseline  applyBody's loop over the same rows -- gas, the exact balance check, debit, two credits, the withdrawals, the account
                writes -- with the accounts in a std::unordered_map keyed by row and balances in five 64-bit limbs, on one core,
                compiled by this tool (g++ -O2), wall time
Every output is compared with tests/settle_ref.py before anything is timed.  Needs a GPU.  One size a process, under a time limit:
  timeout -k 10 300 python tools/bench_settle.py --sizes 200 && timeout -k 10 300 python tools/bench_settle.py --sizes 2000 && \\
  timeout -k 10 300 python tools/bench_settle.py --sizes 10000
"""
import argparse
import ctypes as C
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
#include <unordered_map>
#include <vector>
typedef unsigned __int128 u128;
struct Acc { uint64_t b[5]; uint64_t nonce; };  // the balance: five limbs, two's complement
static void be(const uint8_t* p, uint64_t w[5]) { for (int q = 0; q < 4; ++q) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v = v << 8 | p[8 * (3 - q) + k]; w[q] = v; } w[4] = 0; }
static void add(uint64_t a[5], const uint64_t c[5]) { u128 carry = 0; for (int q = 0; q < 5; ++q) { carry += (u128)a[q] + c[q]; a[q] = (uint64_t)carry; carry >>= 64; } }
static void sub(uint64_t a[5], const uint64_t c[5]) { uint64_t borrow = 0; for (int q = 0; q < 5; ++q) { u128 t = (u128)a[q] - c[q] - borrow; a[q] = (uint64_t)t; borrow = (uint64_t)(t >> 64) & 1; } }
static void mul(uint64_t g, const uint64_t p[5], uint64_t out[5]) { u128 carry = 0; for (int q = 0; q < 5; ++q) { carry += (u128)g * p[q]; out[q] = (uint64_t)carry; carry >>= 64; } }
static bool less(const uint64_t a[5], const uint64_t c[5]) { if (a[4] >> 63) return true; for (int q = 4; q >= 0; --q) if (a[q] != c[q]) return a[q] < c[q]; return false; }
static void store(uint8_t* p, const uint64_t w[5]) { for (int q = 0; q < 4; ++q) for (int k = 0; k < 8; ++k) p[8 * (3 - q) + k] = (uint8_t)(w[q] >> (56 - 8 * k)); }
// -> nanoseconds of one pass over a block of plain rows
extern "C" uint64_t settle_pass(uint32_t n, const uint64_t* gas_limit, const uint64_t* gas, const uint8_t* value, const uint8_t* price, const uint8_t* cost,
                                const uint32_t* sender_row, const uint32_t* to_row, uint64_t block_gas_limit, const uint8_t* base_fee, uint32_t coinbase,
                                uint32_t na, const uint64_t* nonces, const uint8_t* balances, uint32_t n_wd, const uint32_t* wd_row, const uint64_t* wd_gwei,
                                uint32_t* flags, uint64_t* cum_out, uint8_t* before, uint8_t* op, uint64_t* nonces_after, uint8_t* balances_after) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<uint32_t, Acc> state;
    state.reserve(2 * (size_t)na);
    for (uint32_t j = 0; j < na; ++j) { Acc a; be(balances + 32ull * j, a.b); a.nonce = nonces[j]; state.emplace(j, a); }
    std::vector<uint8_t> touched(na, 0);
    uint64_t fee[5], cum = 0;
    be(base_fee, fee);
    for (uint32_t i = 0; i < n; ++i) {
        Acc& s = state.find(sender_row[i])->second;
        uint64_t v[5], p[5], c[5], charge[5], tip[5];
        be(value + 32ull * i, v), be(price + 32ull * i, p), be(cost + 32ull * i, c);
        uint32_t f = gas_limit[i] > block_gas_limit - cum ? 2u : 0u;
        if (less(s.b, c)) f |= 4u;
        store(before + 32ull * i, s.b);
        mul(gas[i], p, charge);
        add(charge, v);
        sub(s.b, charge);
        s.nonce += 1;
        add(state.find(to_row[i])->second.b, v);
        sub(p, fee);
        mul(gas[i], p, tip);
        add(state.find(coinbase)->second.b, tip);
        touched[sender_row[i]] = touched[to_row[i]] = touched[coinbase] = 1;
        cum += gas[i];
        flags[i] = f, cum_out[i] = cum;
    }
    for (uint32_t j = 0; j < n_wd; ++j) {
        const uint64_t giga[5] = {1000000000ull, 0, 0, 0, 0};
        uint64_t w[5];
        mul(wd_gwei[j], giga, w);
        add(state.find(wd_row[j])->second.b, w);
        touched[wd_row[j]] = 1;
    }
    for (uint32_t j = 0; j < na; ++j) {
        const Acc& a = state.find(j)->second;
        const bool empty = a.nonce == 0 && !(a.b[0] | a.b[1] | a.b[2] | a.b[3]);
        op[j] = !touched[j] ? 0 : empty ? 2 : 1;
        nonces_after[j] = a.nonce;
        store(balances_after + 32ull * j, a.b);
    }
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
"""


def baseline_lib(tmp):
    src, so = os.path.join(tmp, "settle.cpp"), os.path.join(tmp, "settle.so")
    with open(src, "w") as f:
        f.write(BASELINE)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.settle_pass.restype = C.c_uint64
    lib.settle_pass.argtypes = [C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
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
    from tests import settle_ref as R

    ctx = default_context()
    lib = ctx._lib
    rng = np.random.default_rng(2029)
    names = [name for name, _, _, _ in R.OUTPUTS]
    base_fee, bgl = 7, 10**12

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    with tempfile.TemporaryDirectory() as tmp:
        cpu = baseline_lib(tmp)
        for n in [int(x) for x in args.sizes.split(",") if x]:
            na = TABLE.get(n, 2 * n + 100)
            accounts = [R.account(int(rng.integers(0, 10**6)), ((1 << 61) + int(rng.integers(1, 1 << 61))) << 40) for j in range(na)]
            coinbase = na - 1
            wd = [(int(k), int(rng.integers(1, 1 << 40))) for k in rng.integers(0, na, 16)]
            for dist in ("distinct", "skewed", "single"):
                who = {"distinct": np.arange(n) % na, "skewed": (na * rng.random(n) ** 4).astype(int), "single": np.full(n, na // 3)}[dist]
                txs = [R.tx(int(j), int(rng.integers(0, na)), value=int(rng.integers(1, 1 << 62)) << int(rng.integers(0, 30)), price=8 + int(rng.integers(0, 10**9)))
                       for j in who.tolist()]
                ins = R.inputs(base_fee, txs, accounts, wd)
                exp, scalars = R.expected(R.PRAGUE, bgl, base_fee, coinbase, txs, accounts, wd)
                assert scalars["first_bad"] == n and scalars["n_not_plain"] == 0
                counts = {"n": n, "n_accounts": na, "n_wd": len(wd)}
                width = {name: np.dtype(dt).itemsize * k * counts[rows] for name, dt, k, rows in R.OUTPUTS}

                def call(fn, ptr_in, ptr_out):
                    arg = L.PhantSettleIn(C.sizeof(L.PhantSettleIn), R.PRAGUE, n, na, len(wd), coinbase, (C.c_uint32 * 2)(0, 0), bgl, *[ptr_in(k) for k in L.SETTLE_INPUTS])
                    out = L.PhantSettleOut(C.sizeof(L.PhantSettleOut), 0, 0, 0, 0, 0, 0, *[ptr_out(k) for k in names])
                    ctx.check(fn(ctx.handle, C.byref(arg), C.byref(out)))
                    assert {k: int(getattr(out, k)) for k in R.SCALARS} == scalars

                # ---- host form: the answers first, then the clock
                flat = {k: np.ascontiguousarray(a).reshape(-1).view(np.uint8) for k, a in ins.items()}
                bufs = {k: np.zeros(max(width[k], 8), np.uint8) for k in names}
                host = lambda: call(lib.phant_block_settle, lambda k: flat[k].ctypes.data, lambda k: bufs[k].ctypes.data)  # noqa: E731
                host()
                for k in names:
                    assert bufs[k][:width[k]].tobytes() == exp[k], k + " differs from the definition (host form)"
                ms = []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    host()
                    ms.append((time.perf_counter() - t0) * 1e3)
                res = {"n": n, "n_accounts": na, "n_wd": len(wd), "senders": dist, "distinct_senders": len(set(who.tolist())), "host_ms": stats(ms[args.warmup:])}

                # ---- device form
                d_in = {k: torch.from_numpy(a.copy()).cuda() for k, a in flat.items()}
                d_out = {k: torch.zeros(max(width[k], 8), dtype=torch.uint8, device="cuda") for k in names}
                dev = lambda: call(lib.phant_block_settle_dev, lambda k: d_in[k].data_ptr(), lambda k: d_out[k].data_ptr())  # noqa: E731
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
                gas = np.maximum(ins["intrinsic_gas"], ins["floor_gas"])
                wd_row, wd_gwei = ins["wd_row"], ins["wd_amount_gwei"]
                o = {"flags": np.zeros(n, np.uint32), "cum": np.zeros(n, np.uint64), "before": np.zeros((n, 32), np.uint8), "op": np.zeros(na, np.uint8),
                     "nonces": np.zeros(na, np.uint64), "balances": np.zeros((na, 32), np.uint8)}
                p = lambda a: a.ctypes.data  # noqa: E731
                one = lambda: cpu.settle_pass(n, p(ins["gas_limit"]), p(gas), p(ins["value"]), p(ins["effective_gas_price"]), p(ins["upfront_cost"]),  # noqa: E731
                                              p(ins["sender_row"]), p(ins["to_row"]), bgl, p(ins["base_fee"]), coinbase, na, p(ins["nonces"]), p(ins["balances"]),
                                              len(wd), p(wd_row), p(wd_gwei), p(o["flags"]), p(o["cum"]), p(o["before"]), p(o["op"]), p(o["nonces"]), p(o["balances"]))
                ns = [one() for _ in range(args.warmup + args.reps)][args.warmup:]
                assert o["flags"].tobytes() == exp["settle_flags"] and o["cum"].tobytes() == exp["cumulative_gas_used"] and o["before"].tobytes() == exp["balance_before"]
                assert o["op"].tobytes() == exp["account_op"] and o["nonces"].tobytes() == exp["nonces_after"] and o["balances"].tobytes() == exp["balances_after"], \
                    "the host core's accounts differ from the definition"
                res["cpu_baseline"] = dict(stats([x / 1e6 for x in ns]), cores=1, kind="std::unordered_map loop", unit="ms")
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
