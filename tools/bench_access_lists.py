#!/usr/bin/env python3
"""A block's access lists (phant_block_access_lists) beside one host core doing the same decode and join: a JSON line per shape.

Three shapes -- `ordinary` (200 transactions of 2 tuples x 3 keys against a witness of 500 accounts / 2 000 slots), `heavy` (2 000
transactions of 8 x 16 against 5 000 / 20 000) and `one` (one transaction carrying 4 000 keys under one address, 500 / 2 000) --,
medians and interquartile spreads over --reps calls:
  dev_ms        phant_timing's device region of phant_block_access_lists_dev, every output
  host_ms       host-form wall time, every output
  cpu_baseline  the same walk of every span, the same joins and first occurrences as a plain C++ std::unordered_map loop on one core,
                compiled by this tool (g++ -O2), wall time
Every output of all three is compared with tests/access_ref.py before anything is timed.  Needs a GPU.  One shape a process, under a
time limit:
  timeout -k 10 300 python tools/bench_access_lists.py --shapes ordinary && timeout -k 10 300 python tools/bench_access_lists.py --shapes heavy && \\
  timeout -k 10 300 python tools/bench_access_lists.py --shapes one
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
# shape: (transactions, tuples each, keys per tuple, witness accounts, witness slots)
SHAPES = {"ordinary": (200, 2, 3, 500, 2000), "heavy": (2000, 8, 16, 5000, 20000), "one": (1, 1, 4000, 500, 2000)}

BASELINE = r"""
#include <chrono>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>
template <int N> struct Key { uint8_t b[N]; bool operator==(const Key& o) const { return !std::memcmp(b, o.b, N); } };
template <int N> struct KeyHash { size_t operator()(const Key<N>& k) const { uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int q = 0; q + 4 <= N; q += 4) { uint32_t w; std::memcpy(&w, k.b + q, 4); h = (h ^ w) * 0xC2B2AE3D27D4EB4Full; h ^= h >> 29; } return (size_t)h; } };
// one canonical RLP item at p[pos, end) -> its payload; false: cut short or not canonical
static bool item(const uint8_t* p, uint32_t pos, uint32_t end, uint32_t& pay, uint32_t& pend, bool& list) {
    if (pos >= end) return false;
    const uint32_t c = p[pos];
    if (c < 0x80) { pay = pos, pend = pos + 1, list = false; return true; }
    if (c <= 0xb7 || (c >= 0xc0 && c <= 0xf7)) {
        list = c >= 0xc0;
        const uint32_t len = c - (list ? 0xc0 : 0x80);
        if (1 + len > end - pos || (!list && len == 1 && p[pos + 1] < 0x80)) return false;
        pay = pos + 1, pend = pay + len;
        return true;
    }
    list = c >= 0xf8;
    const uint32_t ll = c - (list ? 0xf7 : 0xb7);
    if (1 + ll > end - pos || p[pos + 1] == 0) return false;
    uint64_t len = 0;
    for (uint32_t i = 0; i < ll; ++i) len = len << 8 | p[pos + 1 + i];
    if (len <= 55 || len > end - pos - 1 - ll) return false;
    pay = pos + 1 + ll, pend = pay + (uint32_t)len;
    return true;
}
// -> nanoseconds of one pass over the block: the witness's two maps, every span walked, every entry joined, the first occurrences
extern "C" uint64_t access_pass(uint32_t n, const uint8_t* txs, const uint64_t* al_off, const uint32_t* al_len, uint32_t na, const uint8_t* addresses,
                                const uint32_t* slot_first, const uint8_t* slots, uint32_t* totals /* 5 */, uint32_t* tuple_first, uint32_t* al_flags,
                                uint32_t* warm_addresses, uint32_t* warm_keys, uint8_t* address, uint32_t* key_first, uint32_t* account_row,
                                uint32_t* tuple_same, uint8_t* key, uint32_t* slot_row, uint32_t* key_same) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t NONE = 0xffffffffu;
    std::unordered_map<Key<20>, uint32_t, KeyHash<20>> row;
    std::unordered_map<Key<36>, uint32_t, KeyHash<36>> slot;
    row.reserve(2 * (size_t)na);
    slot.reserve(2 * (size_t)(na ? slot_first[na] : 0));
    for (uint32_t j = 0; j < na; ++j) {
        Key<20> k; std::memcpy(k.b, addresses + 20ull * j, 20);
        row.emplace(k, j);
        for (uint32_t s = slot_first[j]; s < slot_first[j + 1]; ++s) { Key<36> q; std::memcpy(q.b, &j, 4); std::memcpy(q.b + 4, slots + 32ull * s, 32); slot.emplace(q, s); }
    }
    uint32_t e = 0, k = 0, miss_a = 0, miss_s = 0, first_bad = n;
    std::unordered_map<Key<20>, uint32_t, KeyHash<20>> seen_a;
    std::unordered_map<Key<36>, uint32_t, KeyHash<36>> seen_k;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* const p = txs + al_off[i];
        const uint32_t len = al_len[i], e0 = e, k0 = k;
        uint32_t flags = 0, wa = 0, wk = 0, ma = 0, ms = 0;
        bool ok = true;
        seen_a.clear(), seen_k.clear();
        tuple_first[i] = e;
        for (uint32_t pos = 0; ok && pos < len;) {
            uint32_t tp, te, ip, ie, kp, ke;
            bool list;
            ok = item(p, pos, len, tp, te, list) && list && item(p, tp, te, ip, ie, list) && !list && ie - ip == 20 && item(p, ie, te, kp, ke, list) && list && ke == te;
            if (!ok) break;
            Key<20> a; std::memcpy(a.b, p + ip, 20);
            const auto r = row.find(a);
            const uint32_t arow = r == row.end() ? NONE : r->second, same = seen_a.emplace(a, e).first->second;
            std::memcpy(address + 20ull * e, a.b, 20);
            account_row[e] = arow, tuple_same[e] = same, key_first[e] = k;
            if (same == e) ++wa, ma += arow == NONE; else flags |= 2u;
            while (kp < ke) {
                ok = item(p, kp, ke, ip, ie, list) && !list && ie - ip == 32;
                if (!ok) break;
                Key<36> q; std::memcpy(q.b, &same, 4); std::memcpy(q.b + 4, p + ip, 32);
                const uint32_t ksame = seen_k.emplace(q, k).first->second;
                uint32_t srow = NONE;
                if (arow != NONE) { std::memcpy(q.b, &arow, 4); const auto s = slot.find(q); if (s != slot.end()) srow = s->second; }
                std::memcpy(key + 32ull * k, p + ip, 32);
                slot_row[k] = srow, key_same[k] = ksame;
                if (ksame == k) ++wk, ms += srow == NONE; else flags |= 2u;
                ++k, kp = ie;
            }
            ++e, pos = te;
        }
        if (!ok) { e = e0, k = k0, flags = 1u, wa = wk = ma = ms = 0; if (first_bad == n) first_bad = i; }
        al_flags[i] = flags, warm_addresses[i] = wa, warm_keys[i] = wk, miss_a += ma, miss_s += ms;
    }
    tuple_first[n] = e, key_first[e] = k;
    totals[0] = e, totals[1] = k, totals[2] = miss_a, totals[3] = miss_s, totals[4] = first_bad;
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}
"""


def baseline_lib(tmp):
    src, so = os.path.join(tmp, "access.cpp"), os.path.join(tmp, "access.so")
    with open(src, "w") as f:
        f.write(BASELINE)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.access_pass.restype = C.c_uint64
    lib.access_pass.argtypes = [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 15
    return lib


def make_block(shape, rng):
    """-> (spans, the witness's tables): four addresses in five are the witness's, and two keys in three of those are slots of theirs"""
    from tests import access_ref as R
    n, tuples, keys, na, ns = SHAPES[shape]
    h = lambda tag, k, width: hashlib.sha256(tag + int(k).to_bytes(8, "big")).digest()[:width]  # noqa: E731
    first = np.concatenate([[0], np.sort(rng.integers(0, ns + 1, na - 1)), [ns]]).astype(int).tolist()
    tables = dict(addresses=[h(b"bench address", j, 20) for j in range(na)], slot_first=first, slots=[h(b"bench slot", s, 32) for s in range(ns)])
    spans = []
    for i in range(n):
        entries = []
        for t in range(tuples):
            j = int(rng.integers(0, na))
            mine = range(first[j], first[j + 1])
            a = tables["addresses"][j] if rng.random() < 0.8 else h(b"bench stranger", 10 * i + t, 20)
            ks = [tables["slots"][int(rng.integers(mine.start, mine.stop))] if len(mine) and rng.random() < 0.67 else h(b"bench key", int(rng.integers(0, 1 << 40)), 32)
                  for _ in range(keys)]
            entries.append((a, ks))
        spans.append(R.encode(entries))
    return spans, tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ordinary,heavy,one")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from tests import access_ref as R

    ctx = default_context()
    lib = ctx._lib
    rng = np.random.default_rng(2930)
    names = [name for name, _, _, _, _ in R.OUTPUTS]
    inputs = ("txs", "al_off", "al_len", "addresses", "slot_first", "slots")

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    with tempfile.TemporaryDirectory() as tmp:
        cpu = baseline_lib(tmp)
        for shape in [s for s in args.shapes.split(",") if s]:
            spans, tables = make_block(shape, rng)
            ins = R.inputs(spans, **tables)
            exp, totals = R.expected(spans, **tables)
            n, na, ns = len(spans), len(tables["addresses"]), len(tables["slots"])
            rows = {"n": n, "n_tuples": totals["n_tuples"], "n_keys": totals["n_keys"]}
            width = {name: np.dtype(dt).itemsize * k * (rows[r] + extra) for name, dt, k, r, extra in R.OUTPUTS}

            def call(fn, ptr_in, ptr_out):
                arg = L.PhantAccessIn(C.sizeof(L.PhantAccessIn), n, na, ns, ptr_in("txs"), int(ins["txs"].size), *[ptr_in(k) for k in inputs[1:]])
                out = L.PhantAccessOut(C.sizeof(L.PhantAccessOut), 0, 0, 0, 0, 0, rows["n_tuples"], rows["n_keys"], *[ptr_out(k) for k in names])
                ctx.check(fn(ctx.handle, C.byref(arg), C.byref(out)))
                assert {t: int(getattr(out, t)) for t in R.TOTALS} == totals

            # ---- host form: the answers first, then the clock
            flat = {k: np.ascontiguousarray(ins[k]).reshape(-1).view(np.uint8) for k in inputs}
            bufs = {k: np.zeros(max(width[k], 8), np.uint8) for k in names}
            host = lambda: call(lib.phant_block_access_lists, lambda k: flat[k].ctypes.data, lambda k: bufs[k].ctypes.data)  # noqa: E731
            host()
            for k in names:
                assert bufs[k][:width[k]].tobytes() == exp[k], k + " differs from the definition (host form)"
            ms = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                host()
                ms.append((time.perf_counter() - t0) * 1e3)
            res = {"shape": shape, "n": n, "n_tuples": totals["n_tuples"], "n_keys": totals["n_keys"], "n_accounts": na, "n_slots": ns,
                   "span_bytes": int(ins["al_len"].sum()), "host_ms": stats(ms[args.warmup:])}

            # ---- device form
            d_in = {k: torch.from_numpy(a.copy()).cuda() for k, a in flat.items()}
            d_out = {k: torch.zeros(max(width[k], 8), dtype=torch.uint8, device="cuda") for k in names}
            dev = lambda: call(lib.phant_block_access_lists_dev, lambda k: d_in[k].data_ptr(), lambda k: d_out[k].data_ptr())  # noqa: E731
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
            o = {k: np.zeros(max(width[k], 8), np.uint8) for k in names}
            tot = np.zeros(5, np.uint32)
            p = lambda a: a.ctypes.data  # noqa: E731
            one = lambda: cpu.access_pass(n, p(ins["txs"]), p(ins["al_off"]), p(ins["al_len"]), na, p(ins["addresses"]), p(ins["slot_first"]), p(ins["slots"]),  # noqa: E731
                                          p(tot), *[p(o[k]) for k in names])
            ns_ = [one() for _ in range(args.warmup + args.reps)][args.warmup:]
            assert tot.tolist() == [totals[t] for t in R.TOTALS], "the host core's totals differ from the definition"
            for k in names:
                assert o[k][:width[k]].tobytes() == exp[k], k + ": the host core differs from the definition"
            res["cpu_baseline"] = dict(stats([x / 1e6 for x in ns_]), cores=1, kind="std::unordered_map loop", unit="ms")
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
