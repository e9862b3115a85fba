#!/usr/bin/env python3
"""A block's transactions before execution (phant_block_transactions) beside what a caller did before it existed: one JSON line.

For n = 200, 2 000, 10 000 reference-signed transactions in a mainnet-like mix (about 60 % EIP-1559 transfers of ~110 bytes, 35 % calls
with 200 - 700 bytes of calldata, 5 % with an access list; a tenth of them legacy), medians and interquartile spreads over --reps calls:
  dev_ms / dev_no_recovery_ms   phant_timing's device region of phant_block_transactions_dev, every output, with and without the
                                secp256k1 launch
  host_all_ms                   host-form wall time, every output
  host_core_ms                  host-form wall time with tx_hash, sender, sig_status and flags only: what the two old calls answer
  old_two_calls_ms              in the same process: phant_tx_senders + types.transaction.hashes, the caller's path before this call
--long adds one line: 200 transactions of which one carries 49 152 bytes of calldata (a Keccak message is sequential: the call lasts as
long as its longest transaction in one lane).
--fork london|cancun|prague measures phant_block_transactions_ex instead (another JSON line, see bench_fork below): cancun turns about
5 % of the mix into blob transactions (type 3, 1 - 6 versioned hashes), prague also about 2 % into set-code transactions (type 4, 1 - 3
signed authorizations); --one-auth (with prague) instead makes transaction 0 the only one of type 4, with a single authorization.
Every output is compared with the reference before anything is timed: all of them against tests/tx_ref.py for the first --check
transactions, senders (known from the signing keys), hashes and flags for all.
Needs a GPU.  One size a process, each under a time limit of its own:
  timeout -k 10 300 python tools/bench_transactions.py --sizes 200 && timeout -k 10 300 python tools/bench_transactions.py --sizes 2000 && \\
  timeout -k 10 600 python tools/bench_transactions.py --sizes 10000 && timeout -k 10 300 python tools/bench_transactions.py --sizes "" --long
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_senders import sign_with, signers  # noqa: E402


def mix(S, O, rng, who, n, long_at=None, fork=0, one_auth=False):
    """n signed transactions, chain id 1.  fork > 0: -> (the transactions, their TWINS: the block with every type-3 and type-4 entry
    replaced by a type-2 transaction of the same fields and calldata, which a call without a fork can decode)"""
    txs, twins = [], []
    for i in range(n):
        kind = rng.random()
        data = b"" if kind < 0.6 else bytes(b if j % 3 else 0 for j, b in enumerate(rng.bytes(int(rng.integers(200, 701)))))
        if i == long_at:
            data = bytes(b if j % 3 else 0 for j, b in enumerate(rng.bytes(49152)))
        al = S.rlp_list([S.rlp_list([S.rlp_bytes(rng.bytes(20)), S.rlp_list([S.rlp_bytes(rng.bytes(32)) for _ in range(int(rng.integers(0, 4)))])])
                         for _ in range(2)]) if kind >= 0.95 else b"\xc0"
        to, gas = S.rlp_bytes(rng.bytes(20)), S.rlp_int(21000 + 16 * len(data) + 20000)
        if i % 10 == 9:
            typ, fields = 0, [S.rlp_int(i), S.rlp_int(3 * 10**9), gas, to, S.rlp_int(10**15 + i), S.rlp_bytes(data)]
            pre = S.rlp_list(fields + [S.rlp_int(1), b"\x80", b"\x80"])
        else:
            typ, fields = 2, [S.rlp_int(1), S.rlp_int(i), S.rlp_int(10**9), S.rlp_int(3 * 10**9), gas, to, S.rlp_int(10**15 + i), S.rlp_bytes(data), al]
            pre = b"\x02" + S.rlp_list(fields)
        r, s, recid = sign_with(S, who[i], int.from_bytes(O.keccak256(pre), "big"))
        raw = S.rlp_list(fields + [S.rlp_int(recid + (37 if typ == 0 else 0)), S.rlp_int(r), S.rlp_int(s)])
        txs.append((b"\x02" if typ else b"") + raw)
        if not fork:
            continue
        twins.append(txs[-1])
        u = rng.random()
        new = 0 if typ == 0 else (4 if i == 0 else 0) if one_auth else 3 if u < 0.05 else 4 if u < 0.07 and fork >= 2 else 0
        if new == 3:
            extra = [S.rlp_int(10), S.rlp_list([S.rlp_bytes(b"\x01" + rng.bytes(31)) for _ in range(int(rng.integers(1, 7)))])]
        elif new == 4:
            tuples = []
            for k in range(1 if one_auth else int(rng.integers(1, 4))):
                address, nonce = rng.bytes(20), int(rng.integers(0, 1000))
                z = int.from_bytes(O.keccak256(b"\x05" + S.rlp_list([S.rlp_int(1), S.rlp_bytes(address), S.rlp_int(nonce)])), "big")
                ar, as_, ay = sign_with(S, who[(i + 1 + k) % n], z)
                tuples.append(S.rlp_list([S.rlp_int(1), S.rlp_bytes(address), S.rlp_int(nonce), S.rlp_int(ay), S.rlp_int(ar), S.rlp_int(as_)]))
            fields[4] = S.rlp_int(21000 + 16 * len(data) + 20000 + 25000 * len(tuples))
            extra = [S.rlp_list(tuples)]
        else:
            continue
        fields = fields + extra
        r, s, recid = sign_with(S, who[i], int.from_bytes(O.keccak256(bytes([new]) + S.rlp_list(fields)), "big"))
        txs[-1] = bytes([new]) + S.rlp_list(fields + [S.rlp_int(recid), S.rlp_int(r), S.rlp_int(s)])
    return (txs, twins) if fork else txs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,2000,10000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=1000)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--fork", choices=("london", "cancun", "prague"))
    ap.add_argument("--one-auth", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import _lib as L, signer
    from phant_amd.context import default_context
    from phant_amd.types import transaction as X
    from tests import secp_ref as S
    from tests import tx_ref as T

    O.build()
    rng = np.random.default_rng(2027)
    nmax = max(sizes + [200])
    who = signers(S, rng, nmax)
    keys = np.frombuffer(b"".join(S.pubkey_bytes(w[1]) for w in who), np.uint8)
    addrs = np.ascontiguousarray(O.keccak256_batch(keys, np.arange(nmax + 1, dtype=np.uint64) * 64)[:, 12:])
    ctx = default_context()
    lib = ctx._lib
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    BASE_FEE, GAS_LIMIT = 2 * 10**9, 30_000_000
    fee = np.frombuffer(BASE_FEE.to_bytes(32, "big"), np.uint8).copy()

    def stats(ms):
        q1, med, q3 = np.percentile(ms, [25, 50, 75])
        return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}

    def bench(txs, label):
        n = len(txs)
        blob, off = X.pack(txs)
        # ---- the answers, before anything is timed
        r = X.block_transactions(txs, 1, base_fee=BASE_FEE, block_gas_limit=GAS_LIMIT, ctx=ctx)
        k = min(n, args.check)
        exp, first_bad = T.expected(O, txs[:k], 1, BASE_FEE, GAS_LIMIT)
        for name, _, _ in T.OUTPUTS:
            assert getattr(r, name)[:k].tobytes() == exp[name], name + " differs from the reference"
        assert r.first_bad == n and not (r.flags & T.ERROR_BITS).any() and not r.sig_status.any()
        assert np.array_equal(r.sender, addrs[:n]) and np.array_equal(r.tx_hash, O.keccak256_batch(blob, off)), "senders / hashes differ"
        old_ad, old_st = signer.senders(txs, 1, ctx=ctx)
        assert np.array_equal(old_ad, r.sender) and np.array_equal(old_st, r.sig_status) and np.array_equal(X.hashes(txs, ctx=ctx), r.tx_hash)

        # ---- device form
        d_blob, d_off = torch.from_numpy(blob).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        d_out = {name: torch.zeros(max(1, n * k_ * np.dtype(dt).itemsize), dtype=torch.uint8, device="cuda") for name, dt, k_ in T.OUTPUTS}

        def dev_call(recover):
            flags = L.TXS_HAVE_GAS_LIMIT | (0 if recover else L.TXS_NO_RECOVERY)
            arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, d_blob.data_ptr(), d_off.data_ptr(), int(off[-1]), 1, fee.ctypes.data, GAS_LIMIT)
            out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[d_out[name].data_ptr() if recover or name not in ("sender", "sig_status") else None
                                                               for name, _, _ in T.OUTPUTS])
            ctx.check(lib.phant_block_transactions_dev(ctx.handle, C.byref(arg), C.byref(out)))
            assert out.first_bad == n

        def timed_dev(recover):
            ctx.check(lib.phant_timing(ctx.handle, 1))
            ms = []
            try:
                for i in range(args.warmup + args.reps):
                    dev_call(recover)
                    if i >= args.warmup:
                        ms.append(ctx.last_kernel_ms())
            finally:
                ctx.check(lib.phant_timing(ctx.handle, 0))
            return stats(ms)

        res = {"n": n, "bytes": int(off[-1]), "dev_ms": timed_dev(True), "dev_no_recovery_ms": timed_dev(False)}
        ctx.sync()
        assert np.array_equal(d_out["sender"].cpu().numpy().reshape(-1, 20), addrs[:n])

        # ---- host form: every output, and the outputs the two old calls give
        bufs = {name: np.zeros((n, k_) if k_ > 1 else n, dt) for name, dt, k_ in T.OUTPUTS}

        def host_call(names):
            arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, L.TXS_HAVE_GAS_LIMIT, 0, p(blob), p(off), int(off[-1]), 1, p(fee), GAS_LIMIT)
            out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[p(bufs[name]) if name in names else None for name, _, _ in T.OUTPUTS])
            ctx.check(lib.phant_block_transactions(ctx.handle, C.byref(arg), C.byref(out)))

        def wall(fn):
            ms = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return stats(ms[args.warmup:])

        o_ad, o_st, o_h = np.zeros((n, 20), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)

        def old():
            ctx.check(lib.phant_tx_senders(ctx.handle, p(blob), p(off), n, 1, p(o_ad), p(o_st)))
            ctx.check(lib.phant_keccak256_batch(ctx.handle, p(blob), p(off), n, p(o_h)))

        res["host_all_ms"] = wall(lambda: host_call([name for name, _, _ in T.OUTPUTS]))
        res["host_core_ms"] = wall(lambda: host_call(("tx_hash", "sender", "sig_status", "flags")))
        res["old_two_calls_ms"] = wall(old)
        assert np.array_equal(o_ad, bufs["sender"]) and np.array_equal(o_h, bufs["tx_hash"])
        return label, res

    def bench_fork(txs, twins, fork):
        """phant_block_transactions_ex at `fork` over txs, every output, beside phant_block_transactions over their twins:
          dev_ms / dev_no_recovery_ms / host_all_ms            the _ex call (device region; host-form wall time)
          twin_dev_ms / twin_dev_no_recovery_ms / twin_host_all_ms   the call without a fork over the twins"""
        from tests import tx_ref_forks as F
        n = len(txs)
        blob, off = X.pack(txs)
        r = X.block_transactions(txs, 1, base_fee=BASE_FEE, block_gas_limit=GAS_LIMIT, ctx=ctx, fork=fork, blob_base_fee=1)
        k = min(n, args.check)
        exp, _, n_auth_k, _ = F.expected(O, txs[:k], 1, fork, BASE_FEE, GAS_LIMIT, 1)
        for name, _, _ in T.OUTPUTS + tuple(x for x in F.TX_OUTPUTS if x[0] != "auth_first"):
            assert getattr(r, name)[:k].tobytes() == exp[name], name + " differs from the reference"
        assert r.auth_first[:k + 1].tobytes() == exp["auth_first"], "auth_first differs from the reference"
        for name, _, _ in F.AUTH_OUTPUTS:
            assert getattr(r, name)[:n_auth_k].tobytes() == exp[name], name + " differs from the reference"
        assert r.first_bad == n and not (r.flags & F.ERROR_BITS).any() and not r.sig_status.any() and not r.auth_status.any()
        assert np.array_equal(r.sender, addrs[:n]) and np.array_equal(r.tx_hash, O.keccak256_batch(blob, off)), "senders / hashes differ"
        cap = max(1, r.n_auth)
        per_tx = tuple(T.OUTPUTS) + tuple(F.TX_OUTPUTS)
        d_blob, d_off = torch.from_numpy(blob).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        d_out = {name: torch.zeros(max(8, (n + 1) * k_ * np.dtype(dt).itemsize), dtype=torch.uint8, device="cuda") for name, dt, k_ in per_tx}
        d_out.update({name: torch.zeros(cap * k_ * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda") for name, dt, k_ in F.AUTH_OUTPUTS})
        h_out = {name: np.zeros((n + 1) * k_, dt) for name, dt, k_ in per_tx}
        h_out.update({name: np.zeros(cap * k_, dt) for name, dt, k_ in F.AUTH_OUTPUTS})
        bfee = np.frombuffer((1).to_bytes(32, "big"), np.uint8).copy()
        skip = ("sender", "sig_status", "authority", "auth_status")

        def ex_call(dev, recover):
            ptr = (lambda name: d_out[name].data_ptr()) if dev else (lambda name: p(h_out[name]))
            want = lambda name: ptr(name) if recover or name not in skip else None  # noqa: E731
            b_, o_ = (d_blob.data_ptr(), d_off.data_ptr()) if dev else (p(blob), p(off))
            flags = L.TXS_HAVE_GAS_LIMIT | (0 if recover else L.TXS_NO_RECOVERY)
            base = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, b_, o_, int(off[-1]), 1, fee.ctypes.data, GAS_LIMIT)
            arg = L.PhantTxsExIn(C.sizeof(L.PhantTxsExIn), fork, base, bfee.ctypes.data, cap, 0)
            out = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0, 0, L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[want(name) for name, _, _ in T.OUTPUTS]),
                                  *[want(name) for name, _, _ in F.TX_OUTPUTS + F.AUTH_OUTPUTS])
            ctx.check((lib.phant_block_transactions_ex_dev if dev else lib.phant_block_transactions_ex)(ctx.handle, C.byref(arg), C.byref(out)))
            assert out.base.first_bad == n and out.n_auth == r.n_auth

        t_blob, t_off = X.pack(twins)
        dt_blob, dt_off = torch.from_numpy(t_blob).cuda(), torch.from_numpy(t_off.view(np.int64)).cuda()

        def twin_call(dev, recover):
            ptr = (lambda name: d_out[name].data_ptr()) if dev else (lambda name: p(h_out[name]))
            flags = L.TXS_HAVE_GAS_LIMIT | (0 if recover else L.TXS_NO_RECOVERY)
            b_, o_ = (dt_blob.data_ptr(), dt_off.data_ptr()) if dev else (p(t_blob), p(t_off))
            arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, b_, o_, int(t_off[-1]), 1, fee.ctypes.data, GAS_LIMIT)
            out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0, *[ptr(name) if recover or name not in skip else None for name, _, _ in T.OUTPUTS])
            ctx.check((lib.phant_block_transactions_dev if dev else lib.phant_block_transactions)(ctx.handle, C.byref(arg), C.byref(out)))
            assert out.first_bad == n

        def region(fn):
            ctx.check(lib.phant_timing(ctx.handle, 1))
            ms = []
            try:
                for i in range(args.warmup + args.reps):
                    fn()
                    if i >= args.warmup:
                        ms.append(ctx.last_kernel_ms())
            finally:
                ctx.check(lib.phant_timing(ctx.handle, 0))
            return stats(ms)

        def wall(fn):
            ms = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return stats(ms[args.warmup:])

        types = [t[0] if t[0] < 0x80 else 0 for t in txs]
        res = {"n": n, "bytes": int(off[-1]), "twin_bytes": int(t_off[-1]), "type3": types.count(3), "type4": types.count(4), "n_auth": r.n_auth,
               "blobs": r.blob_gas_used // 131072}
        res["dev_ms"], res["twin_dev_ms"] = region(lambda: ex_call(True, True)), region(lambda: twin_call(True, True))
        res["dev_no_recovery_ms"], res["twin_dev_no_recovery_ms"] = region(lambda: ex_call(True, False)), region(lambda: twin_call(True, False))
        ctx.sync()
        res["host_all_ms"], res["twin_host_all_ms"] = wall(lambda: ex_call(False, True)), wall(lambda: twin_call(False, True))
        return res

    if args.fork:
        fork = ("london", "cancun", "prague").index(args.fork)
        out = {"tool": "bench_transactions", "fork": args.fork, "one_auth": args.one_auth, "reps": args.reps, "sizes": {}}
        for n in sizes:
            txs, twins = mix(S, O, rng, who, n, fork=fork, one_auth=args.one_auth) if fork else (mix(S, O, rng, who, n),) * 2
            out["sizes"][str(n)] = bench_fork(txs, twins, fork)
        print(json.dumps(out))
        return

    out = {"tool": "bench_transactions", "reps": args.reps, "sizes": {}}
    for n in sizes:
        label, res = bench(mix(S, O, rng, who, n), str(n))
        out["sizes"][label] = res
    if args.long:
        out["long_200_one_49k"] = bench(mix(S, O, rng, who, 200, long_at=100), "long")[1]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
