#!/usr/bin/env python3
"""Block headers, fields in and hashes + flags out: one JSON line.

Chains: one valid segment of n headers of 17 fields (n = 2, 256, 8 192, 100 000 by default), arrays packed beforehand.  Per size,
medians over --reps calls after --warmup calls:
  host_ms        phant_header_chain, wall time (the call synchronises): hashes, flags and first_bad
  host_enc_ms    the same with the encodings and their offsets fetched as well
  dev_ms         phant_header_chain_dev on arrays that live in device memory, the device region of the call (events around it:
                 it includes the call's two synchronisations)
  cpu_keccak_ms  ONE CPU core hashing the same headers: the oracle's keccak256_batch over the PRE-ENCODED headers.  This leaves
                 out the encoding and all thirteen checks, which favours the CPU.
Every output of both forms is compared with tests/headers_ref.py before anything is timed.
Needs a GPU.  python tools/bench_headers.py [--sizes 2,256,8192,100000] [--reps 20] [--warmup 3]
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


def make_chain(H, rng, n):
    """a valid segment: every header passes every rule against the one before it"""
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    out, p = [], None
    for i in range(n):
        h = {f: None for f in H.FIELDS}
        h.update(parent_hash=rb(32) if p is None else H.hash(p), uncle_hash=H.EMPTY_UNCLE_HASH, fee_recipient=rb(20), state_root=rb(32),
                 transactions_root=rb(32), receipts_root=rb(32), logs_bloom=rb(256), difficulty=0, block_number=17_000_000 + i,
                 gas_limit=30_000_000, gas_used=int(rng.integers(0, 30_000_001)), timestamp=1_700_000_000 + 12 * i,
                 extra_data=rb(int(rng.integers(0, 33))), prev_randao=rb(32), nonce=bytes(8),
                 base_fee_per_gas=10 ** 10 if p is None else H.expected_base_fee(p), withdrawals_root=rb(32))
        out.append(h)
        p = h
    return out


def median(values):
    return round(float(np.median(values)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,256,8192,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import phant_amd  # noqa: F401
    from oracle import oracle as O
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from phant_amd.types import block as B
    from tests import headers_ref as H

    O.build()
    ctx = default_context()
    lib = ctx._lib
    rng = np.random.default_rng(2028)
    out = {"tool": "bench_headers", "reps": args.reps, "warmup": args.warmup, "sizes": {}}
    for n in (int(x) for x in args.sizes.split(",")):
        headers = make_chain(H, rng, n)
        want_hashes, want_flags, want_first = H.validate_chain(headers)
        want_enc = [H.encode(h) for h in headers]
        total = sum(map(len, want_enc))
        want_off = np.cumsum([0] + [len(e) for e in want_enc]).astype(np.uint64)
        assert not any(want_flags) and want_first == n
        a = B.pack_headers([B.BlockHeader(**h) for h in headers])

        # ---- host form
        hashes, flags = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint32)
        enc, enc_off = np.zeros(total, np.uint8), np.zeros(n + 1, np.uint64)
        arg = B._struct(a, n)

        def host_call(with_enc):
            o = L.PhantHeadersOut(C.sizeof(L.PhantHeadersOut), 0, total, hashes.ctypes.data, flags.ctypes.data,
                                  enc.ctypes.data if with_enc else None, enc_off.ctypes.data if with_enc else None, 0)
            ctx.check(lib.phant_header_chain(ctx.handle, C.byref(arg), C.byref(o)))
            return o

        o = host_call(True)
        assert (o.first_bad, o.enc_len) == (n, total) and hashes.tobytes() == b"".join(want_hashes) and not flags.any(), "host form differs from the reference"
        assert enc.tobytes() == b"".join(want_enc) and np.array_equal(enc_off, want_off), "encodings differ from the reference"

        def wall(fn):
            ms = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                fn()
                if i >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            return median(ms)

        rec = {"headers": n, "field_bytes": int(sum(v.nbytes for v in a.values())), "encoded_bytes": total}
        rec["host_ms"] = wall(lambda: host_call(False))
        rec["host_enc_ms"] = wall(lambda: host_call(True))

        # ---- device form
        up = lambda v: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda()  # noqa: E731
        d = {k: up(v) for k, v in a.items()}
        d_hashes = torch.zeros((n, 32), dtype=torch.uint8).cuda()
        d_flags = torch.zeros(n, dtype=torch.int32).cuda()
        d_arg = L.PhantHeadersIn(C.sizeof(L.PhantHeadersIn), n, 0, 0, *[d[k].data_ptr() if k in d else None for k in L.HEADER_ARRAYS])
        ctx.timing(True)

        def dev_call():
            o = L.PhantHeadersOut(C.sizeof(L.PhantHeadersOut), 0, 0, d_hashes.data_ptr(), d_flags.data_ptr(), None, None, 0)
            ctx.check(lib.phant_header_chain_dev(ctx.handle, C.byref(d_arg), C.byref(o)))
            ctx.sync()
            return o, ctx.last_kernel_ms()

        o, _ = dev_call()
        assert (o.first_bad, o.enc_len) == (n, total) and d_hashes.cpu().numpy().tobytes() == b"".join(want_hashes) and not d_flags.any().item(), \
            "device form differs from the reference"
        rec["dev_ms"] = median([dev_call()[1] for _ in range(args.warmup + args.reps)][args.warmup:])
        ctx.timing(False)

        # ---- one CPU core: Keccak alone over the encodings
        blob = np.frombuffer(b"".join(want_enc), np.uint8).copy()
        assert O.keccak256_batch(blob, want_off).tobytes() == b"".join(want_hashes)
        rec["cpu_keccak_ms"] = wall(lambda: O.keccak256_batch(blob, want_off))
        out["sizes"][str(n)] = rec
        print(f"bench_headers: {n} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
