"""The host splitter of phant_bodies_decode_rlp -- body_split of phant_amd/csrc/host_rlp.cpp -- compiled as a stand-alone program under
AddressSanitizer + UBSan (tests/native/bodies_decode_main.cpp) and held against the verdicts of tests/bodies_ref.py: the status, the
counts and every value byte of every truncation, every single-byte replacement and a length field of 2^64 - 1 at every position of a
few seed blocks and bodies.  Then the C entry point itself, through the built library: its two-step sizing and what it leaves
untouched.  No GPU is involved, and nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bodies_ref as B
from tests import secp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (0x00, 0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8, 0xFF)


def _variants(x):
    out = [x] + [x[:k] for k in range(len(x))] + [x + b"\x00"]
    for k in range(len(x)):
        out += [x[:k] + bytes([b]) + x[k + 1:] for b in VALUES if b != x[k]]
        out += [x[:k] + bytes([head]) + b"\xff" * 8 + x[k:] for head in (0xBF, 0xFF)]  # a length of 2^64 - 1 from here on
    return out


def _seeds():
    legacy = S.rlp_list([S.rlp_int(3), S.rlp_int(10**9), S.rlp_bytes(b"\x11" * 20)])
    typed = b"\x02" + S.rlp_list([S.rlp_int(1), S.rlp_bytes(b"\x77" * 60)])
    w = [B.withdrawal(k, amount=10**9 + k) for k in range(3)]
    header = S.rlp_list([S.rlp_bytes(b"p" * 32), S.rlp_int(7)])
    return [(False, B.make_block([legacy, typed, b"\x01" + S.rlp_list([])], w, header=header)), (False, B.make_block([typed], None, header=header)),
            (True, S.rlp_list([S.rlp_list([legacy, S.rlp_bytes(typed)]), b"\xc0", S.rlp_list(w[:1])])), (True, S.rlp_list([b"\xc0", b"\xc0"]))]


def test_the_splitter_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "bodies_decode"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "bodies_decode_main.cpp"), os.path.join(ROOT, "phant_amd", "csrc", "host_rlp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    records, counts = [], [0] * 5
    for bodies_only, seed in _seeds():
        assert B.split(seed, bodies_only)[0] == B.SPLIT_OK
        for v in _variants(seed) + [seed[1:], b""]:
            for only in (bodies_only, not bodies_only) if v is seed else (bodies_only,):
                st, txs, wds = B.split(v, only)
                counts[st] += 1
                t, w = b"".join(txs), b"".join(wds)
                records.append(struct.pack("<IIIIIII", len(v), int(only), st, len(txs), len(wds), len(t), len(w)) + v + t + w)
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:entries|split|BAD_RLP|BAD_TX|UNCLES|BAD_WITHDRAWAL)", r.stdout)]
    assert got == [len(records)] + counts, r.stdout
    # (most damage lands inside a header, a transaction or a withdrawal, which the splitter does not look into; every verdict occurs)
    assert counts[0] > 1000 and counts[1] > 1000 and counts[2] >= 10 and counts[3] >= 2 and counts[4] >= 5, counts


def test_two_step_sizing_through_the_library():
    """the totals are always written; nothing else is when a capacity is short; a refused block contributes no rows"""
    from phant_amd import build as Bd
    Bd.build()
    from phant_amd import _lib as L
    lib = L.lib()
    seeds = [s for only, s in _seeds() if not only]
    raws = [seeds[0], seeds[0][:-1], seeds[1], seeds[0]]
    status_ref, txs, wds = B.split_all(raws)
    assert status_ref == [0, B.SPLIT_BAD_RLP, 0, 0]
    blob = np.frombuffer(b"".join(raws), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in raws]).astype(np.uint64)
    n, n_wd = sum(map(len, txs)), sum(map(len, wds))
    tx_bytes, wd_bytes = sum(len(t) for b in txs for t in b), sum(len(w) for b in wds for w in b)

    def call(tx_cap, wd_cap, txb_cap, wdb_cap, null=()):
        ee = lambda count, dtype: np.full(count * np.dtype(dtype).itemsize, 0xEE, np.uint8).view(dtype)  # noqa: E731
        a = {"txs": ee(tx_bytes + 8, np.uint8), "tx_off": ee(n + 2, np.uint64), "block_first": ee(6, np.uint32),
             "withdrawals": ee(wd_bytes + 8, np.uint8), "wd_off": ee(n_wd + 2, np.uint64), "wd_first": ee(6, np.uint32)}
        status = np.full(5, 0xEE, np.uint8)
        arg = L.PhantBodiesSplit(C.sizeof(L.PhantBodiesSplit), 0, tx_cap, wd_cap, txb_cap, wdb_cap, *[None if k in null else a[k].ctypes.data for k in L.BODIES_SPLIT_ARRAYS],
                                 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE, 0xEEEEEEEEEEEEEEEE)
        rc = lib.phant_bodies_decode_rlp(blob.ctypes.data, off.ctypes.data, len(raws), 0, C.byref(arg), status.ctypes.data)
        return rc, a, status, (arg.n, arg.n_wd, arg.tx_bytes, arg.wd_bytes)

    untouched = lambda a, status: all((v.view(np.uint8) == 0xEE).all() for v in a.values()) and (status == 0xEE).all()  # noqa: E731
    for caps, null in (((0, 0, 0, 0), L.BODIES_SPLIT_ARRAYS), ((n - 1, n_wd, tx_bytes, wd_bytes), ()), ((n, n_wd - 1, tx_bytes, wd_bytes), ()),
                       ((n, n_wd, tx_bytes - 1, wd_bytes), ()), ((n, n_wd, tx_bytes, wd_bytes - 1), ()), ((n, n_wd, tx_bytes, wd_bytes), ("wd_first",))):
        rc, a, status, totals = call(*caps, null=null)
        assert rc == L.OK and totals == (n, n_wd, tx_bytes, wd_bytes) and untouched(a, status), (caps, null)
    rc, a, status, totals = call(n, n_wd, tx_bytes, wd_bytes)
    assert rc == L.OK and totals == (n, n_wd, tx_bytes, wd_bytes) and status.tolist() == status_ref + [0xEE]
    assert a["txs"][:tx_bytes].tobytes() == b"".join(t for b in txs for t in b) and (a["txs"][tx_bytes:] == 0xEE).all()
    assert a["withdrawals"][:wd_bytes].tobytes() == b"".join(w for b in wds for w in b) and (a["withdrawals"][wd_bytes:] == 0xEE).all()
    assert a["tx_off"][:n + 1].tolist() == np.cumsum([0] + [len(t) for b in txs for t in b]).tolist() and a["tx_off"][n + 1] == 0xEEEEEEEEEEEEEEEE
    assert a["block_first"][:5].tolist() == np.cumsum([0] + [len(b) for b in txs]).tolist() == [0, 3, 3, 4, 7] and a["block_first"][5] == 0xEEEEEEEE
    assert a["wd_first"][:5].tolist() == [0, 3, 3, 3, 6] and a["wd_off"][n_wd] == wd_bytes
    # refusals
    arg = L.PhantBodiesSplit(C.sizeof(L.PhantBodiesSplit) + 8)
    assert lib.phant_bodies_decode_rlp(blob.ctypes.data, off.ctypes.data, 4, 0, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    arg = L.PhantBodiesSplit(C.sizeof(L.PhantBodiesSplit))
    assert lib.phant_bodies_decode_rlp(blob.ctypes.data, off.ctypes.data, 4, 2, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    assert lib.phant_bodies_decode_rlp(blob.ctypes.data, off[::-1].copy().ctypes.data, 4, 0, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    assert lib.phant_bodies_decode_rlp(blob.ctypes.data, off.ctypes.data, 4, 0, C.byref(arg), None) == L.E_INVALID_ARG
    assert lib.phant_bodies_decode_rlp(None, None, 0, 0, C.byref(arg), None) == L.OK and (arg.n, arg.tx_bytes) == (0, 0)
