"""The host splitter of phant_receipts_decode_rlp -- receipts_split of phant_amd/csrc/host_rlp.cpp -- compiled as a stand-alone program
under AddressSanitizer + UBSan (tests/native/receipts_decode_main.cpp) and held against the verdicts of tests/receipts_seg_ref.py: the
status, the count and every value byte of every truncation, every single-byte replacement and a length field of 2^64 - 1 at every
position of a few seed messages, in both wire forms.  Then the C entry point itself, through the built library: its two-step sizing and
what it leaves untouched.  No GPU is involved, and nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import receipts_ref as R
from tests import receipts_seg_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (0x00, 0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8, 0xFF)


def _variants(x):
    out = [x] + [x[:k] for k in range(len(x))] + [x + b"\x00"]
    for k in range(len(x)):
        out += [x[:k] + bytes([b]) + x[k + 1:] for b in VALUES if b != x[k]]
        out += [x[:k] + bytes([head]) + b"\xff" * 8 + x[k:] for head in (0xBF, 0xFF)]  # a length of 2^64 - 1 from here on
    return out


def _seeds():
    """(eth69, the per-block element of a message)"""
    log = (b"\x11" * 20, [b"\x22" * 32], b"\x01\x02")
    receipts = [(0, True, 21000, []), (2, False, 50000, [log]), (1, b"\x77" * 32, 2**40, [log, log])]
    return [(False, G.message_item([G.encode_consensus(r) for r in receipts])), (False, G.message_item([G.encode_consensus(receipts[1])])),
            (True, G.message_item([G.encode_eth69(r) for r in receipts], True)), (True, b"\xc0"), (False, R.rlp_list([R.rlp_list([b"\x01"]), R.rlp_str(b"\x7f")]))]


def test_the_splitter_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "receipts_decode"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "receipts_decode_main.cpp"), os.path.join(ROOT, "phant_amd", "csrc", "host_rlp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    records, counts = [], {G.SPLIT_OK: 0, G.SPLIT_BAD_RLP: 0, G.SPLIT_BAD_RECEIPT: 0}
    for eth69, seed in _seeds():
        assert G.split(seed, eth69)[0] == G.SPLIT_OK
        for v in _variants(seed) + [seed[1:], b""]:
            for form in (eth69, not eth69) if v is seed else (eth69,):
                st, values = G.split(v, form)
                counts[st] += 1
                joined = b"".join(values)
                records.append(struct.pack("<IIIII", len(v), int(form), st, len(values), len(joined)) + v + joined)
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:entries|split|BAD_RLP|BAD_RECEIPT)", r.stdout)]
    assert got == [len(records), counts[G.SPLIT_OK], counts[G.SPLIT_BAD_RLP], counts[G.SPLIT_BAD_RECEIPT]], r.stdout
    # (most damage lands inside a receipt, which the splitter does not look into; every verdict occurs)
    assert counts[G.SPLIT_OK] > 1000 and counts[G.SPLIT_BAD_RLP] > 1000 and counts[G.SPLIT_BAD_RECEIPT] >= 10, counts


def test_two_step_sizing_through_the_library():
    """the totals are always written; nothing else is when a capacity is short; a refused block contributes no rows"""
    from phant_amd import build as Bd
    Bd.build()
    from phant_amd import _lib as L
    lib = L.lib()
    seeds = [s for eth69, s in _seeds() if not eth69]
    raws = [seeds[0], seeds[0][:-1], seeds[1], b"\xc0", seeds[2]]
    status_ref, values = G.split_all(raws)
    assert status_ref == [0, G.SPLIT_BAD_RLP, 0, 0, 0]
    blob = np.frombuffer(b"".join(raws), np.uint8).copy()
    off = np.cumsum([0] + [len(r) for r in raws]).astype(np.uint64)
    n, nbytes = sum(map(len, values)), sum(len(v) for b in values for v in b)

    def call(rc_cap, bytes_cap, null=(), flags=0):
        ee = lambda count, dtype: np.full(count * np.dtype(dtype).itemsize, 0xEE, np.uint8).view(dtype)  # noqa: E731
        a = {"receipts": ee(nbytes + 8, np.uint8), "rc_off": ee(n + 2, np.uint64), "block_first": ee(len(raws) + 2, np.uint32)}
        status = np.full(len(raws) + 1, 0xEE, np.uint8)
        arg = L.PhantReceiptsSplit(C.sizeof(L.PhantReceiptsSplit), 0, rc_cap, 0xEEEEEEEE, bytes_cap, *[None if k in null else a[k].ctypes.data for k in a], 0xEEEEEEEEEEEEEEEE)
        rc = lib.phant_receipts_decode_rlp(blob.ctypes.data, off.ctypes.data, len(raws), flags, C.byref(arg), status.ctypes.data)
        return rc, a, status, (arg.n, arg.rc_bytes)

    untouched = lambda a, status: all((v.view(np.uint8) == 0xEE).all() for v in a.values()) and (status == 0xEE).all()  # noqa: E731
    for caps, null in (((0, 0), ("receipts", "rc_off", "block_first")), ((n - 1, nbytes), ()), ((n, nbytes - 1), ()), ((n, nbytes), ("block_first",)), ((n, nbytes), ("rc_off",))):
        rc, a, status, totals = call(*caps, null=null)
        assert rc == L.OK and totals == (n, nbytes) and untouched(a, status), (caps, null)
    rc, a, status, totals = call(n, nbytes)
    assert rc == L.OK and totals == (n, nbytes) and status.tolist() == status_ref + [0xEE]
    assert a["receipts"][:nbytes].tobytes() == b"".join(v for b in values for v in b) and (a["receipts"][nbytes:] == 0xEE).all()
    assert a["rc_off"][:n + 1].tolist() == np.cumsum([0] + [len(v) for b in values for v in b]).tolist() and a["rc_off"][n + 1] == 0xEEEEEEEEEEEEEEEE
    assert a["block_first"][:6].tolist() == np.cumsum([0] + [len(b) for b in values]).tolist() == [0, 3, 3, 4, 4, 6] and a["block_first"][6] == 0xEEEEEEEE
    # the ETH69 rule refuses the typed strings
    rc, a, status, totals = call(n, nbytes, flags=L.RCPTS_SPLIT_ETH69)
    assert rc == L.OK and status.tolist()[:5] == [L.SPLIT_BAD_RECEIPT, G.SPLIT_BAD_RLP, L.SPLIT_BAD_RECEIPT, 0, L.SPLIT_BAD_RECEIPT] and totals == (0, 0)
    # refusals
    status = np.zeros(8, np.uint8)
    arg = L.PhantReceiptsSplit(C.sizeof(L.PhantReceiptsSplit) + 8)
    assert lib.phant_receipts_decode_rlp(blob.ctypes.data, off.ctypes.data, 5, 0, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    arg = L.PhantReceiptsSplit(C.sizeof(L.PhantReceiptsSplit), 1)
    assert lib.phant_receipts_decode_rlp(blob.ctypes.data, off.ctypes.data, 5, 0, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    arg = L.PhantReceiptsSplit(C.sizeof(L.PhantReceiptsSplit))
    assert lib.phant_receipts_decode_rlp(blob.ctypes.data, off.ctypes.data, 5, 2, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    assert lib.phant_receipts_decode_rlp(blob.ctypes.data, off[::-1].copy().ctypes.data, 5, 0, C.byref(arg), status.ctypes.data) == L.E_INVALID_ARG
    assert lib.phant_receipts_decode_rlp(blob.ctypes.data, off.ctypes.data, 5, 0, C.byref(arg), None) == L.E_INVALID_ARG
    assert lib.phant_receipts_decode_rlp(None, None, 0, 0, C.byref(arg), None) == L.OK and (arg.n, arg.rc_bytes) == (0, 0)
