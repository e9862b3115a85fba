"""phant_amd/csrc/rlp.h -- the one statement of RLP's rules that every kernel and all host code share -- compiled by a bare g++ as a
stand-alone program under AddressSanitizer + UBSan (tests/native/rlp_main.cpp) and held against an encoder and a decoder written here,
from the Yellow Paper's appendix B and independent of csrc: the writers and their length functions at every boundary of the rules, and
the decoder, with 32-bit and with size_t offsets, over every truncation and every header byte of those encodings.  No GPU and no
Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def be(v):
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def enc_hdr(base, n):
    return bytes([base + n]) if n <= 55 else bytes([base + 55 + len(be(n))]) + be(n)


def enc_str(s):
    return s if len(s) == 1 and s[0] < 0x80 else enc_hdr(0x80, len(s)) + s


def enc_uint(v):
    return enc_str(be(v))


def dec(buf):
    """(pay, len, total, is_list) of the canonical item at the front of buf, or None"""
    if not buf:
        return None
    if buf[0] < 0x80:
        return 0, 1, 1, 0
    lst = int(buf[0] >= 0xC0)
    n, hdr = buf[0] - (0xC0 if lst else 0x80), 1
    if n > 55:
        hdr = 1 + n - 55
        n = int.from_bytes(buf[1:hdr], "big")
        if hdr > len(buf) or buf[1] == 0 or n <= 55:
            return None
    if n > len(buf) - hdr or (not lst and n == 1 and hdr == 1 and buf[1] < 0x80):
        return None
    return hdr, n, hdr + n, lst


def record(kind, a=0, b=0, inp=b"", exp=b""):
    return struct.pack("<cQQII", kind, a, b, len(inp), len(exp)) + inp + exp


def test_rlp_header_against_a_reference_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "rlp_main"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "rlp_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]

    # ---- writers and sizes
    lengths = [0, 1, 55, 56, 255, 256, 65535, 65536, 2**32 - 1, 2**32, 2**56, 2**64 - 1]
    ints = [0, 1, 0x7F, 0x80, 0xFF, 0x100, 2**64 - 1]
    strings = [b"", b"\x00", b"\x7f", b"\x80", b"\x81" * 55, b"\x82" * 56, b"\x83" * 256]
    words = [b"\x00" * 32, b"\x00" * 31 + b"\x05", b"\x00" * 31 + b"\x80", b"\x00\x09" + b"\x00" * 30, b"\xff" + b"\x00" * 31]  # 0, 1, 1, 31, 32 bytes
    recs = []
    for base in (0x80, 0xC0):
        recs += [record(b"h", base, n, exp=enc_hdr(base, n)) for n in lengths]
    recs += [record(b"u", v, len(be(v)), exp=enc_uint(v)) for v in ints]
    recs += [record(b"s", inp=s, exp=enc_str(s)) for s in strings]
    recs += [record(b"m", len(w.lstrip(b"\x00")), inp=w, exp=enc_str(w.lstrip(b"\x00"))) for w in words]
    n_written = len(recs)
    assert sorted(len(w.lstrip(b"\x00")) for w in words) == [0, 1, 1, 31, 32]

    # ---- the decoder's corpus: the encodings above whose payload is short, with the payload behind the bare headers
    seeds = [enc_uint(v) for v in ints] + [enc_str(s) for s in strings] + [enc_str(w.lstrip(b"\x00")) for w in words]
    seeds += [enc_hdr(0x80, n) + (b"\x84" * n) for n in lengths if n <= 256] + [enc_hdr(0xC0, n) + (b"\x01" * n) for n in lengths if n <= 256]
    corpus = [b""]  # avail == 0
    for s in seeds:
        assert dec(s) is not None and dec(s)[2] == len(s), s[:4].hex()
        corpus += [s[:k] for k in range(len(s) + 1)]  # every truncation, and the whole
        corpus += [s + b"\x55"]  # (a byte behind the item is not the item's)
        corpus += [s[:k] + bytes([x]) + s[k + 1:] for k in range(dec(s)[0] or 1) for x in range(256)]  # every value in each header byte
    for lead in (0xB7, 0xF7):
        corpus += [bytes([lead + 8]) + b"\xff" * 8 + b"\x01" * 70]  # a length field of 2^64 - 1
        corpus += [bytes([lead + 8]) + b"\xff" * 7 + b"\xc0" + b"\x01" * 70]  # (and one that wraps a 32-bit sum of header and length)
        corpus += [bytes([lead + 4]) + b"\xff\xff\xff\xf8" + b"\x01" * 70, bytes([lead + 5]) + b"\x01\x00\x00\x00\x3c" + b"\x01" * 70]  # (2^32 - 8, 2^32 + 60)
        corpus += [bytes([lead + 1, 0]) + b"\x01" * 70, bytes([lead + 2, 0, 60]) + b"\x01" * 70, bytes([lead + 3, 0, 1, 0]) + b"\x01" * 300]  # a leading zero
        corpus += [bytes([lead + 1, n]) + b"\x81" * n for n in (0, 1, 55)] + [bytes([lead + 2, 0, 55]) + b"\x81" * 55]  # long form, length <= 55
        corpus += [bytes([lead + 1, 56]) + b"\x81" * 56, bytes([lead + 2, 1, 0]) + b"\x81" * 256]  # (the least long forms: accepted)
    n_acc = n_ref = 0
    for c in corpus:
        d = dec(c)
        recs.append(record(b"d", int(d is not None), inp=c, exp=struct.pack("<4Q", *d) if d else b""))
        n_acc, n_ref = n_acc + (d is not None), n_ref + (d is None)
    assert n_acc > 2000 and n_ref > 2000

    p = tmp_path / "records.bin"
    p.write_bytes(b"".join(recs))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert [int(x) for x in re.findall(r"\d+", r.stdout)] == [n_written, n_acc, n_ref], r.stdout
