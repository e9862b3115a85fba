"""The device decode of phant_block_transactions -- tx::decode of phant_amd/csrc/transactions.hip.h, the routine tx_decode_kernel runs in
every lane -- compiled for the host as a stand-alone program under AddressSanitizer + UBSan (tests/native/tx_decode_main.cpp) and held
against host_rlp.cpp::tx_signing_parts, the decode of phant_tx_senders: every truncation, every single-byte replacement, an appended
byte and a length field of 2^64 - 1 at every position of one transaction per kind and chain id.  No GPU and no Python-loaded library
is involved."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import secp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_decode_against_the_host_decode_under_sanitizers(oracle, tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "tx_decode"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "tx_decode_main.cpp"), os.path.join(ROOT, "phant_amd", "csrc", "host_rlp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    al = [(b"\x22" * 20, [b"\x01" * 32, b"\x02" * 32]), (b"\x33" * 20, [])]
    big = (1 << 64) - 1
    seeds = [(1, S.make_tx(oracle, 7, 0, 1, data=b"\x99" * 60)), (1, S.make_tx(oracle, 7, 0, 1, eip155=False, to=b"")),
             (1, S.make_tx(oracle, 7, 1, 1, access_list=al, data=b"ab")), (1, S.make_tx(oracle, 7, 2, 1, access_list=al, data=b"\x80" * 300)),
             (big, S.make_tx(oracle, 7, 0, big, data=b"\x00")), (big, S.make_tx(oracle, 7, 2, big, access_list=al[1:])), (128, S.make_tx(oracle, 7, 0, 128)),
             (0, S.make_tx(oracle, 7, 0, 0))]
    p = tmp_path / "seeds.bin"
    p.write_bytes(b"".join(struct.pack("<IQ", len(t), cid) + t for cid, t in seeds))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert r.stdout.startswith("8 seeds: "), r.stdout
    decoded, bad_tx, bad_v = (int(x) for x in re.findall(r"(\d+) (?:decoded|BAD_TX|BAD_V)", r.stdout))
    assert decoded > 3000 and bad_tx > 3000 and bad_v > 100, r.stdout
