"""The host side of phant_tx_senders -- the strict transaction decode and the preimage splice of phant_amd/csrc/host_rlp.cpp --
as a stand-alone program under AddressSanitizer + UBSan (tests/native/fuzz_tx_preimage.cpp): every truncation and every
single-byte replacement of one transaction per type.  No GPU and no Python-loaded library is involved."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import secp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preimage_builder_under_sanitizers(oracle, tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "fuzz_tx_preimage"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "fuzz_tx_preimage.cpp"), os.path.join(ROOT, "phant_amd", "csrc", "host_rlp.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    al = [(b"\x22" * 20, [b"\x01" * 32, b"\x02" * 32]), (b"\x33" * 20, [])]
    seeds = [S.make_tx(oracle, 7, 0, 1, data=b"\x99" * 60), S.make_tx(oracle, 7, 0, 1, eip155=False, to=b""),
             S.make_tx(oracle, 7, 1, 1, access_list=al, data=b"ab"), S.make_tx(oracle, 7, 2, 1, access_list=al, data=b"\x80" * 300)]
    p = tmp_path / "seeds.bin"
    p.write_bytes(b"".join(struct.pack("<I", len(s)) + s for s in seeds))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert r.stdout.startswith("4 seeds: "), r.stdout
    decoded, bad_tx, bad_v = (int(x) for x in __import__("re").findall(r"(\d+) (?:decoded|BAD_TX|BAD_V)", r.stdout))
    # replacements inside data, value, r or s still decode; those that break a header do not; some hit v
    assert decoded > 1000 and bad_tx > 1000 and bad_v > 100, r.stdout
