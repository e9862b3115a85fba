"""The host side of phant_headers_decode_rlp -- the strict header decode of phant_amd/csrc/host_rlp.cpp -- as a stand-alone program
under AddressSanitizer + UBSan (tests/native/fuzz_headers_rlp.cpp): every truncation and every single-byte replacement of three
fixture headers; every input is either refused or re-encodes to itself.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import headers_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_decoder_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "fuzz_headers_rlp"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "fuzz_headers_rlp.cpp"), os.path.join(ROOT, "phant_amd", "csrc", "host_rlp.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    chains = H.load_vectors()
    seeds = [chains[0][0][2], chains[0][1][2], max((x for c in chains for x in c), key=lambda x: x[0]["block_number"])[2]]
    assert len({bytes(s) for s in seeds}) == 3
    p = tmp_path / "seeds.bin"
    p.write_bytes(b"".join(struct.pack("<I", len(s)) + s for s in seeds))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    assert r.stdout.startswith("3 seeds: "), r.stdout
    decoded, refused = (int(x) for x in re.findall(r"(\d+) (?:decoded|refused)", r.stdout))
    # a replacement inside a hash, the bloom or an integer's low bytes still decodes (to other fields); one that breaks a header,
    # a width or an integer's leading byte does not
    assert decoded > 100_000 and refused > 5_000 and decoded + refused == sum(len(s) * 256 + 2 for s in seeds), r.stdout
