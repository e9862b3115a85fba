"""The trie-order functions of phant_amd/csrc/segment_lists.hip.h -- pos_of_index, index_of_pos and key_bytes_before, which decide where
every transaction, withdrawal and receipt of a segment lies in its trie -- compiled as a stand-alone program under AddressSanitizer +
UBSan (tests/native/segment_lists_main.cpp) and held against the definition of the keys: for every list length from 0 to 0x102 and for
0xffff, 0x10000 and 0x10001 the two functions are inverse permutations, the positions visit the indices in the bytewise order of
rlp(index), and key_bytes_before sums those keys' lengths; then key_bytes_before on each side of 0x1000000.  No GPU is involved, and
nothing loaded into Python runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trie_order_against_the_keys_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "segment_lists"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
           "-I", os.path.join(ROOT, "tests", "native", "shim"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "segment_lists_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    lengths, points = map(int, re.fullmatch(r"(\d+) lengths, (\d+) points\n", r.stdout).groups())
    assert lengths == 0x103 + 3 and points >= 4
