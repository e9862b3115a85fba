"""The leaf rules and the walkers' slot and divergence decisions of phant_mpt_verify_ranges -- range::leaf_rule, cmp_keys and SideRule of
phant_amd/csrc/range_verify.hip.h, the routines range_leaf_rule_kernel and the two walkers run in every lane -- compiled for the host
as a stand-alone program under AddressSanitizer + UBSan (tests/native/ranges_main.cpp) and held against tests/range_ref.py: leaves
with values of every length at and next to the bounds, keys equal to, next to and far from their predecessor and their origin in the
first, a middle and the last byte, every nibble on either side, both divergences on either side.  No GPU and no Python-loaded library
is involved."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import range_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Sized:
    """a value of which the rules see all they look at: its length"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def leaf_record(key, vlen, prev, origin):
    """the definition's answer for one leaf"""
    leaves = ([(prev, b"v")] if prev is not None else []) + [(key, Sized(vlen))]
    st, j = R.leaf_rules(origin if origin is not None and prev is None else bytes(32), leaves, origin is not None and prev is None)
    want = st if j == len(leaves) - 1 else 0
    flags = (1 if prev is not None else 0) | (2 if origin is not None and prev is None else 0)
    return struct.pack("<IIQ", 0, flags, vlen) + key + (prev or bytes(32)) + (origin or bytes(32)) + struct.pack("<I", want) + bytes(12)


def test_rules_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "ranges"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "ranges_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(3)
    records = []
    lengths = [0, 1, 2, 55, 56, 559, 560, 561, 562, 1 << 16, (1 << 32) - 1, 1 << 32, (1 << 32) + 560, 1 << 62]
    for trial in range(400):
        key = bytearray(rng.bytes(32))
        other = bytearray(key)
        where = [0, 15, 31][trial % 3]
        step = [0, 1, -1, 16, -16][trial % 5]
        other[where] = (other[where] + step) % 256
        if trial % 7 == 0:
            other = bytearray(rng.bytes(32))
        if trial % 11 == 0:
            key, other = bytearray(bytes(32)), bytearray([255] * 32)
        key, other = bytes(key), bytes(other)
        for vlen in (lengths if trial < 40 else [lengths[trial % len(lengths)], 33]):
            records.append(leaf_record(key, vlen, None, None))           # the first leaf of a range without a proof
            records.append(leaf_record(key, vlen, other, None))          # a leaf behind another
            records.append(leaf_record(other, vlen, key, None))
            records.append(leaf_record(key, vlen, key, None))            # the same key twice
            records.append(leaf_record(key, vlen, None, other))          # the first leaf of a range with a proof
            records.append(leaf_record(other, vlen, None, key))
            records.append(leaf_record(key, vlen, None, key))            # at its origin
    for right in (0, 1):
        for nib in range(16):
            mask = sum(1 << s for s in R.slots_of(nib, bool(right)))
            records.append(struct.pack("<IIII", 1, right, nib, mask) + bytes(112))
        for before in (0, 1):  # the node's path against the key's nibbles: smaller (it sorts in front of the key) or greater
            path, mine = ((1, 2), (1, 3)) if before else ((1, 3), (1, 2))
            records.append(struct.pack("<IIII", 2, right, before, int(R.diverging(path, mine, bool(right)))) + bytes(112))
    assert all(len(x) == 128 for x in records)
    corpus = tmp_path / "corpus.bin"
    corpus.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    counted = [int(x) for x in r.stdout.replace("(", " ").split() if x.isdigit()]
    assert counted[0] == len(records) and counted[2] > 1000 and counted[3:] == [32, 4], r.stdout
