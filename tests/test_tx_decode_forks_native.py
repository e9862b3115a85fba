"""The fork-taking device decode of phant_block_transactions_ex -- tx::decode of phant_amd/csrc/transactions.hip.h with types 3 and 4,
the routine tx_decode_kernel runs in every lane -- compiled for the host as a stand-alone program under AddressSanitizer + UBSan
(tests/native/tx_decode_forks_main.cpp) and held against the verdicts of tests/tx_ref_forks.py: the status and the tuple and blob
counts of every truncation, every single-byte replacement and a length field of 2^64 - 1 at every position of type-3 and type-4
seeds.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import secp_ref as S
from tests import tx_ref_forks as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (0x00, 0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8, 0xFF)


def _variants(tx):
    out = [tx] + [tx[:k] for k in range(len(tx))] + [tx + b"\x00"]
    for k in range(len(tx)):
        out += [tx[:k] + bytes([b]) + tx[k + 1:] for b in VALUES if b != tx[k]]
        out += [tx[:k] + bytes([head]) + b"\xff" * 8 + tx[k:] for head in (0xBF, 0xFF)]  # a length of 2^64 - 1 from here on
    return out


def test_fork_decode_against_the_definition_under_sanitizers(oracle, tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "tx_decode_forks"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "tx_decode_forks_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    al = [(b"\x22" * 20, [b"\x01" * 32]), (b"\x33" * 20, [])]
    big = (1 << 64) - 1
    tup = [F.raw_tuple(1, b"\x77" * 20, 5, 1, 1 << 255, 3), F.raw_tuple(0, b"\x78" * 20, 0, 0, 1, 1), F.raw_tuple(F.M256, b"\x79" * 20, big, 2, 0x80, 0x7F)]
    seeds = [(1, F.raw_tx(3, data=b"\x99" * 60, hashes=[F.versioned(0), F.versioned(1, 2)])),
             (1, F.raw_tx(3, hashes=[], to=b"", al=F._access_list(al))), (big, F.raw_tx(3, chain_id=big, blob_fee=F.M256, v=1)),
             (1, F.raw_tx(4, auths=tup, data=b"ab", al=F._access_list(al))), (1, F.raw_tx(4, auths=[])), (big, F.raw_tx(4, chain_id=big, auths=tup[:1] * 3, to=b""))]
    records, counts = [], {S.OK: 0, S.BAD_TX: 0, S.BAD_V: 0}

    def entry(tx, chain_id, fork):
        st, f, _ = F.decode(tx, chain_id, fork)
        counts[st] += 1
        records.append(struct.pack("<IIQIII", len(tx), fork, chain_id, st, len(f["auths"]) if f else 0, len(f["blobs"]) if f else 0) + tx)

    for chain_id, tx in seeds:
        assert F.decode(tx, chain_id, F.PRAGUE)[0] == S.OK
        for fork in (F.LONDON, F.CANCUN):
            entry(tx, chain_id, fork)
        for v in _variants(tx):
            entry(v, chain_id, F.PRAGUE)
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:entries|decoded|BAD_TX|BAD_V|tuples|blobs)", r.stdout)]
    assert got[:4] == [len(records), counts[S.OK], counts[S.BAD_TX], counts[S.BAD_V]], r.stdout
    # (BAD_V: y_parity is one byte, and of the ten replacement values only 0x7f is a canonical integer above 1 -- one entry a seed)
    assert counts[S.OK] > 5000 and counts[S.BAD_TX] > 5000 and counts[S.BAD_V] >= len(seeds) and got[4] > 1000 and got[5] > 500, r.stdout
