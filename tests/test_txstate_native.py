"""The per-row rule and the 288-bit arithmetic of phant_block_txs_prestate -- txst::sender_rule, add288 / sub288 / less288 of
phant_amd/csrc/txstate.hip.h, the routines txst_rules_kernel and the scan run in every lane -- compiled for the host as a stand-alone
program under AddressSanitizer + UBSan (tests/native/txstate_main.cpp) and held against the rows of tests/txstate_ref.py: blocks of one
to three senders at every fork with costs of ff..ff in every dword, 2^256 - 1 and beyond, balances at and next to the need, nonces at and
next to the expected one, every kind of code and authorities.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import txstate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = [bytes([0x10 + k]) * 20 for k in range(3)]
CODES = [b"\x60\x00", b"\xef\x01\x00" + b"\x44" * 20, b"\xef\x01\x00" + b"\x44" * 19, b"\xef\x01\x02" + b"\x44" * 20]


def _limbs(v):
    return struct.pack("<9I", *[(v >> (32 * k)) & 0xFFFFFFFF for k in range(9)])


def records_of(fork, txs, accounts, auth_first, auths):
    """the definition's answer for a block, row by row, with what the rule reads worked out here"""
    out, _, _ = R.define(fork, txs, accounts, CODES, auth_first, auths)
    rank, spent, authorized, records = {}, {}, set(), []
    for i, t in enumerate(txs):
        s = out["sender_row"][i]
        a = accounts[s]
        cost = 1 << 256 if t["flags"] & R.TX_COST_OVERFLOW else t["cost"]
        before = spent.get(s, 0)
        bits = (a["code_hash"] == R.EMPTY_CODE_HASH) | (a["code_index"] == R.CODE_NONE) << 1 | \
            (a["code_index"] != R.CODE_NONE and R.is_designator(dict(a, code_hash=b""), CODES)) << 2 | (t["sender"] in authorized) << 3 | \
            (a["balance"] < before + cost) << 4
        records.append(struct.pack("<IIIIQQ", fork, i, rank.get(s, 0), bits, t["nonce"], a["nonce"]) + _limbs(cost) + _limbs(before) + _limbs(before + cost) +
                       a["balance"].to_bytes(32, "big") + struct.pack("<IQ", out["state_flags"][i], out["expected_nonce"][i]) +
                       out["spent_before"][i].to_bytes(32, "big"))
        rank[s], spent[s] = rank.get(s, 0) + 1, before + cost
        authorized |= {bytes(x) for x, st in auths[auth_first[i]:auth_first[i + 1]] if st == R.SIG_OK}
    return records


def test_rule_and_arithmetic_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "txstate"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "txstate_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(7)
    wide = [0xFFFFFFFF << (32 * k) for k in range(8)] + [R.M256, R.M256 - 1, 1 << 256, 0, 1, (1 << 255) + 1]
    records = []
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        for trial in range(120):
            kinds = [dict(), dict(code_hash=bytes(32)), dict(code_hash=bytes(32), code_index=int(rng.integers(0, 4))), dict(code_index=1)]
            accounts = [R.account(A[k], nonce=[0, 7, R.M64 - 2][int(rng.integers(0, 3))], **kinds[int(rng.integers(0, 4)) if trial % 3 == 0 else 0])
                        for k in range(3)]
            n = int(rng.integers(1, 12))
            who = rng.integers(0, 1 + trial % 3, n)
            costs = [int(wide[int(rng.integers(0, len(wide)))]) if rng.random() < 0.6 else int(rng.integers(0, 1 << 62)) for _ in range(n)]
            need = {}
            for j, c in zip(who, costs):
                need[int(j)] = need.get(int(j), 0) + c
            for j, total in need.items():  # a balance at, one below or one above what some prefix of the sequence needs
                accounts[j]["balance"] = max(0, min(R.M256, total // int(rng.integers(1, 3)) + int(rng.integers(-1, 2))))
            sent, txs = {}, []
            for j, c in zip(who, costs):
                j = int(j)
                txs.append(R.tx(A[j], max(0, min(R.M64, accounts[j]["nonce"] + sent.get(j, 0) + int(rng.integers(-1, 2)) * (rng.random() < 0.3))), c, A[j]))
                sent[j] = sent.get(j, 0) + 1
            per_tx = [int(rng.random() < 0.2) for _ in range(n)]
            auth_first = [0] + np.cumsum(per_tx).astype(int).tolist()
            auths = [(A[int(rng.integers(0, 3))], int(rng.integers(0, 2)) * 4) for _ in range(auth_first[-1])]
            records += records_of(fork, txs, accounts, auth_first, auths)
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:entries|flagged|undetermined|saturated)", r.stdout)]
    assert got[0] == len(records) > 1500 and got[1] > 300 and got[2] > 30 and got[3] > 100, r.stdout
