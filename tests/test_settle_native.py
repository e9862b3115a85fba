"""The per-row functions and the 320-bit signed arithmetic of phant_block_settle -- settle::classify, tx_event / wd_event, row_rule,
account_rule, add320 / sub320 / neg320 / mul_u64_u256 / clamp256 / below of phant_amd/csrc/settle.hip.h, the routines the kernels run in
every lane -- compiled for the host as a stand-alone program under AddressSanitizer + UBSan (tests/native/settle_main.cpp) and held
against the rows of tests/settle_ref.py: blocks of a few accounts at every fork with every class, values and prices of ff..ff in every
dword, gas beyond 2^32, balances at and next to the need, at zero and at 2^256 - 1.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import settle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = bytes(range(32))


def _limbs(v, k=10):
    v %= 1 << (32 * k)
    return struct.pack(f"<{k}I", *[(v >> (32 * j)) & 0xFFFFFFFF for j in range(k)])


def records_of(fork, bgl, base_fee, coinbase, txs, accounts, wd):
    """the definition's answer for a block as records, with the running sums a record carries worked out here"""
    out, _ = R.define(fork, bgl, base_fee, coinbase, txs, accounts, wd)
    proven = lambda j: j != R.ROW_NONE and accounts[j]["status"] in (R.PRESENT, R.ABSENT)  # noqa: E731
    balance, sends, touched, cum, records = [a["balance"] for a in accounts], [0] * len(accounts), set(), 0, []
    for i, t in enumerate(txs):
        f = out["settle_flags"][i]
        cls = f & (R.UPSTREAM | R.NOT_PLAIN)
        gas = 0 if cls else max(t["intrinsic"], t["floor"])
        s, r = t["sender_row"], t["to_row"]
        events = [0, 0, 0] if cls else [-(gas * t["price"] + t["value"]), t["value"], gas * (t["price"] - base_fee)]
        cum += gas
        head = struct.pack("<6I4Q", fork, t["type"], t["tx_flags"], t["state_flags"], s, r, t["intrinsic"], t["floor"], t["gas_limit"], bgl) + \
            b"".join(v.to_bytes(32, "big") for v in (t["value"], t["price"], base_fee, t["cost"])) + \
            (accounts[r]["code_hash"] if r != R.ROW_NONE else bytes(32)) + t["to"]
        records.append(b"\x01" + head + _limbs(cum, 3) + _limbs(0 if cls else balance[s]) + struct.pack("<IQ", cls, gas) + b"".join(_limbs(v) for v in events) +
                       struct.pack("<IQ", f & (R.GAS_LIMIT | R.BALANCE_SHORT), out["cumulative_gas_used"][i]) + out["balance_before"][i].to_bytes(32, "big"))
        if not cls:
            balance[s] += events[0]
            balance[r] += events[1]
            sends[s] += 1
            touched |= {s, r}
            if proven(coinbase):
                balance[coinbase] += events[2]
                touched.add(coinbase)
    for row, gwei in wd:
        records.append(b"\x03" + struct.pack("<Q", gwei) + _limbs(gwei * 10**9))
        if proven(row):
            balance[row] += gwei * 10**9
            touched.add(row)
    for j in sorted(touched):
        a = accounts[j]
        records.append(b"\x02" + struct.pack("<BBQI", a["status"], a["code_hash"] == R.EMPTY_CODE_HASH, a["nonce"], sends[j]) + _limbs(balance[j]) +
                       struct.pack("<IQ", out["account_op"][j], out["nonces_after"][j]) + out["balances_after"][j].to_bytes(32, "big") +
                       struct.pack("<I", out["account_flags"][j]))
    return records


def test_rules_and_arithmetic_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "settle"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "settle_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(7)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    wide = [0xFFFFFFFF << (32 * k) for k in range(8)] + [R.M256, R.M256 - 1, 0, 1, (1 << 255) + 1, 1 << 128]
    records = []
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        for trial in range(150):
            accounts = [R.account(pick([0, 0, 7, R.M64 - 1, R.M64]), pick([0, 0, 1, 10**18, 10**30, R.M256, R.M256 - 5, int(pick(wide))]),
                                  pick([R.PRESENT, R.PRESENT, R.PRESENT, R.ABSENT, 20]), CODE if rng.random() < 0.1 else R.EMPTY_CODE_HASH) for _ in range(4)]
            for a in accounts:
                if a["status"] == R.ABSENT:
                    a.update(nonce=0, balance=0, code_hash=R.EMPTY_CODE_HASH)
            base_fee = pick([0, 7, 10**9, 1 << 200])
            txs = []
            for i in range(int(rng.integers(0, 9))):
                price = base_fee + pick([0, 1, 5, -1, 10**9, int(pick(wide)) >> 70])
                gas = pick([21000, 21000, 21001, 53000, 1 << 33, R.M64])
                t = R.tx(int(rng.integers(0, 4)), int(rng.integers(0, 4)), value=pick([0, 1, 10**18, int(pick(wide)) >> pick([0, 1, 64])]), price=max(price, 0),
                         gas_limit=gas, intrinsic=pick([gas, 21000, gas - 1 if gas > 1 else 1]), floor=pick([0, 0, 21500, gas]),
                         to=pick([b"\x22" * 20, bytes(19) + bytes([pick([0, 1, 9, 10, 11, 17, 18])]), bytes([1]) + bytes(19)]), type=pick([0, 1, 2, 2, 2, 3, 4]),
                         tx_flags=pick([0] * 12 + [R.TX_IS_CREATE, 0x20, 0x20000, 0x400]), state_flags=pick([0] * 12 + [R.TXST_SKIPPED, R.TXST_UNDETERMINED, 0x10, 0x400]))
                t["cost"] = min(t["cost"], R.M256) if rng.random() < 0.8 else pick([0, accounts[t["sender_row"]]["balance"], min(accounts[t["sender_row"]]["balance"] + 1, R.M256)])
                if t["tx_flags"] & R.TX_IS_CREATE or rng.random() < 0.03:
                    t["to_row"] = R.ROW_NONE
                txs.append(t)
            wd = [(pick([0, 1, 2, 3, R.ROW_NONE]), pick([0, 0, 1, 10**9, R.M64])) for _ in range(int(rng.integers(0, 5)))]
            accounts.append(R.account())  # present and empty, named by nothing but ...
            if trial % 3 == 0:
                wd.append((4, 0))          # ... a withdrawal of nothing: EIP-161 deletes it
            bgl = pick([30_000_000, 21000 * max(len(txs), 1), R.M64, 0])
            records += records_of(fork, bgl, base_fee, pick([0, 1, 2, 3, R.ROW_NONE]), txs, accounts, wd)
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:entries|plain|flagged|deleted|clamped)", r.stdout)]
    assert got[0] == len(records) > 2000 and got[1] > 300 and got[2] > 100 and got[3] > 10 and got[4] > 20, r.stdout
