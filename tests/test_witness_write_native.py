"""phant_witness_to_json's host code -- witness_json.cpp: witness_to_json -- compiled with host_rlp.cpp and a main of its own
(tests/native/witness_write_main.cpp) under AddressSanitizer + UBSan: parse -> write -> parse over per-proof and node-set documents, an
empty account list, zero-node proofs, accounts that declare nothing, quantities and bare hex, each text written into a heap buffer of
exactly the needed size and into one a byte shorter.  No GPU and no Python-loaded library is involved."""
import copy
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.witness_util import block_witness_json, node_set_document

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phant_amd", "csrc")


def _documents(oracle):
    rng = np.random.default_rng(5)
    doc, _, _ = block_witness_json(oracle, rng, n_accounts=60, n_contracts=4, max_slots=20, n_touched=10, slots_per=3)
    assert any(sp["proof"] == [] for a in doc["accounts"] for sp in a["storageProof"])  # zero-node proofs are in it
    docs = {"per_proof": doc, "node_set": node_set_document(doc, np.random.default_rng(1)),
            "node_set_state_first": node_set_document(doc, np.random.default_rng(2), state_first=True),
            "no_accounts": {"stateRoot": doc["stateRoot"], "accounts": []}, "root_only": {"stateRoot": doc["stateRoot"]},
            "no_accounts_node_set": {"stateRoot": doc["stateRoot"], "state": [], "accounts": []}}
    # accounts that declare nothing beyond what the form requires, entries without a value, members in another order
    bare = copy.deepcopy(doc)
    for i, a in enumerate(bare["accounts"]):
        for name in (("nonce", "balance"), ("codeHash",), ("storageHash",) if not a["storageProof"] else (), ("nonce", "balance", "codeHash"))[i % 4]:
            a.pop(name, None)
        for sp in a["storageProof"][::2]:
            sp.pop("value")
        if i % 3 == 0:
            bare["accounts"][i] = dict(reversed(list(a.items())))
    docs["bare"] = bare
    # zero-node proofs only, an account without a storageProof member, hex without its prefix and in capitals, odd-length quantities
    a0 = doc["accounts"][0]
    docs["zero_nodes"] = {"stateRoot": doc["stateRoot"], "accounts": [
        {"address": a0["address"][2:].upper(), "accountProof": [], "nonce": "0x1", "balance": "0xABC", "storageProof": [
            {"key": "0x0", "value": "0x0", "proof": []}, {"key": "1f", "proof": []}]},
        {"address": doc["accounts"][1]["address"], "accountProof": []}]}
    return docs


def test_parse_write_parse_under_sanitizers(oracle, tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "witness_write"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "witness_write_main.cpp"),
           os.path.join(CSRC, "witness_json.cpp"), os.path.join(CSRC, "host_rlp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    docs = _documents(oracle)
    paths = []
    for name, doc in docs.items():
        p = tmp_path / (name + ".json")
        p.write_text(json.dumps(doc, indent=1 if name == "bare" else None))
        paths.append(str(p))
    r = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    n_docs, n_proofs, n_bytes = (int(x) for x in re.match(r"(\d+) documents, (\d+) proofs, (\d+) bytes written", r.stdout).groups())
    want_proofs = sum(len(d.get("accounts", [])) + sum(len(a.get("storageProof", [])) for a in d.get("accounts", [])) for d in docs.values())
    assert n_docs == len(docs) and n_proofs == want_proofs and n_bytes > 10_000
