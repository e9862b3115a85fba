#!/usr/bin/env python3
"""Extract the reference's known answers for sender recovery into tests/golden/sender_vectors.json.

Run where the reference is mounted read-only (tests never need it):

    python tests/golden/make_sender_vectors.py [REFERENCE_DIR]

Nothing here computes a signature, a key or a hash: every value is copied from the reference's tests / fixtures.

  erecover   src/crypto/ecdsa.zig:39-43   the digest, the 65-byte signature (r || s || recid) and the uncompressed public key
  mainnet    src/signer/signer.zig:199-211  two (raw transaction, sender) pairs, chain id 1
  fixtures   src/tests/fixtures/**        every transaction that carries a "sender": the raw transaction out of blocks[].rlp
                                          (decoded as tests/golden/make_golden.py decodes it) and that sender, chain id 1;
                                          a transaction above 2 KB is stored as base64 of its zlib stream
"""
import base64
import json
import os
import re
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, block_body, h, read  # noqa: E402


def tx_field(raw):
    """hex, or -- the initcode-size cases carry 49 KB of repeated bytes each -- base64 of its zlib stream (tests/secp_ref.py:
    load_vectors undoes it); a committed file stays far below 1 MiB"""
    if len(raw) <= 2048:
        return {"tx": raw.hex()}
    return {"tx_zlib_b64": base64.b64encode(zlib.compress(raw, 9)).decode()}


def main():
    ec = read("src/crypto/ecdsa.zig")
    grab = lambda name: re.search(name + r' = common\.comptimeHexToBytes\("([0-9a-f]+)"\)', ec).group(1)  # noqa: E731
    sig, pub = grab("signature"), grab("uncompressed_pubkey")
    assert len(sig) == 130 and len(pub) == 130 and pub.startswith("04")
    erecover = {"hash": grab("hashed_msg"), "r": sig[:64], "s": sig[64:128], "recid": int(sig[128:], 16), "pubkey": pub[2:],
                "source": "src/crypto/ecdsa.zig:39-43"}
    sg = read("src/signer/signer.zig")
    mainnet = [{"tx": m.group(1), "sender": m.group(2), "chain_id": 1, "source": "src/signer/signer.zig:199-211"}
               for m in re.finditer(r'\.rlp_encoded = "([0-9a-f]+)",\s*\n\s*\.expected_sender = "([0-9a-f]{40})"', sg)]
    assert len(mainnet) == 2
    fixtures, files = [], set()
    base = os.path.join(REF, "src/tests/fixtures")
    for root, _, names in sorted(os.walk(base)):
        for fn in sorted(names):
            if not fn.endswith(".json"):
                continue
            rel = os.path.relpath(os.path.join(root, fn), REF)
            with open(os.path.join(root, fn)) as f:
                doc = json.load(f)
            for name, c in doc.items():
                for bi, b in enumerate(c["blocks"]):
                    # (a block the fixture expects to be refused lists its transactions under "rlp_decoded")
                    txs_json = b.get("transactions") or b.get("rlp_decoded", {}).get("transactions")
                    if not txs_json or "rlp" not in b:
                        continue
                    raw, _ = block_body(bytes.fromhex(h(b["rlp"])))
                    assert len(raw) == len(txs_json), (rel, name, bi)
                    for t, tj in zip(raw, txs_json):
                        if "sender" in tj:
                            fixtures.append({**tx_field(t), "sender": h(tj["sender"]).rjust(40, "0"), "v": h(tj["v"]),
                                             "case": name, "block": bi})
                            files.add(rel)
    doc = {"erecover": erecover, "mainnet": mainnet, "fixtures": fixtures, "fixture_chain_id": 1,
           "fixture_source": "src/tests/fixtures/shanghai/** (exec-spec-tests, MIT): %d files" % len(files)}
    with open(os.path.join(OUT, "sender_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print("sender vectors: 1 + %d + %d (%d files), v in %s" % (len(mainnet), len(fixtures), len(files), sorted({x["v"] for x in fixtures})))


if __name__ == "__main__":
    main()
