#!/usr/bin/env python3
"""Extract what the reference's fixtures state about their transactions into tests/golden/tx_vectors.json.gz.

Run where the reference is mounted read-only (tests never need it):

    python tests/golden/make_tx_vectors.py [REFERENCE_DIR]

Nothing here decodes a transaction or computes a value: every field is copied from the fixture JSON.

  fixtures   src/tests/fixtures/**   every transaction that carries a "sender", in the order of tests/golden/sender_vectors.json's
                                     "fixtures" (tests/golden/make_sender_vectors.py walks the same way; entry k here describes raw
                                     transaction k there): the decoded fields the JSON states -- nonce, gasPrice, gasLimit, to, value,
                                     data, v, r, s, sender -- as hex without 0x, and the block's "expectException" if it has one;
                                     data above 2 KB as base64 of its zlib stream

The fixtures hold legacy transactions only; typed transactions and access lists are pinned by the reference's type-2 mainnet vector
(tests/golden/sender_vectors.json "mainnet") and by tests/tx_ref.py.
"""
import base64
import gzip
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, h  # noqa: E402

FIELDS = ("nonce", "gasPrice", "gasLimit", "to", "value", "v", "r", "s", "sender")


def main():
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
                    txs_json = b.get("transactions") or b.get("rlp_decoded", {}).get("transactions")
                    if not txs_json or "rlp" not in b:
                        continue
                    for tj in txs_json:
                        if "sender" not in tj:
                            continue
                        e = {k: h(tj[k]) for k in FIELDS}
                        data = h(tj["data"])
                        if len(data) <= 4096:
                            e["data"] = data
                        else:
                            e["data_zlib_b64"] = base64.b64encode(zlib.compress(bytes.fromhex(data), 9)).decode()
                        e["case"], e["block"] = name, bi
                        if "expectException" in b:
                            e["expectException"] = b["expectException"]
                        fixtures.append(e)
                        files.add(rel)
    doc = {"fixtures": fixtures, "fixture_chain_id": 1,
           "fixture_source": "src/tests/fixtures/shanghai/** (exec-spec-tests, MIT): %d files" % len(files)}
    with gzip.GzipFile(os.path.join(OUT, "tx_vectors.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(doc, indent=1).encode())
    print("tx vectors: %d (%d files), exceptions: %s" % (len(fixtures), len(files), sorted({x.get("expectException", "") for x in fixtures})))


if __name__ == "__main__":
    main()
