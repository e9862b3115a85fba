#!/usr/bin/env python3
"""Extract the reference's known answers for block headers into tests/golden/header_vectors.json.gz.

Run where the reference is mounted read-only (tests never need it):

    python tests/golden/make_header_vectors.py [REFERENCE_DIR]

Nothing here computes a hash or an encoding: every value is copied from the fixtures.

  cases   src/tests/fixtures/**   per case its chain: `genesisBlockHeader`, then every block that carries a `blockHeader` --
                                  the header's fields as the fixture spells them (hex without 0x; a zero bloom as ""), its
                                  `hash`, its raw encoding cut out of `genesisRLP` / `blocks[].rlp` (the first item of the
                                  block's list) and that whole block encoding, in hex
The JSON is gzipped as fixture_roots.json.gz is (4 000 lines of hex are nothing to read in a diff); tests/headers_ref.py:
load_vectors reads it.
"""
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, h, rlp_decode_item  # noqa: E402

FIELDS = ["parentHash", "uncleHash", "coinbase", "stateRoot", "transactionsTrie", "receiptTrie", "bloom", "difficulty", "number",
          "gasLimit", "gasUsed", "timestamp", "extraData", "mixHash", "nonce", "baseFeePerGas", "withdrawalsRoot", "blobGasUsed",
          "excessBlobGas", "parentBeaconBlockRoot", "requestsHash"]


def header_of(hdr, block_rlp):
    is_list, ps, pe, ie = rlp_decode_item(block_rlp, 0)
    assert is_list and ie == len(block_rlp)
    h_is_list, _, _, h_end = rlp_decode_item(block_rlp, ps)
    assert h_is_list
    out = {k: h(hdr[k]) for k in FIELDS if k in hdr}
    assert set(hdr) - set(FIELDS) == {"hash"}, sorted(set(hdr) - set(FIELDS))
    if int(out["bloom"] or "0", 16) == 0:
        out["bloom"] = ""
    out["hash"] = h(hdr["hash"])
    out["raw"] = block_rlp[ps:h_end].hex()
    out["block"] = block_rlp.hex()
    return out


def main():
    base = os.path.join(REF, "src/tests/fixtures")
    cases, n_headers, n_pairs = [], 0, 0
    for root, _, names in sorted(os.walk(base)):
        for fn in sorted(names):
            if not fn.endswith(".json"):
                continue
            rel = os.path.relpath(os.path.join(root, fn), REF)
            with open(os.path.join(root, fn)) as f:
                doc = json.load(f)
            for name, c in doc.items():
                chain = [header_of(c["genesisBlockHeader"], bytes.fromhex(h(c["genesisRLP"])))]
                for b in c["blocks"]:
                    if "blockHeader" in b:
                        chain.append(header_of(b["blockHeader"], bytes.fromhex(h(b["rlp"]))))
                cases.append({"file": rel, "name": name, "headers": chain})
                n_headers += len(chain)
                n_pairs += len(chain) - 1
    doc = {"source": "src/tests/fixtures/shanghai/** (exec-spec-tests, MIT)", "counts": {"cases": len(cases), "headers": n_headers, "pairs": n_pairs},
           "cases": cases}
    path = os.path.join(OUT, "header_vectors.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("header vectors:", doc["counts"], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
