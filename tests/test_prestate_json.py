"""The execution-witness document (phant_exec_witness_parse_json): host-only parsing, no GPU.  Accepted and rejected shapes with
their byte offsets, the key forms, duplicate collapse and the order / slot_first layout the pre-state is computed in."""
import json

import numpy as np
import pytest

from phant_amd import stateless as S
from tests import prestate_ref as R

A1, A2, A3 = bytes([1]) * 20, bytes([2]) * 20, bytes([3]) * 20


def slot(n):
    return n.to_bytes(32, "big")


def parse(doc):
    return S.StatelessWitness.parse_json(doc if isinstance(doc, str) else json.dumps(doc))


def test_accounts_and_slots_in_order_of_first_appearance():
    keys = [A2 + slot(7), A1, A2, A1 + slot(3), A2 + slot(5), A2 + slot(7), A1 + slot(3), A3, A1 + slot(1), A1]
    w = parse({"state": ["0xc0"], "keys": ["0x" + k.hex() for k in keys], "headers": [{"x": 1}]})
    i = w.info()
    assert [bytes(a) for a in i["addresses"]] == [A2, A1, A3]
    assert i["slot_first"].tolist() == [0, 2, 4, 4]
    assert [int.from_bytes(bytes(s), "big") for s in i["slots"]] == [7, 5, 3, 1]
    assert i["n_codes"] == 0 and i["total_nodes"] == 1 and i["nodes"].tobytes() == b"\xc0"
    # the reference's reading of the same document
    addrs, slots = R.keys_of({"keys": ["0x" + k.hex() for k in keys]})
    assert addrs == [A2, A1, A3] and slots == [[slot(7), slot(5)], [slot(3), slot(1)], []]
    w.close()


def test_codes_nodes_and_hex_conventions():
    w = parse('{"keys": [], "codes": ["0x", "0x6001", "6002", "0x0"], "state": ["0xc0", "c180"], "extra": null}')
    i = w.info()
    assert i["code_off"].tolist() == [0, 0, 2, 4, 4] and i["codes"].tobytes() == b"\x60\x01\x60\x02"
    assert i["node_off"].tolist() == [0, 1, 3] and i["n_accounts"] == 0 and i["slot_first"].tolist() == [0]
    w.close()
    w = parse({"state": [], "keys": ["0x" + A1.hex()]})  # no codes member: no codes
    assert w.info()["n_codes"] == 0 and w.info()["n_accounts"] == 1
    w.close()


# (the offset: just behind the string, member or character the parser stopped at)
@pytest.mark.parametrize("doc,msg,at", [
    ('{"state": [], "keys": ["0x' + "11" * 32 + '"]}', "key 0 is a 32-byte slot without its address", 91),
    ('{"state": [], "keys": ["0x' + "11" * 20 + '", "0x' + "22" * 21 + '"]}', "key 1 is 21 bytes", 115),
    ('{"state": [], "keys": ["0x' + "11" * 53 + '"]}', "key 0 is 53 bytes", 133),
    ('{"state": [], "keys": ["0x1"]}', "key 0 is not hex data", 28),
    ('{"state": [], "keys": ["0xzz"]}', "key 0 is not hex data", 29),
    ('{"state": ["0xc"], "keys": []}', "state node is not hex data", 16),
    ('{"state": [], "codes": ["0x6g"], "keys": []}', "code is not hex data", 30),
    ('{"keys": []}', 'missing "state"', 12),
    ('{"state": []}', 'missing "keys"', 13),
    ('{"state": [], "keys": [], "state": []}', 'duplicate "state"', 34),
    ('{"state": [], "keys": [], "codes": [], "codes": []}', 'duplicate "codes"', 47),
    ('{"state": [], "keys": []} x', "trailing characters", 26),
    ('{"state": [], "keys": [1]}', "expected a string", 23),
    ('["state"]', "unexpected character", 0),
])
def test_rejected_documents_with_their_byte_offsets(doc, msg, at):
    with pytest.raises(S.WitnessFormatError) as e:
        parse(doc)
    text = str(e.value)
    assert msg in text and text.endswith(f" at byte {at}"), text
    assert "PHANT_" not in text


def test_duplicates_collapse_and_agree_with_the_reference():
    rng = np.random.default_rng(1)
    addrs = [rng.integers(0, 256, 20, dtype=np.uint8).tobytes() for _ in range(40)]
    keys = []
    for _ in range(600):
        a = addrs[int(rng.integers(0, len(addrs)))]
        keys.append(a if rng.random() < 0.3 else a + slot(int(rng.integers(0, 30))))
    doc = {"state": [], "keys": ["0x" + k.hex() for k in keys]}
    w = parse(doc)
    i = w.info()
    want_a, want_s = R.keys_of(doc)
    assert [bytes(a) for a in i["addresses"]] == want_a
    assert i["slot_first"].tolist() == np.cumsum([0] + [len(s) for s in want_s]).tolist()
    assert [bytes(s) for s in i["slots"]] == [s for ss in want_s for s in ss]
    assert len(set(bytes(s) + bytes(a) for a, s in zip(np.repeat(i["addresses"], np.diff(i["slot_first"]), axis=0), i["slots"]))) == i["n_slots"]
    w.close()


def test_the_existing_witness_parser_is_unchanged_by_the_new_form():
    """An execution witness is not an EIP-1186 document: the existing parser still wants its stateRoot."""
    from phant_amd.engine_api import ExecutionWitness, WitnessFormatError
    with pytest.raises(WitnessFormatError):
        ExecutionWitness.parse_json(json.dumps({"state": [], "keys": []}))
