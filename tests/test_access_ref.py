"""tests/access_ref.py, the definition phant_block_access_lists is checked against, against rows worked out by hand and written here as
literals, and against the counts the transactions call's reference (tests/tx_ref.py) states for the same lists."""
from tests import access_ref as R
from tests import secp_ref as S
from tests import tx_ref as T

NONE = 0xFFFFFFFF
AA, BB, CC = b"\xaa" * 20, b"\xbb" * 20, b"\xcc" * 20
K1, KF = bytes(31) + b"\x01", b"\xff" * 32

# A type-1 transaction, item by item: chain id 1, nonce 0, gas price 1, gas 21000, to 11..11, value 0, no data, the access list,
# y_parity 0, r = s = 1 (nobody signed it: the list does not care).
RAW = bytes.fromhex(
    "01" "f894"                                         # the type, the list's header: 148 bytes follow
    "01" "80" "01" "825208"                              # chain id, nonce, gas price, gas
    "94" + "11" * 20 +                                  # to
    "80" "80"                                           # value, data                                    (32 bytes so far)
    "f872"                                              # the access list: 114 bytes of payload, from offset 34
    "d6" "94" + "aa" * 20 + "c0"                        #   [aa..aa, []]: 23 bytes
    "f859" "94" + "bb" * 20 +                           #   [bb..bb, [..01, ff..ff]]: 2 + 89 bytes
    "f842" "a0" + "00" * 31 + "01" "a0" + "ff" * 32 +   #     its two keys: 2 + 66 bytes
    "80" "01" "01")                                     # y_parity, r, s


def test_a_type_1_transaction_worked_out_by_hand():
    assert len(RAW) == 151
    span = RAW[34:34 + 114]
    assert R.walk(span) == [(AA, []), (BB, [K1, KF])] and R.encode([(AA, []), (BB, [K1, KF])]) == span
    st, f, _ = T.decode(RAW, 1)
    assert f["al"] == (34, 114) and (f["al_addresses"], f["al_keys"]) == (2, 2)
    # the witness: row 0 = bb..bb with the slots ff..ff, ..01, ff..ff; row 1 = cc..cc with ..01; row 2 = bb..bb again with ..01
    o, tot = R.define([b"", span], addresses=[BB, CC, BB], slot_first=[0, 3, 4, 5], slots=[KF, K1, KF, K1, K1])
    assert o == {"tuple_first": [0, 0, 2], "al_flags": [0, 0], "warm_addresses": [0, 2], "warm_keys": [0, 2],
                 "address": [AA, BB], "key_first": [0, 0, 2], "account_row": [NONE, 0], "tuple_same": [0, 1],
                 "key": [K1, KF], "slot_row": [1, 0], "key_same": [0, 1]}
    assert tot == {"n_tuples": 2, "n_keys": 2, "n_missing_accounts": 1, "n_missing_slots": 0, "first_malformed": 2}
    exp, _ = R.expected([b"", span], addresses=[BB, CC, BB], slot_first=[0, 3, 4, 5], slots=[KF, K1, KF, K1, K1])
    assert exp["tuple_first"] == bytes.fromhex("00000000" "00000000" "02000000") and exp["account_row"] == bytes.fromhex("ffffffff" "00000000")
    assert exp["address"] == AA + BB and exp["key"] == K1 + KF and exp["slot_row"] == bytes.fromhex("01000000" "00000000")
    arrays = R.inputs([b"", span], gap=b"\x07\x07")
    assert arrays["al_off"].tolist() == [0, 4] and arrays["al_len"].tolist() == [0, 114] and arrays["txs"].tobytes() == b"\x07\x07" * 2 + span + b"\x07\x07"


def test_the_malformed_flag():
    """a row that is no access-list payload contributes nothing; the rows around it keep their entries; the least such row"""
    good = bytes.fromhex("d6" "94" + "aa" * 20 + "c0")
    short_key = bytes.fromhex("f7" "94" + "bb" * 20 + "e1" "a0" + "ff" * 32)[:-1]            # the key list claims 33 bytes, 32 follow
    wrong_key = bytes.fromhex("f6" "94" + "bb" * 20 + "e0" "9f" + "ff" * 31)                 # a key of 31 bytes
    long_address = bytes.fromhex("d7" "95" + "bb" * 21 + "c0")
    assert R.walk(good) == [(AA, [])] and R.walk(short_key) is None and R.walk(wrong_key) is None and R.walk(long_address) is None
    assert R.walk(good + b"\x80") is None and R.walk(b"\xc0") is None and R.walk(b"") == []
    o, tot = R.define([good, wrong_key, good, short_key], addresses=[AA], slot_first=[0, 0])
    assert o["al_flags"] == [0, R.MALFORMED, 0, R.MALFORMED] and o["tuple_first"] == [0, 1, 1, 2, 2] and o["account_row"] == [0, 0]
    assert o["warm_addresses"] == [1, 0, 1, 0] and o["tuple_same"] == [0, 1]
    assert tot == {"n_tuples": 2, "n_keys": 0, "n_missing_accounts": 0, "n_missing_slots": 0, "first_malformed": 1}


def test_the_duplicates_flag():
    """an address twice in a row: the second tuple points at the first, a key repeated under it points at its first occurrence in either
    tuple; the same address in the next row is no repeat"""
    span = R.encode([(AA, [K1]), (BB, []), (AA, [KF, K1, KF])])
    o, tot = R.define([span, R.encode([(AA, [K1])])], addresses=[CC, AA], slot_first=[0, 1, 2], slots=[K1, KF])
    assert o["tuple_same"] == [0, 1, 0, 3] and o["key_same"] == [0, 1, 0, 1, 4] and o["al_flags"] == [R.DUPLICATES, 0]
    assert o["warm_addresses"] == [2, 1] and o["warm_keys"] == [2, 1] and o["account_row"] == [1, NONE, 1, 1]
    assert o["slot_row"] == [NONE, 1, NONE, 1, NONE]                                # (..01 lies under cc..cc's row, not under aa..aa's)
    assert (tot["n_missing_accounts"], tot["n_missing_slots"]) == (1, 2)            # bb..bb; ..01 under aa..aa once in each row


def test_counts_against_the_transactions_reference(oracle):
    """every vector and fixture transaction, and signed type-1 / type-2 transactions with lists: the walk finds as many tuples and
    keys as tests/tx_ref.py states in al_addresses / al_keys for the same span"""
    doc = S.load_vectors()
    lists = [[(AA, [K1, KF]), (BB, [])], [(CC, [K1] * 9)], [], [(AA, [])] * 4]
    txs = [v["tx"] for v in doc["mainnet"] + doc["fixtures"]] + [S.make_tx(oracle, 5 + k, 1 + k % 2, 1, access_list=al) for k, al in enumerate(lists)]
    with_lists = 0
    for tx in txs:
        st, f, _ = T.decode(tx, 1)
        assert f is not None
        entries = R.walk(tx[f["al"][0]:f["al"][0] + f["al"][1]])
        assert entries is not None and (len(entries), sum(len(ks) for _, ks in entries)) == (f["al_addresses"], f["al_keys"])
        with_lists += bool(entries)
    assert with_lists >= 3 and [R.walk(R.encode(al)) for al in lists] == lists
