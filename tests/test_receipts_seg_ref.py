"""tests/receipts_seg_ref.py, the definition of phant_block_receipt_segments and of its splitter, held against itself and against known
answers that owe nothing to this code: the 87 receiptTrie values of the reference's fixtures, whose receipts
tests/test_gpu_receipts.py::test_fixture_receipt_tries derives.  Encoded in both wire forms, put into messages, split and run through
the definition they must give the fixtures' roots, and the consensus form must come back from the ETH69 form byte for byte.  CPU only."""
import numpy as np
import pytest

from tests import receipts_ref as R
from tests import receipts_seg_ref as G


@pytest.fixture(scope="module")
def fixture_blocks():
    blocks, roots = G.fixture_receipts()
    assert len(blocks) == 87 and sorted(set(map(len, blocks))) == [0, 1, 2]
    return blocks, roots


@pytest.mark.parametrize("form", (G.CONSENSUS, G.ETH69))
def test_the_fixture_receipts_split_and_give_their_headers_roots(fixture_blocks, form):
    blocks, roots = fixture_blocks
    eth69 = form == G.ETH69
    raws = [G.message_item([G.encode(r, form) for r in b], eth69) for b in blocks]
    status, values = G.split_all(raws, eth69)
    assert not any(status) and values == [[G.encode(r, form) for r in b] for b in blocks]
    gas = [b[-1][2] if b else 0 for b in blocks]
    exp, first_bad_block, n_logs, n_topics, enc_len = G.expected(values, form, exp_root=roots, exp_bloom=[bytes(256)] * 87, exp_gas=gas, exp_count=[len(b) for b in blocks])
    assert exp["receipts_root"] == b"".join(roots) and first_bad_block == 87 and (n_logs, n_topics) == (0, 0)
    assert exp["block_flags"] == bytes(4 * 87) and exp["flags"] == bytes(4 * sum(map(len, blocks)))
    # the consensus encodings are the same bytes whichever form went in
    consensus = b"".join(G.encode(r, G.CONSENSUS) for b in blocks for r in b)
    assert exp["encoded"] == consensus and enc_len == len(consensus)


def test_round_trip_between_the_forms_is_the_identity():
    logs = [(b"\x11" * 20, [b"\x22" * 32, b"\x33" * 32], b"data"), (b"\x44" * 20, [], b""), (b"\x55" * 20, [b"\x66" * 32], b"\x05")]
    for receipt in [(0, True, 21000, []), (2, False, 2**32, logs), (0x7F, b"\x99" * 32, 2**64 - 1, logs[:1]), (1, True, 1, logs * 3)]:
        for form in (G.CONSENSUS, G.ETH69):
            raw = G.encode(receipt, form)
            tx_type, status, gas, got_logs, status_item, embedded = G.decode_row(raw, form)
            back = (tx_type, status_item if status == 2 else bool(status), gas, got_logs)
            assert back == (receipt[0], receipt[1], receipt[2], receipt[3]) and G.encode(back, form) == raw
            assert G.encode_consensus(back) == G.encode_consensus(receipt) and (embedded is None) == (form == G.ETH69)
        exp, *_ = G.expected([[G.encode_eth69(receipt)]], G.ETH69)
        assert exp["encoded"] == G.encode_consensus(receipt) and exp["bloom"] == R.bloom_of(receipt[3])
        assert G.decode_row(G.encode_consensus(receipt), G.ETH69) is None and G.decode_row(G.encode_eth69(receipt), G.CONSENSUS) is None


def test_rows_the_rules_refuse():
    good = G.encode_consensus((0, True, 5, [(b"\x11" * 20, [b"\x22" * 32], b"d")]))
    assert G.decode_row(good, G.CONSENSUS) is not None
    for bad in (b"", b"\x00" + good, good + b"\x00", good[:-1], b"\x80", b"\xc0"):
        assert G.decode_row(bad, G.CONSENSUS) is None
    mk = lambda items: R.rlp_list(items)  # noqa: E731
    bloom, nologs = R.rlp_str(bytes(256)), b"\xc0"
    assert G.decode_row(mk([b"\x01", b"\x05", bloom, nologs]), G.CONSENSUS) is not None
    for items in ([b"\x02", b"\x05", bloom, nologs], [b"\x01", b"\x82\x00\x05", bloom, nologs], [b"\x01", R.rlp_str(b"\x01" * 9), bloom, nologs],
                  [b"\x01", b"\x05", R.rlp_str(bytes(255)), nologs], [b"\x01", b"\x05", bloom, nologs, b"\x80"], [b"\x01", b"\x05", bloom],
                  [b"\x01", b"\x05", bloom, mk([mk([R.rlp_str(b"\x11" * 19), b"\xc0", b"\x80"])])],
                  [b"\x01", b"\x05", bloom, mk([mk([R.rlp_str(b"\x11" * 20), mk([R.rlp_str(b"\x22" * 31)]), b"\x80"])])],
                  [b"\x01", b"\x05", bloom, mk([mk([R.rlp_str(b"\x11" * 20), b"\xc0", b"\x80", b"\x80"])])]):
        assert G.decode_row(mk(items), G.CONSENSUS) is None, items
    assert G.decode_row(mk([b"\x80", b"\x01", b"\x05", nologs]), G.ETH69)[0] == 0 and G.decode_row(mk([b"\x7f", b"\x01", b"\x05", nologs]), G.ETH69)[0] == 0x7F
    for t in (b"\x00", b"\x81\x80", b"\x82\x01\x00"):
        assert G.decode_row(mk([t, b"\x01", b"\x05", nologs]), G.ETH69) is None


def test_the_flags_of_the_definition():
    r = lambda gas, logs=(): (0, True, gas, list(logs))  # noqa: E731
    log = (b"\x11" * 20, [b"\x22" * 32], b"")
    flipped = bytearray(G.encode_consensus(r(9, [log])))
    flipped[20] ^= 1
    blocks = [[G.encode_consensus(r(5)), G.encode_consensus(r(5)), G.encode_consensus(r(4)), b"\xc0", G.encode_consensus(r(1))], [G.encode_consensus(r(0))], [bytes(flipped)], []]
    exp, first_bad_block, n_logs, n_topics, _ = G.expected(blocks, G.CONSENSUS, exp_gas=[1, 0, 9, 1], exp_count=[5, 1, 1, 0])
    assert np.frombuffer(exp["flags"], "<u4").tolist() == [0, G.GAS_ORDER, G.GAS_ORDER, G.UNDECODABLE, 0, G.GAS_ORDER, G.BLOOM]
    assert np.frombuffer(exp["block_flags"], "<u4").tolist() == [G.RB_RECEIPT, G.RB_RECEIPT, G.RB_RECEIPT, G.RB_GAS_USED]
    assert np.frombuffer(exp["block_first_bad"], "<u4").tolist() == [1, 0, 0, 0] and (first_bad_block, n_logs, n_topics) == (0, 1, 1)
    assert np.frombuffer(exp["gas_used"], "<u8").tolist() == [5, 0, 2**64 - 1, 0, 1, 0, 9]


def test_the_splitter_of_the_definition():
    legacy, typed = G.encode_consensus((0, True, 5, [])), G.encode_consensus((2, True, 5, []))
    item = G.message_item([legacy, typed])
    assert G.split(item) == (G.SPLIT_OK, [legacy, typed]) and G.split(item, True)[0] == G.SPLIT_BAD_RECEIPT
    assert G.split(item + b"\x00")[0] == G.SPLIT_BAD_RLP and G.split(item[:-1])[0] == G.SPLIT_BAD_RLP and G.split(R.rlp_str(legacy))[0] == G.SPLIT_BAD_RLP
    assert G.split(R.rlp_list([R.rlp_str(b"\x80" + legacy)]))[0] == G.SPLIT_BAD_RECEIPT and G.split(R.rlp_list([b"\x80"]))[0] == G.SPLIT_BAD_RECEIPT
    assert G.split(b"\xc0") == (G.SPLIT_OK, []) and G.split(b"\xc0", True) == (G.SPLIT_OK, [])
