"""tests/filters_ref.py pinned: the bloom it builds for a set of logs from its own bit rule is the bloom tests/receipts_seg_ref.py computes
for the same logs (that one is held against receipt.zig's rule and against the device by the receipts' tests), and its set semantics on a
few logs by hand.  tests/golden/ holds no block whose logs and logsBloom are both known (its header vectors carry blooms without
receipts), so there is no such check here."""
import numpy as np

from tests import filters_ref as F
from tests import receipts_seg_ref as G
from tests.test_gpu_log_filters import addr, log, rows_by_hand, topic
from tests.test_gpu_receipt_segments import _enc, _plain


def test_the_bit_rule_gives_the_blooms_of_the_receipts_reference():
    logs = [log(k) for k in range(40)]
    blocks = [[logs[:3], logs[3:10]], [], [[]], [logs[10:]]]
    for form in (G.CONSENSUS, G.ETH69):
        out, *_ = G.expected(_enc([[_plain(i, logs=ls) for i, ls in enumerate(b)] for b in blocks], form), form)
        for b, mine in enumerate(([x for a, ts, _ in logs[:10] for x in [a] + ts], [], [], [x for a, ts, _ in logs[10:] for x in [a] + ts])):
            assert out["logs_bloom"][256 * b:256 * b + 256] == F.bloom_of(mine), (form, b)
    for a, ts, _ in logs:
        assert all(F.in_bloom(F.bloom_of([a] + ts), e) for e in [a] + ts)


def test_known_bits():
    """keccak256 of twenty zero bytes is 5380c7b7ae81a58eb98d9c78de4a1fd7fd9535fc953ed2be602daaa41767312a: the values 0x380, 0x7b7, 0x681"""
    assert F.bloom_values(bytes(20)) == [0x5380 & 0x7FF, 0xC7B7 & 0x7FF, 0xAE81 & 0x7FF]
    assert F.bloom_bits(bytes(20))[0] == ((2047 - 0x380) // 8, 1 << (7 - (2047 - 0x380) % 8))
    b = bytearray(256)
    b[255] = 1  # value 0: the last byte's lowest bit
    assert [(2047 - v) // 8 for v in (0, 7, 8, 2047)] == [255, 255, 254, 0] and 1 << (7 - (2047 - 0) % 8) == 1 and 1 << (7 - (2047 - 2047) % 8) == 0x80


def test_set_semantics_by_hand():
    logs = [log(0, 0), log(1, 1), log(2, 2), (addr(1), [topic(2, 0), topic(1, 0)], b"")]
    rows = rows_by_hand([[logs[:2]], [], [logs[2:]]])
    filters = [F.Filter(), F.Filter([addr(1)]), F.Filter([], [[topic(1, 0)]]), F.Filter([], [[], [topic(1, 0)]]), F.Filter([addr(1), addr(1)], [[topic(2, 0), topic(1, 0)]]),
               F.Filter(lo=1), F.Filter(hi=1), F.Filter(lo=1, hi=2), F.Filter([], [[], [], []])]
    exp, n = F.expected_matches(rows, filters)
    first = np.frombuffer(exp["filter_first"], "<u4").tolist()
    match = np.frombuffer(exp["match_log"], "<u4").tolist()
    assert [match[a:b] for a, b in zip(first, first[1:])] == [[0, 1, 2, 3], [1, 3], [1], [3], [1, 3], [2, 3], [0, 1], [], [0, 1, 2, 3]] and n == len(match)
    assert np.frombuffer(exp["filter_count"], "<u4").tolist() == [4, 2, 1, 1, 2, 2, 2, 0, 4]
    may, count = F.expected_may([F.bloom_of([addr(1)]), bytes(256), b"\xff" * 256], [F.Filter([addr(1)]), F.Filter(), F.Filter([addr(1)], lo=1)])
    assert np.frombuffer(may, "<u8").tolist() == [0b101, 0b111, 0b100] and np.frombuffer(count, "<u4").tolist() == [2, 3, 1]
