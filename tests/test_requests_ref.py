"""tests/requests_ref.py, the definition of phant_block_requests, held against an independent restatement of the EIP-7685 formula, the
constant an empty block commits to, and the layout arithmetic of the deposit event: a builder that ABI-encodes five `bytes` values
generically must produce exactly the 576 bytes and the offsets the rule names.  No GPU, no library."""
import hashlib

import numpy as np

from tests import requests_ref as Q

CONTRACT = bytes(range(1, 21))


def _eip7685(requests):
    m = hashlib.sha256()
    for r in requests:
        if len(r) > 1:
            m.update(hashlib.sha256(r).digest())
    return m.digest()


def test_the_formula_and_the_empty_constant():
    assert Q.requests_hash([]) == Q.EMPTY_HASH == hashlib.sha256(b"").digest() == _eip7685([])
    assert Q.requests_hash([(1, b"")]) == Q.EMPTY_HASH  # (a request without data is left out)
    rng = np.random.default_rng(5)
    for n in range(1, 5):
        reqs = [(t, rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()) for t in range(n)]
        assert Q.requests_hash(reqs) == _eip7685([bytes([t]) + d for t, d in reqs])
    assert Q.requests_hash([(0, b"a"), (1, b"b")]) != Q.requests_hash([(1, b"b"), (0, b"a")])


def test_the_event_topic_is_the_signature_hash(oracle):
    """the constant is keccak256 of the event's signature, by the oracle's Keccak"""
    assert oracle.keccak256(b"DepositEvent(bytes,bytes,bytes,bytes,bytes)") == Q.DEPOSIT_TOPIC


def test_the_layout_arithmetic():
    f = [bytes([k + 1]) * n for k, n in enumerate(Q.SIZES)]
    d = Q.deposit_event(*f)
    assert len(d) == Q.EVENT_BYTES == 576
    word = lambda at: int.from_bytes(d[at:at + 32], "big")  # noqa: E731
    assert [word(32 * k) for k in range(5)] == list(Q.OFFSETS) == [160, 256, 320, 384, 512]
    assert [word(o) for o in Q.OFFSETS] == list(Q.SIZES) == [48, 32, 8, 96, 8]
    assert Q.well_formed(d, len(d), 0, len(d)) and Q.deposit_row(d) == b"".join(f) and len(Q.deposit_row(d)) == Q.ROW_BYTES
    # a field of another size moves every offset behind it: the generic builder no longer produces the fixed layout
    assert not Q.well_formed(Q.abi_bytes([f[0] + b"\x00"] + f[1:]), 576, 0, 576)
    assert not Q.well_formed(d, 575, 0, 576) and not Q.well_formed(b"\x00" + d, 577, 1, 575) and Q.well_formed(b"\x00" + d, 577, 1, 576)


def test_expected_on_a_hand_made_segment():
    f = [bytes([k + 1]) * n for k, n in enumerate(Q.SIZES)]
    good = Q.deposit_event(*f)
    bad = good[:31] + b"\xa1" + good[32:]
    logs = [(CONTRACT, [Q.DEPOSIT_TOPIC], good), (b"\x09" * 20, [Q.DEPOSIT_TOPIC], good), (CONTRACT, [Q.DEPOSIT_TOPIC, b"\x01" * 32], bad), (CONTRACT, [], good),
            (CONTRACT, [Q.DEPOSIT_TOPIC], good)]
    blob, at = b"", []
    for _, _, d in logs:
        at.append(len(blob))
        blob += d
    a = {"receipts": np.frombuffer(blob, np.uint8), "block_first": [0, 2, 2, 3], "log_first": [0, 1, 3, 5], "address": np.frombuffer(b"".join(x for x, _, _ in logs), np.uint8),
         "topic_first": [0, 1, 2, 4, 4, 5], "topics": np.frombuffer(b"".join(t for _, ts, _ in logs for t in ts), np.uint8), "data_at": at, "data_len": [576] * 5}
    other = [[(1, b"w")], [(2, b"c"), (1, b"w")], []]
    out, nd, first_bad = Q.expected(a, CONTRACT, other)
    row = b"".join(f)
    assert nd == 2 and first_bad == 0 and out["deposit"] == row * 2 and np.frombuffer(out["deposit_log"], "<u4").tolist() == [0, 4]
    assert np.frombuffer(out["block_flags"], "<u4").tolist() == [Q.LAYOUT, Q.ORDER, 0] and np.frombuffer(out["deposit_first"], "<u4").tolist() == [0, 1, 1, 2]
    assert out["requests_hash"] == _eip7685([b"\x00" + row, b"\x01w"]) + _eip7685([b"\x02c", b"\x01w"]) + _eip7685([b"\x00" + row])
    out, nd, first_bad = Q.expected(a, CONTRACT, other, active=[0, 1, 1], exp_hash=[b"\x01" * 32] * 3)
    assert nd == 1 and first_bad == 1 and np.frombuffer(out["block_flags"], "<u4").tolist() == [0, Q.ORDER | Q.HASH, Q.HASH] and out["requests_hash"][:32] == bytes(32)
