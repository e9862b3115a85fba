"""tests/secp_ref.py -- the Python-integer reference of the sender recovery -- against every known answer the reference
project carries (tests/golden/sender_vectors.json), and against itself: what it signs it recovers."""
import numpy as np
import pytest

from tests import secp_ref as S


@pytest.fixture(scope="module")
def vectors():
    return S.load_vectors()


def test_curve_constants():
    assert S.on_curve(S.G) and S.mul(S.N, S.G) is None and S.mul(S.N - 1, S.G) == S.neg(S.G)
    assert S.P % 4 == 3  # the square root is the power (p + 1) / 4


def test_erecover_known_answer(vectors):
    e = vectors["erecover"]
    st, q = S.recover(int(e["hash"], 16), int(e["r"], 16), int(e["s"], 16), e["recid"])
    assert st == S.OK and S.pubkey_bytes(q).hex() == e["pubkey"]


def test_mainnet_and_fixture_senders(vectors, oracle):
    assert len(vectors["mainnet"]) == 2 and len(vectors["fixtures"]) == 81
    assert {t["v"] for t in vectors["fixtures"]} == {"25", "26"}
    for t in vectors["mainnet"] + vectors["fixtures"]:
        st, addr = S.tx_sender(oracle, t["tx"], 1)
        assert st == S.OK and addr.hex() == t["sender"], t.get("case")


def test_signs_what_it_recovers_and_the_status_order(oracle):
    rng = np.random.default_rng(5)
    for _ in range(40):
        d = int.from_bytes(rng.bytes(32), "big") % (S.N - 1) + 1
        z = int.from_bytes(rng.bytes(32), "big")
        r, s, recid = S.sign(d, z)
        assert S.recover(z, r, s, recid, S.LOW_S) == (S.OK, S.mul(d, S.G))
        assert S.recover(z, *S.high_s_twin(r, s, recid)) == (S.OK, S.mul(d, S.G))
        assert S.recover(z, *S.high_s_twin(r, s, recid), S.LOW_S)[0] == S.HIGH_S
    assert S.recover(1, 0, 0, 4)[0] == S.BAD_RECID          # recid first
    assert S.recover(1, 0, S.N - 1, 3, S.LOW_S)[0] == S.BAD_RANGE  # the range before high s
    assert S.recover(1, S.N - 1, S.N - 1, 2, S.LOW_S)[0] == S.HIGH_S  # high s before r + n >= p
    assert S.recover(1, S.N - 1, 1, 2)[0] == S.BAD_RECID


def test_transactions_of_every_type_and_their_failures(oracle):
    d = 0xC0FFEE
    want = oracle.keccak256(S.pubkey_bytes(S.mul(d, S.G)))[12:]
    al = [(b"\x22" * 20, [b"\x01" * 32, b"\x02" * 32]), (b"\x33" * 20, [])]
    for typ, kw in ((0, {}), (0, {"eip155": False}), (1, {}), (1, {"access_list": al}), (2, {}), (2, {"access_list": al, "to": b""})):
        for data in (b"", b"\x00", b"a" * 55, b"b" * 56, b"c" * 5000):
            tx = S.make_tx(oracle, d, typ, 1, data=data, **kw)
            assert S.tx_sender(oracle, tx, 1) == (S.OK, want), (typ, kw, len(data))
            for cut in range(len(tx)):
                assert S.tx_signing_parts(tx[:cut], 1)[0] == S.BAD_TX
    assert S.tx_sender(oracle, S.make_tx(oracle, d, 0, 5), 1)[0] == S.BAD_V
    assert S.tx_sender(oracle, S.make_tx(oracle, d, 2, 1, v_override=2), 1)[0] == S.BAD_V
    assert S.tx_sender(oracle, S.make_tx(oracle, d, 1, 1, high_s=True), 1)[0] == S.HIGH_S
    assert S.tx_sender(oracle, b"\x03" + S.make_tx(oracle, d, 2, 1)[1:], 1)[0] == S.BAD_TX
