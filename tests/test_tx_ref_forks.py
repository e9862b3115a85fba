"""tests/tx_ref_forks.py, the definition phant_block_transactions_ex is checked against, pinned by numbers worked out by hand from
EIP-4844, EIP-7702 and EIP-7623, by the blob base fee's known values, and by signing and recovering.  No public vector of a type-3 or
type-4 transaction is part of this repository: these are the evidence."""
from tests import secp_ref as S
from tests import tx_ref as T
from tests import tx_ref_forks as F

D, D2 = 0xC0FFEE, 0xA11CE


def _address(oracle, d):
    return oracle.keccak256(S.pubkey_bytes(S.mul(d, S.G)))[12:]


def test_three_transactions_by_hand(oracle):
    # 1. a blob transaction: 2 blobs, calldata 00 01 02 00 (2 zero, 2 non-zero bytes), one access-list address with one key
    tx = F.raw_tx(3, data=b"\x00\x01\x02\x00", al=S.rlp_list([S.rlp_list([S.rlp_bytes(b"\x22" * 20), S.rlp_list([S.rlp_bytes(b"\x01" * 32)])])]),
                  hashes=[F.versioned(0), F.versioned(1)], blob_fee=7, max_fee=100, max_priority=2, gas=30000, value=5)
    o, auths = F.analyse(oracle, tx, 1, F.PRAGUE, base_fee=10, blob_fee_base=7, recover=False)
    assert o["intrinsic_gas"] == 21000 + 2 * 4 + 2 * 16 + 2400 + 1900 == 25340
    assert o["floor_gas"] == 21000 + 10 * (2 + 4 * 2) == 21100
    assert int.from_bytes(o["upfront_cost"], "big") == 30000 * 100 + 5 + 2 * 131072 * 7 == 4835013
    assert int.from_bytes(o["effective_gas_price"], "big") == 12 and o["flags"] == 0 and o["blobs"] == 2 and auths == []
    assert F.analyse(oracle, tx, 1, F.PRAGUE, blob_fee_base=8, recover=False)[0]["flags"] == F.BLOB_FEE_BELOW_BASE
    assert F.analyse(oracle, tx, 1, F.LONDON, recover=False)[0]["flags"] == T.UNDECODABLE
    assert F.analyse(oracle, tx, 1, F.CANCUN, recover=False)[0]["floor_gas"] == 0
    # 2. a set-code transaction: 3 authorizations, 10 non-zero bytes of calldata -- the floor is below the intrinsic gas
    tx = F.raw_tx(4, data=b"\xff" * 10, auths=[F.raw_tuple(1, b"\x77" * 20, k, 0, 1, 1) for k in range(3)], gas=96160, max_fee=3, value=0)
    o, auths = F.analyse(oracle, tx, 1, F.PRAGUE, recover=False)
    assert o["intrinsic_gas"] == 21000 + 10 * 16 + 3 * 25000 == 96160 and o["floor_gas"] == 21000 + 10 * 40 == 21400
    assert int.from_bytes(o["upfront_cost"], "big") == 96160 * 3 and o["flags"] == 0 and len(auths) == 3
    assert F.analyse(oracle, tx, 1, F.CANCUN, recover=False)[0]["flags"] == T.UNDECODABLE
    assert F.analyse(oracle, tx + b"\x00", 1, F.PRAGUE, recover=False)[0]["flags"] == T.UNDECODABLE  # (a byte behind the list)
    # 3. a legacy transaction with 100 non-zero bytes: the floor (25000) is above the intrinsic gas (22600)
    tx = S.make_tx(oracle, D, 0, 1, data=b"\x01" * 100, gas=24999, gas_price=2, value=1)
    o, _ = F.analyse(oracle, tx, 1, F.PRAGUE)
    assert o["intrinsic_gas"] == 21000 + 1600 == 22600 and o["floor_gas"] == 21000 + 10 * 400 == 25000 and o["flags"] == F.FLOOR_GAS
    assert int.from_bytes(o["upfront_cost"], "big") == 24999 * 2 + 1
    assert F.analyse(oracle, S.make_tx(oracle, D, 0, 1, data=b"\x01" * 100, gas=25000), 1, F.PRAGUE)[0]["flags"] == 0
    assert F.analyse(oracle, tx, 1, F.CANCUN)[0]["flags"] == 0


def test_strictness_of_the_new_lists(oracle):
    bad = lambda tx: F.decode(tx, 1, F.PRAGUE)[0] == S.BAD_TX  # noqa: E731
    good = F.raw_tuple(1, b"\x77" * 20, 0, 0, 1, 1)
    assert not bad(F.raw_tx(4, auths=[good, good])) and not bad(F.raw_tx(4, auths=[])) and not bad(F.raw_tx(3, hashes=[]))
    seven = S.rlp_list([S.rlp_int(1), S.rlp_bytes(b"\x77" * 20), b"\x80", b"\x80", b"\x01", b"\x01", b"\x80"])
    five = S.rlp_list([S.rlp_int(1), S.rlp_bytes(b"\x77" * 20), b"\x80", b"\x80", b"\x01"])
    for t in (seven, five, S.rlp_bytes(b"\x01" * 30), F.raw_tuple(1, b"\x77" * 19, 0, 0, 1, 1), F.raw_tuple(1, b"\x77" * 21, 0, 0, 1, 1),
              F.raw_tuple(1 << 256, b"\x77" * 20, 0, 0, 1, 1), F.raw_tuple(1, b"\x77" * 20, 1 << 64, 0, 1, 1), F.raw_tuple(1, b"\x77" * 20, 0, 256, 1, 1),
              F.raw_tuple(1, b"\x77" * 20, 0, 0, 1 << 256, 1), F.raw_tuple(1, b"\x77" * 20, 0, 0, 1, 1 << 256),
              S.rlp_list([b"\x81\x01", S.rlp_bytes(b"\x77" * 20), b"\x80", b"\x80", b"\x01", b"\x01"]),
              S.rlp_list([b"\x01", S.rlp_bytes(b"\x77" * 20), b"\x82\x00\x01", b"\x80", b"\x01", b"\x01"])):
        assert bad(F.raw_tx(4, auths=[good, t])), t.hex()
    assert not bad(F.raw_tx(4, auths=[F.raw_tuple(F.M256, b"\x77" * 20, F.M64, 255, F.M256, F.M256)]))
    for hashes in ([b"\x01" * 31], [b"\x01" * 33], [F.versioned(0), b""], S.rlp_bytes(b"\x01" * 32), S.rlp_list([S.rlp_list([S.rlp_bytes(F.versioned(0))])])):
        assert bad(F.raw_tx(3, hashes=hashes)), hashes
    assert bad(F.raw_tx(3, blob_fee=1 << 256)) and not bad(F.raw_tx(3, blob_fee=F.M256))
    assert bad(F.raw_tx(3)[:-1]) and bad(F.raw_tx(4) + b"\x00") and bad(b"\x03") and bad(b"\x04\xc0")
    assert F.decode(F.raw_tx(3, v=2), 1, F.PRAGUE)[0] == S.BAD_V and F.decode(F.raw_tx(4, v=1), 1, F.PRAGUE)[0] == S.OK
    # thirteen items under 0x03 and fourteen under 0x04 are neither
    assert bad(b"\x03" + F.raw_tx(4)[1:]) and bad(b"\x04" + F.raw_tx(3)[1:])


def test_blob_base_fee():
    """EIP-4844: fake_exponential(1, 0, d) = 1; the fee grows with the excess, ~ e^(excess / d)"""
    for fork, d in ((F.CANCUN, 3338477), (F.PRAGUE, 5007716)):
        assert F.blob_base_fee(0, fork) == 1 and F.blob_base_fee(d, fork) == 2  # e = 2.718...
        fees = [F.blob_base_fee(k * 393216, fork) for k in range(0, 400, 7)]
        assert all(a <= b for a, b in zip(fees, fees[1:])) and fees[-1] > fees[0]
        assert F.blob_base_fee(10 * d, fork) in range(22020, 22030)  # e^10 = 22026.47
    assert F.blob_base_fee(10**8, F.CANCUN) > F.blob_base_fee(10**8, F.PRAGUE)
    from phant_amd.types import transaction as X
    for excess in (0, 1, 393216, 3338477, 5007716, 10**8, 2**40 // 1000):
        for fork in (F.CANCUN, F.PRAGUE):
            assert X.blob_base_fee(excess, fork) == F.blob_base_fee(excess, fork)


def test_sign_then_recover(oracle):
    me, authority = _address(oracle, D), _address(oracle, D2)
    for typ, kw in ((3, dict(hashes=[F.versioned(k) for k in range(2)])), (4, dict(auths=[F.make_authorization(oracle, D2, 1, nonce=7),
                                                                                              F.make_authorization(oracle, D2, 0),
                                                                                              F.make_authorization(oracle, D2, 1, high_s=True)]))):
        tx = F.make_tx(oracle, D, typ, 1, data=b"ab", **kw)
        o, auths = F.analyse(oracle, tx, 1, F.PRAGUE)
        assert o["sender"] == me and o["sig_status"] == S.OK and o["flags"] == 0 and o["type"] == typ
        st, f, (pre, r, s, recid) = F.decode(tx, 1, F.PRAGUE)
        assert pre[0] == typ and S.recover(int.from_bytes(oracle.keccak256(pre), "big"), r, s, recid, S.LOW_S)[0] == S.OK
        twin = F.analyse(oracle, F.make_tx(oracle, D, typ, 1, data=b"ab", high_s=True, **kw), 1, F.PRAGUE)[0]
        assert twin["sig_status"] == S.HIGH_S and twin["flags"] == T.SIGNATURE and twin["sender"] == bytes(20)
        if typ == 4:
            assert [a["auth_status"] for a in auths] == [S.OK, S.OK, S.HIGH_S] and [a["authority"] for a in auths] == [authority, authority, bytes(20)]
            assert auths[0]["auth_nonce"] == 7 and auths[0]["auth_hash"] == oracle.keccak256(b"\x05" + S.rlp_list([b"\x01", b"\x94" + b"\x77" * 20, b"\x07"]))
            # the slow recovery of tests/secp_ref.py agrees
            a = auths[0]
            st, q = S.recover(int.from_bytes(a["auth_hash"], "big"), int.from_bytes(a["auth_sig"][:32], "big"), int.from_bytes(a["auth_sig"][32:64], "big"),
                              a["auth_sig"][64], S.LOW_S)
            assert st == S.OK and S.address(oracle, q) == authority
