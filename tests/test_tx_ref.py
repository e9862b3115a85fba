"""tests/tx_ref.py, the definition phant_block_transactions is checked against, against what the reference's fixtures state about their
own transactions (tests/golden/tx_vectors.json.gz: copied values, nothing computed) and against the reference's two mainnet vectors."""
import collections

from tests import secp_ref as S
from tests import tx_ref as T

# https://etherscan.io/tx/0x4debed... and 0x8fe400...: src/types/transaction.zig:283-303
MAINNET_HASHES = ("4debed4e6d4fdbc05c2f9198733b24f2f8b08452b6d3d70cb8f86bf0d3f7aa8c", "8fe4006825c930e54e5c418a030cd57e90988eb627155aa366927afcfd2454ff")


def _fixtures():
    raw, stated = S.load_vectors()["fixtures"], T.load_vectors()["fixtures"]
    assert len(raw) == len(stated) == 81
    return list(zip(raw, stated))


def test_fields_and_senders_of_every_fixture_transaction(oracle):
    for raw, want in _fixtures():
        tx = raw["tx"]
        o = T.analyse(oracle, tx, 1)
        assert not o["flags"] & (T.UNDECODABLE | T.BAD_V | T.SIGNATURE), want["case"]
        got = dict(nonce=o["nonce"], gasPrice=int.from_bytes(o["gas_price"], "big"), gasLimit=o["gas_limit"], value=int.from_bytes(o["value"], "big"),
                   r=int.from_bytes(o["sig"][:32], "big"), s=int.from_bytes(o["sig"][32:64], "big"), sender=o["sender"],
                   to=b"" if o["flags"] & T.IS_CREATE else o["to"], data=tx[o["data_off"]:o["data_off"] + o["data_len"]])
        assert got == {k: want[k] for k in got}, want["case"]
        assert want["v"] in (27, 28, 37, 38) and o["sig"][64] == (want["v"] - 27) % 2 == (want["v"] - 37) % 2
        assert o["chain_id"] == (0 if want["v"] < 35 else 1) and o["type"] == 0
        assert o["priority_fee"] == o["gas_price"] and o["sig_status"] == S.OK
        assert (o["al_off"], o["al_len"], o["al_addresses"], o["al_keys"]) == (0, 0, 0, 0)


def test_the_fixtures_refused_blocks(oracle):
    """the 8 "intrinsic gas too low" blocks give exactly PHANT_TX_INTRINSIC_GAS, the 2 "max initcode size exceeded" blocks
    PHANT_TX_INITCODE_SIZE; every transaction of a block without an exception passes every state-free rule ("Transaction without funds"
    needs the sender's balance: no state-free rule sees it)"""
    seen = collections.Counter()
    for raw, want in _fixtures():
        o = T.analyse(oracle, raw["tx"], 1, base_fee=None, block_gas_limit=None)
        err = o["flags"] & T.ERROR_BITS
        exc = want.get("expectException")
        seen[exc] += 1
        if exc == "intrinsic gas too low":
            assert err == T.INTRINSIC_GAS, want["case"]
        elif exc == "max initcode size exceeded":
            assert err == T.INITCODE_SIZE and o["data_len"] > 2 * T.MAX_CODE_SIZE, want["case"]
        else:
            assert err == 0, (want["case"], exc)
    assert seen == {None: 70, "intrinsic gas too low": 8, "max initcode size exceeded": 2, "Transaction without funds": 1}


def test_mainnet_hashes_and_senders(oracle):
    for t, h in zip(S.load_vectors()["mainnet"], MAINNET_HASHES):
        o = T.analyse(oracle, t["tx"], 1, base_fee=1)
        assert o["tx_hash"].hex() == h and o["sender"].hex() == t["sender"] and not o["flags"] & T.ERROR_BITS
    two = T.analyse(oracle, S.load_vectors()["mainnet"][1]["tx"], 1, base_fee=10**9)
    # 02f871 01 83063c38 80 850e58157afa 825ac2 94.. 8789c1870632dbf6 80 c0: priority 0, max fee 0xe58157afa, gas 0x5ac2
    assert (two["type"], two["chain_id"], two["nonce"], two["gas_limit"]) == (2, 1, 0x063C38, 0x5AC2)
    assert int.from_bytes(two["priority_fee"], "big") == 0 and int.from_bytes(two["gas_price"], "big") == 0x0E58157AFA
    assert int.from_bytes(two["effective_gas_price"], "big") == 10**9 and two["intrinsic_gas"] == 21000
    assert int.from_bytes(two["upfront_cost"], "big") == 0x5AC2 * 0x0E58157AFA + 0x89C1870632DBF6


def test_expected_packs_rows_and_first_bad(oracle):
    txs = [S.make_tx(oracle, 3, 0, 1), b"", S.make_tx(oracle, 3, 2, 1, gas=20999)]
    out, first_bad = T.expected(oracle, txs, 1)
    assert first_bad == 1 and len(out["tx_hash"]) == 96 and len(out["flags"]) == 12
    assert out["tx_hash"][32:64] == oracle.keccak256(b"")
    assert int.from_bytes(out["flags"][8:12], "little") == T.INTRINSIC_GAS


def test_the_fast_recovery_is_secp_refs_recovery(oracle):
    z = int.from_bytes(oracle.keccak256(b"a message"), "big")
    cases = []
    for d in (1, 2, 0xC0FFEE, S.N - 1):
        r, s, recid = S.sign(d, z)
        cases += [(z, r, s, recid), (z, *S.high_s_twin(r, s, recid)), (z, r, s, recid ^ 1), (z ^ 1, r, s, recid), (z, r, s, recid | 2), (z, r, s, 4)]
    cases += [(z, 0, 1, 0), (z, 1, 0, 0), (z, S.N, 1, 0), (z, 1, S.N, 1), (z, 5, 5, 0), (z, 6, 7, 1), (0, S.GX, S.GX, 0), (z, S.P - S.N + 1, 1, 2),
              (S.N - 1, 1, 1, 0), (z, S.GX % S.N, 3, 1)]
    # z = s: (-z / r) G + (s / r) R with R = G is the point at infinity
    cases += [(9, S.GX % S.N, 9, S.GY & 1)]
    seen = set()
    for c in cases:
        for flags in (0, S.LOW_S):
            want = S.recover(*c, flags)
            assert T.fast_recover(*c, flags) == want, c
            seen.add(want[0])
    assert seen >= {S.OK, S.BAD_RANGE, S.HIGH_S, S.BAD_RECID, S.NOT_ON_CURVE, S.INFINITY}, seen
