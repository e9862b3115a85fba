"""tests/txstate_ref.py, the definition phant_block_txs_prestate is checked against, held against rows worked out by hand for every flag
and against what the reference's fixtures state about their own blocks (tests/golden/fixture_roots.json.gz: the accounts before and
after, the raw transactions -- nothing this project computed)."""
from tests import txstate_ref as R

A, B, C_, D = (bytes([k]) * 20 for k in (0xA1, 0xB2, 0xC3, 0xD4))
CODE_HASH = bytes(range(32))
DESIGNATOR = b"\xef\x01\x00" + b"\x77" * 20


def one(fork, txs, accounts, **kw):
    out, first_bad, n_und = R.define(fork, txs, accounts, **kw)
    return out, first_bad, n_und


def test_a_plain_block_by_hand():
    """two senders interleaved, a create, a recipient the witness lacks"""
    accounts = [R.account(A, nonce=5, balance=100), R.account(B, nonce=0, balance=10), R.account(C_, status=R.ABSENT)]
    txs = [R.tx(A, 5, 40, B), R.tx(B, 0, 10, C_), R.tx(A, 6, 60, D), R.tx(A, 7, 1, B, flags=R.TX_IS_CREATE), R.tx(B, 2, 0, A), R.tx(B, 1, 0, A)]
    out, first_bad, n_und = one(R.LONDON, txs, accounts, probes=[C_, D])
    assert out["sender_row"] == [0, 1, 0, 0, 1, 1] and out["to_row"] == [1, 2, R.ROW_NONE, R.ROW_NONE, 0, 0]
    assert out["expected_nonce"] == [5, 0, 6, 7, 1, 2] and out["spent_before"] == [0, 0, 40, 100, 10, 10]
    assert out["state_flags"] == [0, 0, R.TO_UNKNOWN, R.NEEDS_INFLOW, R.NONCE_HIGH, R.NONCE_LOW]
    assert (first_bad, n_und) == (2, 0) and out["sends"] == [3, 3, 0]
    assert out["roles"] == [R.ROLE_SENDER | R.ROLE_RECIPIENT, R.ROLE_SENDER | R.ROLE_RECIPIENT, R.ROLE_RECIPIENT | R.ROLE_PROBE]
    assert out["probe_row"] == [2, R.ROW_NONE]
    assert R.errors(out["state_flags"][4]) == ["NonceHigh"]


def test_every_flag_by_hand():
    acc = lambda **kw: [R.account(A, **kw), R.account(B)]  # noqa: E731
    flags = lambda fork, txs, accounts, **kw: one(fork, txs, accounts, **kw)[0]["state_flags"]  # noqa: E731
    # skipped rows: a bad signature, an undecodable row, a bad v -- no sender, no rank taken
    out, first_bad, _ = one(R.LONDON, [R.tx(A, 0, to=B, sig_status=1), R.tx(A, 0, to=B, flags=R.TX_UNDECODABLE), R.tx(A, 0, to=B, flags=R.TX_BAD_V),
                                        R.tx(A, 0, to=B, flags=R.TX_SIGNATURE), R.tx(A, 0, to=B)], acc())
    assert out["state_flags"] == [R.SKIPPED] * 4 + [0] and out["sender_row"] == [R.ROW_NONE] * 4 + [0] and first_bad == 5 and out["sends"] == [1, 0]
    # the sender: missing, unproven (its row is still reported, it joins no sequence)
    out, first_bad, _ = one(R.LONDON, [R.tx(D, 0, to=B), R.tx(A, 0, to=B), R.tx(A, 0, to=B)], acc(status=17, nonce=9))
    assert out["state_flags"] == [R.SENDER_UNKNOWN] * 3 and out["sender_row"] == [R.ROW_NONE, 0, 0] and out["expected_nonce"] == [0, 0, 0]
    assert first_bad == 0 and out["sends"] == [0, 0] and out["roles"] == [R.ROLE_SENDER, R.ROLE_RECIPIENT]
    # the balance: equal to the need, one below; certain only for the block's first transaction
    assert flags(R.LONDON, [R.tx(A, 0, 7, B)], acc(balance=7)) == [0]
    assert flags(R.LONDON, [R.tx(A, 0, 7, B)], acc(balance=6)) == [R.NEEDS_INFLOW | R.BALANCE_SHORT]
    assert flags(R.LONDON, [R.tx(B, 0, 0, A), R.tx(A, 0, 7, B)], acc(balance=6)) == [0, R.NEEDS_INFLOW]
    # EIP-3607 at each fork: code the witness carries, code it lacks, a designator
    plain, lacking = acc(code_hash=CODE_HASH, code_index=0), acc(code_hash=CODE_HASH)
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        assert flags(fork, [R.tx(A, 0, to=B)], plain, codes=[b"\x60\x00"]) == [R.NOT_EOA]
        assert flags(fork, [R.tx(A, 0, to=B)], lacking) == [R.CODE_MISSING if fork == R.PRAGUE else R.NOT_EOA]
        assert flags(fork, [R.tx(A, 3, 99, B)], plain, codes=[DESIGNATOR]) == [R.UNDETERMINED if fork == R.PRAGUE else R.NOT_EOA | R.NONCE_HIGH | R.NEEDS_INFLOW | R.BALANCE_SHORT]
    for code in (DESIGNATOR[:22], DESIGNATOR + b"\x00", b"\xef\x01\x01" + b"\x77" * 20):
        assert flags(R.PRAGUE, [R.tx(A, 0, to=B)], plain, codes=[code]) == [R.NOT_EOA]
    # an authority: of an earlier transaction, of the same one, of a skipped one, of a tuple that failed
    txs = [R.tx(B, 0, to=A), R.tx(A, 5, to=B), R.tx(A, 6, to=B)]
    for fork in (R.LONDON, R.PRAGUE):
        und = R.UNDETERMINED if fork == R.PRAGUE else R.NONCE_HIGH
        assert one(fork, txs, acc(), auth_first=[0, 1, 1, 1], auths=[(A, 0)]) == (
            {**one(fork, txs, acc())[0], "state_flags": [0, und, und], "roles": [7, 3]}, 3 if fork == R.PRAGUE else 1, 2 if fork == R.PRAGUE else 0)
    assert flags(R.PRAGUE, txs, acc(), auth_first=[0, 0, 1, 1], auths=[(A, 0)]) == [0, R.NONCE_HIGH, R.UNDETERMINED]
    assert flags(R.PRAGUE, txs, acc(), auth_first=[0, 1, 1, 1], auths=[(A, 3)]) == [0, R.NONCE_HIGH, R.NONCE_HIGH]
    skipped = [R.tx(B, 0, to=A, sig_status=2)] + txs[1:]
    assert flags(R.PRAGUE, skipped, acc(), auth_first=[0, 1, 1, 1], auths=[(A, 0)]) == [R.SKIPPED, R.NONCE_HIGH, R.NONCE_HIGH]


def test_wide_sums_by_hand():
    top = R.M256
    accounts = [R.account(A, nonce=R.M64 - 1, balance=top)]
    txs = [R.tx(A, R.M64 - 1, top, A), R.tx(A, R.M64, 1, A), R.tx(A, R.M64, 1 << 256, A), R.tx(A, R.M64, 0, A)]
    out, first_bad, _ = one(R.LONDON, txs, accounts)
    assert out["expected_nonce"] == [R.M64 - 1, R.M64, R.M64, R.M64]  # saturating
    assert out["spent_before"] == [0, top, top, top]
    assert out["state_flags"] == [0, R.NEEDS_INFLOW, R.NEEDS_INFLOW | R.SPENT_SATURATED, R.NEEDS_INFLOW | R.SPENT_SATURATED] and first_bad == 4
    assert txs[2]["flags"] == R.TX_COST_OVERFLOW and txs[2]["cost"] == 0
    exp, _, _ = R.expected(R.LONDON, txs, accounts)
    assert exp["spent_before"][32:64] == b"\xff" * 32 and len(exp["expected_nonce"]) == 32 and len(exp["roles"]) == 1


def test_duplicate_rows_resolve_to_the_lowest():
    accounts = [R.account(B), R.account(A, nonce=1), R.account(A, nonce=9, status=17)]
    out, _, _ = one(R.LONDON, [R.tx(A, 1, to=A)], accounts, probes=[A])
    assert out["sender_row"] == [1] and out["to_row"] == [1] and out["probe_row"] == [1] and out["state_flags"] == [0] and out["sends"] == [0, 1, 0]


def test_the_fixtures_blocks_are_a_known_answer(oracle):
    got = R.walk_fixtures(oracle, lambda raws: R.rows_from_analysis(oracle, raws), lambda txs, accounts, codes: R.define(R.LONDON, txs, accounts, codes)[:2])
    assert got == R.FIXTURE_ANSWER
