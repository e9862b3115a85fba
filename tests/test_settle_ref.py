"""tests/settle_ref.py, the definition phant_block_settle is checked against, held against answers that owe nothing to it: rows worked
out by hand for every flag and class, and the known answers of tests/golden/fixture_roots.json.gz -- the 8 cases of withdrawals without
transactions, whose `post` and post_state_root the fixtures state, and the case of a transfer behind a withdrawal block."""
from tests import golden
from tests import settle_ref as R

A, B, C = R.account(0, 10**18), R.account(4, 50), R.account(0, 0, R.ABSENT)
CODE = bytes(range(32))


def run(txs, accounts=(A, B, C), wd=(), coinbase=2, fork=R.LONDON, bgl=10**9, base_fee=7):
    return R.define(fork, bgl, base_fee, coinbase, list(txs), [dict(a) for a in accounts], list(wd))


def test_one_transfer_by_hand():
    out, sc = run([R.tx(0, 1, value=1000, price=10)])
    assert out["settle_flags"] == [0] and out["cumulative_gas_used"] == [21000] and out["balance_before"] == [10**18]
    assert out["account_op"] == [R.POST_SET] * 3 and out["nonces_after"] == [1, 4, 0]
    assert out["balances_after"] == [10**18 - 210000 - 1000, 1050, 63000]  # the coinbase gets gas x (price - base fee), the rest burns
    assert sc == {"first_bad": 1, "n_not_plain": 0, "first_not_plain": 1, "block_flags": 0, "n_wd_unknown": 0, "gas_used": 21000}
    assert R.settled(out, sc, 1)


def test_every_flag_and_class_by_hand():
    # UPSTREAM: each source; no event, no gas, zero outputs
    for kw in ({"tx_flags": 0x20}, {"tx_flags": 0x20000}, {"state_flags": R.TXST_SKIPPED}, {"state_flags": 0x4}, {"price": 6}, {"sender_row": R.ROW_NONE},
               {"to_row": R.ROW_NONE}, {"price": 1 << 250, "intrinsic": 1 << 40}):
        out, sc = run([R.tx(**dict({"sender_row": 0, "to_row": 1}, **kw))])
        assert out["settle_flags"] == [R.UPSTREAM] and out["cumulative_gas_used"] == [0] and out["account_op"] == [R.POST_KEEP] * 3, kw
        assert sc["first_bad"] == 0 and sc["gas_used"] == 0 and sc["block_flags"] == 0 and sc["n_not_plain"] == 0
    # NOT_PLAIN: each reason; advisory, counted
    with_code = (A, R.account(1, 0, code_hash=CODE), C)
    for kw, acc in (({"type": 3}, None), ({"type": 4}, None), ({"tx_flags": R.TX_IS_CREATE, "to_row": R.ROW_NONE}, None), ({"state_flags": R.TXST_UNDETERMINED}, None),
                    ({}, with_code), ({"to": bytes(19) + b"\x09"}, None)):
        out, sc = run([R.tx(0, 2), R.tx(**dict({"sender_row": 0, "to_row": 1}, **kw))], acc or (A, B, C))
        assert out["settle_flags"] == [0, R.NOT_PLAIN] and sc["first_bad"] == 2 and sc["n_not_plain"] == 1 and sc["first_not_plain"] == 1, kw
        assert out["nonces_after"][0] == 1 and sc["gas_used"] == 21000 and not R.settled(out, sc, 2)
    # the precompiles of each fork
    for fork, last in ((R.LONDON, 9), (R.CANCUN, 10), (R.PRAGUE, 17)):
        got = [run([R.tx(0, 1, to=bytes(19) + bytes([b]))], fork=fork)[0]["settle_flags"][0] for b in (0, 1, last, last + 1)]
        assert got == [0, R.NOT_PLAIN, R.NOT_PLAIN, 0]
    # GAS_LIMIT: against what the rows before left, not against the block
    out, sc = run([R.tx(0, 1, gas_limit=50000), R.tx(0, 1, gas_limit=79000), R.tx(0, 1, gas_limit=58001)], bgl=100000)
    assert out["settle_flags"] == [0, 0, R.GAS_LIMIT] and out["cumulative_gas_used"] == [21000, 42000, 63000] and sc["first_bad"] == 2
    # the floor of EIP-7623 is what the row uses
    assert run([R.tx(0, 1, floor=30000, gas_limit=30000)])[1]["gas_used"] == 30000
    # BALANCE_SHORT: exact, with the credits that came before; the verdicts behind assume the row was applied
    out, sc = run([R.tx(1, 0, value=50, price=10, gas_limit=21000)])
    assert out["settle_flags"] == [R.BALANCE_SHORT] and out["balance_before"] == [50] and out["account_flags"] == [0, R.ACCT_NEGATIVE, 0]
    assert out["balances_after"][1] == 0 and out["account_op"][1] == R.POST_SET
    out, sc = run([R.tx(0, 1, value=210000), R.tx(1, 0, value=50)])
    assert out["settle_flags"] == [0, 0] and out["balance_before"] == [10**18, 210050] and out["balances_after"][1] == 0 and R.settled(out, sc, 2)
    # block flags and withdrawals
    assert run([R.tx(0, 1)], coinbase=R.ROW_NONE)[1]["block_flags"] == R.COINBASE_UNKNOWN
    assert run([R.tx(0, 1)], (A, B, R.account(status=20)))[1]["block_flags"] == R.COINBASE_UNKNOWN
    out, sc = run([], wd=[(1, 3), (R.ROW_NONE, 1), (2, 0), (2, 0)])
    assert out["wd_flags"] == [0, 1, 0, 0] and sc["n_wd_unknown"] == 1 and out["balances_after"][1] == 50 + 3 * 10**9
    assert out["account_op"] == [R.POST_KEEP, R.POST_SET, R.POST_KEEP]  # nothing for an absent row is nothing
    # EIP-161: present and empty after a touch: deleted; overflow clamps and is flagged
    out, sc = run([], (A, R.account(0, 0), C), wd=[(1, 0)])
    assert out["account_op"][1] == R.POST_DELETE and R.settled(out, sc, 0)
    out, sc = run([], (A, R.account(0, R.M256), C), wd=[(1, 1)])
    assert out["account_flags"][1] == R.ACCT_OVERFLOW and out["balances_after"][1] == R.M256 and not R.settled(out, sc, 0)
    assert R.errors(R.UPSTREAM | R.BALANCE_SHORT | R.NOT_PLAIN) == ["Upstream", "BalanceShort"]


def test_the_withdrawal_fixtures(oracle):
    """pre + credits, with the EIP-161 rule, is `post`, and its root is post_state_root: in exactly 8 cases"""
    fx = golden.fixtures()
    cases = [c for c in fx["cases"] if all(not b["tx_values"] for b in c["blocks"]) and any(b.get("withdrawal_values") for b in c["blocks"])]
    assert len(cases) == 8
    for case in cases:
        addrs, rows = R.fixture_accounts(fx, case, oracle)
        extra = {a["addr"]: a for a in case["pre"]}
        for block in case["blocks"]:
            wd = R.withdrawals_of(block)
            for a, _ in wd:  # an address `pre` lacks: proven absent, as a witness would
                if a not in addrs:
                    addrs.append(a)
                    rows.append(R.account(status=R.ABSENT))
            out, sc = R.define(R.LONDON, 10**9, 7, R.ROW_NONE, [], rows, [(addrs.index(a), g) for a, g in wd])
            assert R.settled(out, sc, 0) and sc["gas_used"] == block["gas_used"] == 0
            after = R.apply(addrs, rows, out)
            addrs, rows = [a for a, _ in after], [r for _, r in after]
        post = {bytes.fromhex(a["addr"]): (a["nonce"], int(a["balance"] or "0", 16)) for a in case["post"]}
        assert {a: (r["nonce"], r["balance"]) for a, r in zip(addrs, rows)} == post, case["name"]
        accounts = [{"addr": a, "nonce": r["nonce"], "balance": r["balance"], "code": bytes.fromhex(fx["codes"][extra[a.hex()]["code"]]) if a.hex() in extra else b"",
                     "storage": {int(k or "0", 16): int(v or "0", 16) for k, v in extra[a.hex()]["storage"].items()} if a.hex() in extra else {}}
                    for a, r in zip(addrs, rows)]
        assert oracle.state_root(accounts).hex() == case["post_state_root"], case["name"]


def test_a_transfer_behind_a_withdrawal_block(oracle):
    """001-fork=Shanghai-tx_after_withdrawals_block: block 1 credits 0x5209 gwei, block 2 is one legacy transfer of nothing to the absent
    0x..0100 at gas price 10^9 under base fee 7"""
    from tests import tx_ref
    fx = golden.fixtures()
    case = next(c for c in fx["cases"] if c["name"] == "001-fork=Shanghai-tx_after_withdrawals_block")
    coinbase, to = bytes.fromhex("2adc25665018aa1fe0e6bc666dac8fc2697ff9ba"), bytes(18) + b"\x01\x00"
    addrs, rows = R.fixture_accounts(fx, case, oracle)
    for a in (coinbase, to):
        if a not in addrs:
            addrs.append(a)
            rows.append(R.account(status=R.ABSENT))
    sender = bytes.fromhex("a94f5374fce5edbc8e2a8697c15331677e6ebf0b")
    out, sc = R.define(R.LONDON, 0x016345785D8A0000, 7, addrs.index(coinbase), [], rows, [(addrs.index(a), g) for a, g in R.withdrawals_of(case["blocks"][0])])
    assert R.settled(out, sc, 0) and out["balances_after"][addrs.index(sender)] == 1 + 0x5209 * 10**9
    after = dict(R.apply(addrs, rows, out))
    rows = [after.get(a, R.account(status=R.ABSENT)) for a in addrs]
    o = tx_ref.analyse(oracle, bytes.fromhex(case["blocks"][1]["tx_values"][0]), 1)
    assert o["sender"] == sender and o["to"] == to and o["flags"] == 0
    price = int.from_bytes(o["gas_price"], "big")
    t = R.tx(addrs.index(sender), addrs.index(to), value=int.from_bytes(o["value"], "big"), price=price, gas_limit=o["gas_limit"], intrinsic=o["intrinsic_gas"], to=to,
             cost=int.from_bytes(o["upfront_cost"], "big"))
    assert (price, t["value"], t["gas_limit"]) == (10**9, 0, 0x5208)
    out, sc = R.define(R.LONDON, 0x016345785D8A0000, 7, addrs.index(coinbase), [t], rows)
    assert R.settled(out, sc, 1) and sc["gas_used"] == case["blocks"][1]["gas_used"] == 0x5208
    after = dict(R.apply(addrs, rows, out))
    assert after[coinbase]["balance"] == 0x1319718811C8 and (after[sender]["nonce"], after[sender]["balance"]) == (1, 0x3B9ACA01) and to not in after
    assert out["account_op"][addrs.index(to)] == R.POST_KEEP
    root = oracle.state_root([{"addr": a, "nonce": r["nonce"], "balance": r["balance"], "code": b"", "storage": {}} for a, r in sorted(after.items())])
    assert root.hex() == case["post_state_root"]
