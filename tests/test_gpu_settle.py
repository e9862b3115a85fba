"""A block of plain transfers settled on the device (phant_block_settle, phant_block_settle_dev, phant_amd.blockchain) against
tests/settle_ref.py, which defines every output.  Every comparison is exact, in the host form and in the device form, every buffer
between guards of 0xEE.  tests/test_emu_settle.py runs the same bodies over the kernel sources compiled for the host, at the sizes
tests/suite.py gives it."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import settle_ref as R
from tests import suite

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1
ALL = tuple(name for name, _, _, _ in R.OUTPUTS)
M64, M256 = R.M64, R.M256
CODE_HASH = bytes(range(1, 33))
BGL = 10**12


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def addr(k):
    """address number k: bytes nobody chose"""
    return hashlib.sha256(b"settle" + int(k).to_bytes(8, "big")).digest()[:20]


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_settle_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, dev, base_fee, txs, accounts, withdrawals=(), floor=True):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        self.counts = {"n": len(txs), "n_accounts": len(accounts), "n_wd": len(withdrawals)}
        self.arrays = {k: None if a is None else self._up(a) for k, a in R.inputs(base_fee, txs, accounts, withdrawals, floor).items()}

    def _up(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size == 0:
            a = np.zeros(8, np.uint8)  # (a pointer that is not NULL, to nothing the call may read)
        return self.torch.from_numpy(a.copy()).cuda() if self.dev else a.copy()

    def _ptr(self, x):
        return None if x is None else x.data_ptr() if self.dev else x.ctypes.data

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, fork, block_gas_limit, coinbase_row, want=None, guard=64, null=(), counts=None, sizes=None, reserved=0, skew=None):
        """-> (rc, {output: bytes, (output, "guards"): bool}, {scalar: value}); every buffer has `guard` bytes of 0xEE in front of and
        behind its rows.  null: inputs passed as NULL; counts: counts other than the arrays'; skew: {array: bytes its pointer moves up}"""
        L = self.L
        want = ALL if want is None else want
        cnt = dict(self.counts, **(counts or {}))
        ptr = lambda k: None if k in null or self.arrays[k] is None else self._ptr(self.arrays[k]) + (skew or {}).get(k, 0)  # noqa: E731
        arg = L.PhantSettleIn(C.sizeof(L.PhantSettleIn), fork, cnt["n"], cnt["n_accounts"], cnt["n_wd"], coinbase_row, (C.c_uint32 * 2)(reserved, 0),
                              block_gas_limit, *[ptr(k) for k in L.SETTLE_INPUTS])
        size = {name: np.dtype(dt).itemsize * k * cnt[rows] for name, dt, k, rows in R.OUTPUTS if name in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantSettleOut(C.sizeof(L.PhantSettleOut), 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE,
                               *[self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None for k in ALL])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_settle_dev if self.dev else ctx._lib.phant_block_settle
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        return rc, got, {k: int(getattr(out, k)) for k in R.SCALARS}


def _first_difference(name, a, b):
    width = {n: np.dtype(dt).itemsize * k for n, dt, k, _ in R.OUTPUTS}[name]
    for i in range(0, max(len(a), len(b)), width):
        if a[i:i + width] != b[i:i + width]:
            return i // width, a[i:i + width].hex(), b[i:i + width].hex()
    return None


def check(P, fork, txs, accounts, withdrawals=(), coinbase_row=R.ROW_NONE, base_fee=7, block_gas_limit=BGL, forms=(False, True), want=None, floor=True):
    """every answer of the call against the definition, in both forms -> (the definition's lists, its scalars)"""
    if not floor:
        txs = [dict(t, floor=0) for t in txs]
    exp, scalars = R.expected(fork, block_gas_limit, base_fee, coinbase_row, txs, accounts, withdrawals)
    ctx = _ctx(P)
    for dev in forms:
        rc, got, sc = Raw(P, dev, base_fee, txs, accounts, withdrawals, floor).call(ctx, fork, block_gas_limit, coinbase_row, want)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert sc == scalars, (dev, sc, scalars)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(k, got[k], exp[k]))
    return R.define(fork, block_gas_limit, base_fee, coinbase_row, txs, accounts, withdrawals)


# ------------------------------------------------------------------------------------------------------ blocks by arrangement
def make_accounts(na, rng, rich=True):
    """na rows: funded accounts, every ninth proven absent, every eleventh a contract, every thirteenth present and empty"""
    rows = []
    for j in range(na):
        if j % 9 == 8:
            rows.append(R.account(status=R.ABSENT))
        elif j % 13 == 12:
            rows.append(R.account())
        else:
            rows.append(R.account(int(rng.integers(0, 1000)), int(rng.integers(1, 1 << 62)) << (100 if rich else int(rng.integers(0, 30))),
                                  code_hash=CODE_HASH if j % 11 == 10 else R.EMPTY_CODE_HASH))
    return rows


def senders_of(accounts):
    return [j for j, a in enumerate(accounts) if a["status"] == R.PRESENT and a["code_hash"] == R.EMPTY_CODE_HASH and a["balance"]]


def make_block(n, accounts, arrangement, rng, mixed=False):
    """n transfers whose senders are arranged as asked; recipients anywhere.  mixed: every class and every upstream reason among them"""
    ok = senders_of(accounts)
    na = len(accounts)
    txs = []
    for i in range(n):
        s = ok[i % len(ok)] if arrangement == "distinct" else ok[len(ok) // 2] if arrangement == "one" else ok[int(rng.integers(0, len(ok)))]
        r = int(rng.integers(0, na))
        price = 7 + int(rng.integers(0, 1000))
        t = R.tx(s, r, value=int(rng.integers(0, 1 << 60)), price=price, gas_limit=21000 + int(rng.integers(0, 5000)),
                 intrinsic=21000 + int(rng.integers(0, 400)), floor=int(rng.integers(0, 2)) * (21000 + int(rng.integers(0, 800))), to=addr(10**6 + r))
        if mixed:
            k = i % 23
            if k == 3:
                t["type"] = 3 + i % 2
            elif k == 5:
                t.update(tx_flags=R.TX_IS_CREATE, to_row=R.ROW_NONE)
            elif k == 7:
                t["state_flags"] = R.TXST_UNDETERMINED
            elif k == 9:
                t["to"] = bytes(19) + bytes([1 + i % 0x12])
            elif k == 11:
                t["tx_flags"] = 1 << (i % 19) if i % 19 != 11 else 0x20
            elif k == 13:
                t["state_flags"] = [R.TXST_SKIPPED, 0x4, 0x10, 0x2][i % 4]
            elif k == 15:
                t["price"] = 6
            elif k == 17:
                t["cost"] = accounts[s]["balance"] * 3  # short of balance
            elif k == 19:
                t["gas_limit"] = BGL
        txs.append(t)
    return txs


def test_event_counts_around_a_tile(P):
    """3 n + n_wd = 255, 256, 257 and 513 event slots: both sides of a tile of the scan, in both arrangements"""
    rng = np.random.default_rng(1)
    for events in (255, 256, 257, 513):
        for n_wd in (0, 1, 2):
            if (events - n_wd) % 3:
                continue
            n = (events - n_wd) // 3
            accounts = make_accounts(40, rng)
            for arrangement in ("distinct", "one"):
                txs = make_block(n, accounts, arrangement, rng)
                out, sc = check(P, R.PRAGUE, txs, accounts, [(int(rng.integers(0, 40)), int(rng.integers(0, 1 << 40))) for _ in range(n_wd)], coinbase_row=3)
                assert sc["gas_used"] > 21000 * n // 2 and sc["n_not_plain"] > 0


def test_a_segment_across_three_tiles(P):
    """the coinbase of 200 plain rows holds 200 events and one sender of 300 holds 300 (+ its self-transfers): three tiles each"""
    rng = np.random.default_rng(2)
    accounts = [R.account(5, 10**30) for _ in range(suite.scale(210, 70))] + [R.account(0, 0, R.ABSENT)]
    n = len(accounts) - 1
    txs = [R.tx(i % n, (i * 7 + 1) % n, value=i, price=9 + i % 5) for i in range(suite.scale(200, 90))]
    out, sc = check(P, R.LONDON, txs, accounts, coinbase_row=n)
    assert R.settled(out, sc, len(txs)) and out["account_op"][n] == R.POST_SET and out["balances_after"][n] == sum(21000 * (2 + i % 5) for i in range(len(txs)))
    m = suite.scale(300, 100)
    txs = [R.tx(4, 4 if i % 10 == 0 else 1 + i % 3, value=10**18 + i, price=7 + i % 3) for i in range(m)]
    out, sc = check(P, R.LONDON, txs, accounts, coinbase_row=4)
    assert R.settled(out, sc, m) and out["nonces_after"][4] == 5 + m
    # a balance that runs out in the middle of the sequence: exactly one row is short, the rows behind it assume it was applied
    accounts[4]["balance"] = sum((t["value"] if t["to_row"] != 4 else 0) + 21000 * t["price"] for t in txs[:m // 2]) + txs[m // 2]["cost"] - 1
    out, sc = check(P, R.LONDON, txs, accounts, coinbase_row=0)
    assert sc["first_bad"] == m // 2 and out["settle_flags"][m // 2 - 1] == 0 and out["account_flags"][4] == R.ACCT_NEGATIVE


def test_no_transactions_and_no_withdrawals(P):
    rng = np.random.default_rng(3)
    accounts = make_accounts(30, rng)
    wd = [(int(rng.integers(0, 30)), int(rng.integers(0, 1 << 50))) for _ in range(suite.scale(300, 40))] + [(8, 0), (R.ROW_NONE, 5)]
    out, sc = check(P, R.CANCUN, [], accounts, wd, coinbase_row=2)
    assert sc == {"first_bad": 0, "n_not_plain": 0, "first_not_plain": 0, "block_flags": 0, "n_wd_unknown": 1, "gas_used": 0}
    assert out["account_op"][2] == R.POST_KEEP or any(w[0] == 2 for w in wd)
    out, sc = check(P, R.CANCUN, make_block(50, accounts, "any", rng), accounts, (), coinbase_row=2)
    check(P, R.CANCUN, [], accounts, ())
    check(P, R.CANCUN, [], [], ())
    check(P, R.CANCUN, [], [], [(R.ROW_NONE, 1)])


@pytest.mark.parametrize("na", [255, 256, 257])
def test_table_sizes_around_a_key_byte(P, na):
    """n_accounts = 255: the sort key (0 .. n_accounts) fits one byte; 256 and 257: two"""
    rng = np.random.default_rng(na)
    accounts = make_accounts(na, rng)
    txs = make_block(suite.scale(400, 60), accounts, "any", rng, mixed=True)
    txs[0].update(sender_row=senders_of(accounts)[-1], to_row=na - 1)
    txs[1].update(sender_row=0, to_row=0)
    out, sc = check(P, R.PRAGUE, txs, accounts, [(na - 1, 3), (0, 4)], coinbase_row=na - 2)
    assert sc["n_not_plain"] > 3 and sc["first_bad"] < len(txs)


def test_coincidences(P):
    """self-transfer; sender = coinbase; recipient = coinbase; a withdrawal to a sender; withdrawals of zero to an absent row (stays
    absent: KEEP) and to a present empty row (DELETE); a recipient of value 0 that is present and empty (DELETE); a sender emptied to
    nonce 1 (SET)"""
    accounts = [R.account(0, 10**20), R.account(3, 10**20), R.account(0, 0, R.ABSENT), R.account(0, 0), R.account(0, 0), R.account(0, 0, R.ABSENT),
                R.account(0, 21000 * 10 + 5), R.account(0, 0, R.ABSENT), R.account(7, 1)]
    txs = [R.tx(0, 0, value=10**19),                 # self-transfer
           R.tx(1, 0, value=5, price=12),            # the sender is the coinbase
           R.tx(0, 1, value=6),                      # the recipient is the coinbase
           R.tx(0, 4, value=0),                      # a present empty recipient of nothing: deleted
           R.tx(0, 5, value=0),                      # an absent recipient of nothing: stays absent
           R.tx(6, 7, value=5, price=10),            # emptied to the last wei: nonce 1 keeps it
           R.tx(0, 2, value=1)]                      # an absent recipient of one wei: created
    wd = [(0, 3), (2, 0), (3, 0), (8, 10)]
    out, sc = check(P, R.LONDON, txs, accounts, wd, coinbase_row=1)
    assert R.settled(out, sc, len(txs))
    assert out["account_op"] == [R.POST_SET, R.POST_SET, R.POST_SET, R.POST_DELETE, R.POST_DELETE, R.POST_KEEP, R.POST_SET, R.POST_SET, R.POST_SET]
    assert out["balances_after"][6] == 0 and out["nonces_after"][6] == 1 and out["balances_after"][7] == 5 and out["balances_after"][8] == 1 + 10 * R.GWEI
    # the coinbase's credit of transaction 0 (time 1) precedes its own debit (time 2)
    out2, _ = check(P, R.LONDON, txs[:2], accounts, (), coinbase_row=1)
    assert out2["balance_before"][1] == 10**20 + 21000 * 3
    # a withdrawal to a sender cannot fund it: withdrawals come last
    out3, sc3 = check(P, R.LONDON, [R.tx(3, 0, value=1)], accounts, [(3, 10**9)], coinbase_row=1)
    assert sc3["first_bad"] == 0 and out3["settle_flags"] == [R.BALANCE_SHORT] and out3["account_flags"][3] == 0


def test_a_balance_that_an_earlier_credit_covers(P):
    """the case PHANT_TXST_NEEDS_INFLOW leaves open: B cannot pay unless A's transfer came first"""
    accounts = [R.account(0, 10**20), R.account(0, 5), R.account(0, 0, R.ABSENT)]
    need = 21000 * 10 + 1000
    a_pays, b_pays = R.tx(0, 1, value=need - 5), R.tx(1, 2, value=1000)
    out, sc = check(P, R.LONDON, [a_pays, b_pays], accounts, coinbase_row=2)
    assert R.settled(out, sc, 2) and out["balance_before"][1] == need and out["balances_after"][1] == 0
    out, sc = check(P, R.LONDON, [b_pays, a_pays], accounts, coinbase_row=2)
    assert sc["first_bad"] == 0 and out["settle_flags"] == [R.BALANCE_SHORT, 0] and out["account_flags"][1] == 0
    out, sc = check(P, R.LONDON, [dict(a_pays, value=need - 6), b_pays], accounts, coinbase_row=2)
    assert sc["first_bad"] == 1 and out["account_flags"][1] == R.ACCT_NEGATIVE and out["balances_after"][1] == 0


def test_values_near_the_ends(P):
    """balances and values near 2^256: a credit that overflows a row (clamped, flagged), a debit whose cost lies (negative, flagged),
    ff..ff in every dword of a value (a carry or borrow crosses each boundary), gas and nonces at 2^64"""
    accounts = [R.account(0, M256), R.account(M64, M256 - 10), R.account(0, 0, R.ABSENT)]
    out, sc = check(P, R.LONDON, [R.tx(0, 1, value=11, price=8, cost=0)], accounts, coinbase_row=2)
    assert out["account_flags"] == [0, R.ACCT_OVERFLOW, 0] and out["balances_after"][1] == M256 and not R.settled(out, sc, 1)
    out, sc = check(P, R.LONDON, [R.tx(1, 0, value=1, price=8, cost=0), R.tx(1, 2, value=M256 - 21000 * 8, price=8, cost=0)], accounts, coinbase_row=2)
    assert out["account_flags"] == [R.ACCT_OVERFLOW, R.ACCT_NEGATIVE, 0] and out["nonces_after"][1] == M64 and sc["first_bad"] == 2
    for k in range(8):
        ones = 0xFFFFFFFF << (32 * k)
        accounts = [R.account(0, min(2 * ones + 21000 * 20 + 7, M256)), R.account(0, 21000 * 10), R.account(0, 0)]
        txs = [R.tx(0, 1, value=ones if k < 7 else ones >> 1, cost=0), R.tx(1, 2, value=ones if k < 7 else ones >> 1, cost=0), R.tx(0, 2, value=7, cost=0)]
        out, sc = check(P, R.LONDON, txs, accounts, coinbase_row=2)
        assert R.settled(out, sc, 3) == (True), k
    # prices of 2^255, gas_used beyond 2^32, a cumulative gas that saturates; a charge beyond 2^256 - 1 is UPSTREAM
    big = R.tx(0, 1, value=0, price=1 << 255, gas_limit=M64, intrinsic=1, cost=0)
    out, sc = check(P, R.LONDON, [big, dict(big, intrinsic=2), dict(big, intrinsic=M64 - 1, price=1 << 190), dict(big, intrinsic=5, price=9)],
                    [R.account(0, M256), R.account(0, 0)], coinbase_row=1, block_gas_limit=M64)
    assert out["settle_flags"] == [0, R.UPSTREAM, R.GAS_LIMIT, R.GAS_LIMIT] and out["cumulative_gas_used"] == [1, 0, M64, M64] and sc["gas_used"] == M64


def test_gas_limit_at_the_boundary(P):
    accounts = [R.account(0, 10**30), R.account(0, 0)]
    txs = [R.tx(0, 1, gas_limit=30000, floor=22000), R.tx(0, 1, gas_limit=30000), R.tx(0, 1, gas_limit=21000)]
    for bgl, flags in ((22000 + 21000 + 21000, [0, 0, 0]), (22000 + 21000 + 20999, [0, 0, R.GAS_LIMIT]), (22000 + 29999, [0, R.GAS_LIMIT, R.GAS_LIMIT]),
                       (29999, [R.GAS_LIMIT] * 3), (30000, [0, R.GAS_LIMIT, R.GAS_LIMIT])):
        out, sc = check(P, R.PRAGUE, txs, accounts, coinbase_row=1, block_gas_limit=bgl)
        assert out["settle_flags"] == flags and out["cumulative_gas_used"] == [22000, 43000, 64000], bgl
    out, _ = check(P, R.PRAGUE, txs, accounts, coinbase_row=1, block_gas_limit=10**9, floor=False)
    assert out["cumulative_gas_used"] == [21000, 42000, 63000]


def test_classes(P):
    """every class and every reason alone, at each fork; the precompile range of each fork"""
    acc = [R.account(0, 10**20), R.account(0, 0), R.account(1, 0, code_hash=CODE_HASH), R.account(0, 0, status=20)]
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        one = lambda **kw: check(P, fork, [R.tx(0, 1), R.tx(**dict({"sender_row": 0, "to_row": 1}, **kw))], acc, coinbase_row=1, forms=suite.scale((False, True), (False,)))[0]["settle_flags"][1]  # noqa: E731
        assert one() == 0
        for bit in list(range(11)) + list(range(12, 19)):
            assert one(tx_flags=1 << bit) == R.UPSTREAM, bit
        assert one(tx_flags=1 << 19) == 0
        for f in (R.TXST_SKIPPED, 1, 2, 4, 8, 0x10, 0x20, 0x40):
            assert one(state_flags=f) == R.UPSTREAM, f
        assert one(state_flags=0x400 | 0x800) == 0  # NEEDS_INFLOW, SPENT_SATURATED: advisory, and answered here exactly
        assert one(price=6) == R.UPSTREAM and one(price=7) == 0
        assert one(type=1) == 0 and one(type=2) == 0 and one(type=3) == R.NOT_PLAIN and one(type=4) == R.NOT_PLAIN
        assert one(tx_flags=R.TX_IS_CREATE, to_row=R.ROW_NONE) == R.NOT_PLAIN
        assert one(state_flags=R.TXST_UNDETERMINED) == R.NOT_PLAIN
        assert one(to_row=2) == R.NOT_PLAIN
        last = R.LAST_PRECOMPILE[fork]
        assert [one(to=bytes(19) + bytes([b])) for b in (0, 1, last, last + 1)] == [0, R.NOT_PLAIN, R.NOT_PLAIN, 0]
        assert one(to=bytes([1]) + bytes(18) + bytes([1])) == 0 and one(to=bytes(18) + bytes([1, 1])) == 0
    out, sc = check(P, R.LONDON, [R.tx(0, 1)], acc, coinbase_row=3)
    assert sc["block_flags"] == R.COINBASE_UNKNOWN
    assert check(P, R.LONDON, [R.tx(0, 1)], acc)[1]["block_flags"] == R.COINBASE_UNKNOWN
    assert check(P, R.LONDON, [R.tx(0, 1, type=3)], acc)[1]["block_flags"] == 0  # no plain row: nobody asks for the coinbase
    out, sc = check(P, R.LONDON, [], acc, [(3, 1), (1, 1), (R.ROW_NONE, 1)])
    assert out["wd_flags"] == [1, 0, 1] and sc["n_wd_unknown"] == 2


def test_random_blocks_at_each_fork(P):
    rng = np.random.default_rng(23)
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        for n, na, nw in suite.scale(((40, 30, 3), (300, 120, 16), (1500, 900, 40), (2600, 3000, 0)), ((40, 30, 3), (150, 300, 9))):
            accounts = make_accounts(na, rng, rich=False)
            txs = make_block(n, accounts, "any", rng, mixed=True)
            wd = [(int(rng.integers(0, na)) if k % 5 else R.ROW_NONE, int(rng.integers(0, 1 << 44))) for k in range(nw)]
            empty = [j for j, a in enumerate(accounts) if a["status"] == R.PRESENT and not a["balance"]][:2]
            txs = [dict(t, to_row=0) if t["to_row"] in empty else t for t in txs]
            wd += [(j, 0) for j in empty]  # touched and still empty: deleted
            out, sc = check(P, fork, txs, accounts, wd, coinbase_row=int(rng.integers(0, na)), block_gas_limit=21500 * n)
            flags = set(out["settle_flags"])
            assert n < 100 or {0, R.UPSTREAM, R.NOT_PLAIN, R.BALANCE_SHORT, R.GAS_LIMIT} <= flags | {f & ~R.BALANCE_SHORT for f in flags}, flags
            assert len(set(out["account_op"])) == 3 or n < 100


def test_subsets_of_the_outputs(P):
    """each output alone, each left out, none: the span the host form fetches ends at every position"""
    rng = np.random.default_rng(5)
    accounts = make_accounts(40, rng)
    txs = make_block(70, accounts, "any", rng, mixed=True)
    wd = [(3, 5), (8, 0)]
    exp, scalars = R.expected(R.PRAGUE, BGL, 7, 2, txs, accounts, wd)
    ctx = _ctx(P)
    for dev in (False, True):
        raw = Raw(P, dev, 7, txs, accounts, wd)
        for want in [()] + [(k,) for k in ALL] + [tuple(x for x in ALL if x != k) for k in ALL]:
            rc, got, sc = raw.call(ctx, R.PRAGUE, BGL, 2, want)
            assert rc == OK and sc == scalars, (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)


def test_a_call_beyond_the_pinned_stage(P):
    """60 000 pre-state rows (73 input bytes and 74 output bytes each) against 64 transactions: inputs and outputs both end beyond the
    8 MiB stage and cross the bus array by array.  Row for row against the definition, in both forms."""
    rng = np.random.default_rng(41)
    na = 60000
    accounts = make_accounts(na, rng)
    txs = make_block(64, accounts, "any", rng)
    in_bytes = sum(a.nbytes for a in R.inputs(7, txs, accounts).values())
    assert in_bytes > 4 << 20 and 74 * na + in_bytes > 8 << 20
    out, sc = check(P, R.LONDON, txs, accounts, [(na - 1, 9)], coinbase_row=na // 2)
    assert sc["gas_used"] > 0


def test_both_scans_beyond_one_chunk_of_aggregates(P):
    """65 600 plain transfers of distinct senders that all pay ONE coinbase, which also sends, and 10 withdrawals against 2 048 rows:
    196 810 events in 769 tiles, so the aggregate pass over the events runs four chunks of 256 tiles, and 257 gas tiles, so the second
    workgroup's range starts behind the events' and carries into a second chunk.  The coinbase's segment begins inside the first chunk and
    ends inside the last: its running balance crosses every chunk boundary.  Row for row against the definition, in both forms."""
    rng = np.random.default_rng(65600)
    n, na = 65600, 2048
    accounts = make_accounts(na, rng)
    ok = senders_of(accounts)
    c = ok[-2]
    txs = [dict(t, to_row=c) for t in make_block(n, accounts, "distinct", rng)]
    for i, t in enumerate(txs):
        if i % 23 == 17:
            t["cost"] = accounts[t["sender_row"]]["balance"] * 3  # short of balance
        elif i % 23 == 19:
            t["gas_limit"] = BGL
    wd = [(ok[k], int(rng.integers(0, 1 << 40))) for k in range(10)]
    events, chunk = 3 * n + len(wd), 256 * 256
    assert (events + 255) // 256 == 769 and (n + 255) // 256 == 257
    before = sum(t["sender_row"] < c for t in txs) + sum(r < c for r, _ in wd)  # the sorted slots in front of the coinbase's segment
    segment = 2 * n + sum(t["sender_row"] == c for t in txs) + sum(r == c for r, _ in wd)
    assert before < chunk and before + segment > 3 * chunk
    out, sc = check(P, R.PRAGUE, txs, accounts, wd, coinbase_row=c)
    assert sc["n_not_plain"] == 0 and sc["gas_used"] > 21000 * n
    assert {0, R.GAS_LIMIT, R.BALANCE_SHORT} <= set(out["settle_flags"]) and out["nonces_after"][c] > accounts[c]["nonce"]


def test_refused_arguments(P):
    """one refusal per rule of the header, in both forms; nothing is written"""
    rng = np.random.default_rng(6)
    accounts = make_accounts(12, rng)
    txs = make_block(20, accounts, "any", rng)
    wd = [(1, 5), (2, 6)]
    ctx = _ctx(P)

    def refused(dev, t=txs, w=wd, coinbase_row=1, fork=R.PRAGUE, **kw):
        rc, got, sc = Raw(P, dev, 7, t, accounts, w).call(ctx, fork, BGL, coinbase_row, **kw)
        assert rc == E_INVALID_ARG, (dev, kw, rc)
        assert all((np.frombuffer(got[k], np.uint8) == 0xEE).all() for k in ALL), (dev, kw)
        assert ctx._lib.phant_last_error(ctx.handle)

    for dev in (False, True):
        for col in ("sender_row", "to_row"):
            for bad in (12, 0xFFFFFFFE):
                refused(dev, t=[dict(x, **{col: bad}) if i == 17 else x for i, x in enumerate(txs)])  # a row index beyond the table
        refused(dev, w=[(1, 5), (12, 6)])
        refused(dev, coinbase_row=12)
        refused(dev, fork=3)
        refused(dev, reserved=1)
        refused(dev, sizes=(8, 8))
        for name in R.inputs(7, txs, accounts, wd):
            if name != "floor_gas":
                refused(dev, null=(name,))                                                # a NULL input whose count is not zero
        rc, _, _ = Raw(P, dev, 7, txs, accounts, wd).call(ctx, R.PRAGUE, BGL, 1, null=("floor_gas",))
        assert rc == OK
        rc, _, _ = Raw(P, dev, 7, txs, accounts, ()).call(ctx, R.PRAGUE, BGL, R.ROW_NONE, null=("wd_row", "wd_amount_gwei"))
        assert rc == OK
    refused(True, skew={"gas_limit": 4})                                                  # device form: a misaligned array
    refused(True, skew={"settle_flags": 2})


# ------------------------------------------------------------------------------------------------ through phant_amd.blockchain
def _witness(P, oracle, state, keys, may_remove=()):
    """state: address -> {nonce, balance[, code, storage]}"""
    from phant_amd.state import AccountState
    from phant_amd.stateless import build_witness
    return build_witness([AccountState(addr=a, nonce=r["nonce"], balance=r["balance"], code=r.get("code", b""), storage=r.get("storage", {}))
                          for a, r in sorted(state.items())], keys, may_remove)


def _oracle_root(oracle, state):
    return oracle.state_root([{"addr": a, "nonce": r["nonce"], "balance": r["balance"], "code": r.get("code", b""), "storage": r.get("storage", {})}
                              for a, r in sorted(state.items())])


def _applied(state, info, s):
    """the state after a block: what the settlement's account_op / nonces_after / balances_after say"""
    now = {a: dict(r) for a, r in state.items()}
    for j, a in enumerate(bytes(x) for x in info["addresses"]):
        if s.account_op[j] == R.POST_SET:
            now[a] = dict(now.get(a, {}), nonce=int(s.nonces_after[j]), balance=int.from_bytes(s.balances_after[j].tobytes(), "big"))
        elif s.account_op[j] == R.POST_DELETE:
            del now[a]
    return now


def test_the_fixtures_through_run_transfer_block(P, oracle):
    """The 8 fixture cases of withdrawals without transactions, and the case of a transfer behind a withdrawal block: raw bytes and a
    witness cut from the state in, the fixture's gasUsed, receipt trie and post_state_root out"""
    from phant_amd import blockchain as B
    from phant_amd.types import transaction as TX
    from tests import golden
    fx = golden.fixtures()
    header = {"coinbase": bytes.fromhex("2adc25665018aa1fe0e6bc666dac8fc2697ff9ba"), "base_fee": 7, "gas_limit": 0x016345785D8A0000}
    special = "001-fork=Shanghai-tx_after_withdrawals_block"
    cases = [c for c in fx["cases"] if any(b.get("withdrawal_values") for b in c["blocks"]) and (all(not b["tx_values"] for b in c["blocks"]) or c["name"] == special)]
    assert len(cases) == 9
    for case in suite.scale(cases, [c for c in cases if c["name"] == special] + cases[:2]):
        state = {a["addr"]: {k: a[k] for k in ("nonce", "balance", "code", "storage")} for a in golden.accounts_of(case["pre"], fx["codes"])}
        for block in case["blocks"]:
            wd = R.withdrawals_of(block)
            raws = [bytes.fromhex(t) for t in block["tx_values"]]
            bt = TX.block_transactions(raws, 1, fork=TX.FORK_LONDON)
            keys = list(dict.fromkeys([header["coinbase"]] + [a for a, _ in wd] + [bt.sender[i].tobytes() for i in range(bt.n)] + [bt.to[i].tobytes() for i in range(bt.n)]))
            w = _witness(P, oracle, state, keys, may_remove=keys)
            r = B.run_transfer_block(raws, wd, header, w, w.state_root, 1, TX.FORK_LONDON)
            assert r.gas_used == block["gas_used"] and r.settlement.settled and r.receipts_root.hex() == block["receipt_trie"]
            state = _applied(state, w.info(), r.settlement)
            assert r.state_root == _oracle_root(oracle, state)
            w.close()
        assert r.state_root.hex() == case["post_state_root"], case["name"]
        if case["name"] == special:
            sender = state[bytes.fromhex("a94f5374fce5edbc8e2a8697c15331677e6ebf0b")]
            assert state[header["coinbase"]]["balance"] == 0x1319718811C8 and (sender["nonce"], sender["balance"]) == (1, 0x3B9ACA01)
            assert bytes(18) + b"\x01\x00" not in state


def test_a_synthetic_block_end_to_end(P, oracle):
    """about 300 signed transfers over about 120 accounts, 10 withdrawals, one account emptied by nothing (deleted): the state root and
    the receipts root against the oracle over the definition's accounts"""
    from phant_amd import blockchain as B
    from phant_amd.types import transaction as TX
    from tests import receipts_ref, secp_ref as S
    rng = np.random.default_rng(77)
    na, n = suite.scale((120, 300), (24, 40))
    keys = [int.from_bytes(hashlib.sha256(b"key" + bytes([k])).digest(), "big") % (S.N - 1) + 1 for k in range(na)]
    addrs = [S.address(oracle, S.mul(k, S.G)) for k in keys]
    state = {a: {"nonce": int(rng.integers(0, 50)), "balance": 10**21 + int(rng.integers(0, 10**18))} for a in addrs}
    empty, fresh, coinbase = addr(1), addr(2), addr(3)
    state[empty] = {"nonce": 0, "balance": 0}
    raws, sent, expect = [], {}, []
    for i in range(n):
        k = int(rng.integers(0, na))
        to = empty if i == 5 else fresh if i == 9 else addrs[int(rng.integers(0, na))]
        nonce = state[addrs[k]]["nonce"] + sent.get(k, 0)
        sent[k] = sent.get(k, 0) + 1
        value = 0 if i == 5 else int(rng.integers(0, 10**18))
        raws.append(S.make_tx(oracle, keys[k], (0, 1, 2)[i % 3], 1, nonce=nonce, gas_price=10 + i % 7, gas=21000, to=to, value=value, max_priority=10 + i % 7))
        expect.append((addrs[k], to, value, 10 + i % 7))
    wd = [(addrs[int(rng.integers(0, na))] if j % 3 else fresh, int(rng.integers(1, 1 << 36))) for j in range(10)]
    header = {"coinbase": coinbase, "base_fee": 7, "gas_limit": 30_000_000}
    touched = list(dict.fromkeys(addrs + [empty, fresh, coinbase]))
    w = _witness(P, oracle, state, touched, may_remove=[empty])
    r = B.run_transfer_block(raws, wd, header, w, w.state_root, 1, TX.FORK_LONDON)
    # the same block by the definition over the same rows, and by plain bookkeeping
    now = {a: dict(v) for a, v in state.items()}
    for s, to, value, price in expect:
        now[s]["balance"] -= 21000 * price + value
        now[s]["nonce"] += 1
        now.setdefault(to, {"nonce": 0, "balance": 0})["balance"] += value
        now.setdefault(coinbase, {"nonce": 0, "balance": 0})["balance"] += 21000 * (price - 7)
    for a, g in wd:
        now.setdefault(a, {"nonce": 0, "balance": 0})["balance"] += g * R.GWEI
    del now[empty]
    assert r.gas_used == 21000 * n and r.settlement.settled
    assert int(r.settlement.account_op[[bytes(x) for x in w.info()["addresses"]].index(empty)]) == R.POST_DELETE
    assert r.state_root == _oracle_root(oracle, now) == _oracle_root(oracle, _applied(state, w.info(), r.settlement))
    assert r.receipts_root == receipts_ref.receipts_root([((0, 1, 2)[i % 3], True, 21000 * (i + 1), []) for i in range(n)])
    w.close()
