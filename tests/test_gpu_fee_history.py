"""Fee history over chain segments on the device (phant_block_fee_history, phant_block_fee_history_dev,
phant_amd.types.block.reward_percentiles and fee_history) against tests/feehist_ref.py, which defines every output from the rules of
include/phant_gpu.h in Python integers.  Every comparison is exact, in the host and the device form.  The rows come once out of real
block_bodies and receipt_segments calls over a small generated segment, otherwise they are packed by hand.
tests/test_emu_fee_history.py runs the same bodies over the kernel sources compiled for the host."""
import contextlib
import ctypes as C
import random

import numpy as np
import pytest

from tests import feehist_ref as R
from tests.test_gpu_requests import RawReq
from tests.test_gpu_transactions import OK, E_INVALID_ARG, E_UNSUPPORTED, _ctx, _first_difference

pytestmark = pytest.mark.gpu
UNTOUCHED = 0xEEEEEEEE
M64, M256 = (1 << 64) - 1, (1 << 256) - 1
WIDTH = {"reward": 32, "tip": 32, "order": 4, "block_gas_used": 8, "block_flags": 4}
PCT = [5000, 0, 10000, 1, 2500, 9999, 10000, 0, 7, 5000]  # unordered, repeated, both ends


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


@contextlib.contextmanager
def block_max(ctx, rows):
    ctx.diag_set("feehist_block_max", rows)
    try:
        yield
    finally:
        ctx.diag_set("feehist_block_max", 0)


# ------------------------------------------------------------------------------------------------------------- the rows
def be32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values) or bytes(32), np.uint8)[:32 * len(values)].reshape(-1, 32).copy()


def pack(blocks, base=None):
    """blocks: per block its rows (price, gas_used); base: per block its base fee, or None (a NULL base_fee) -> the arrays of
    phant_fee_history_in and the integers tests/feehist_ref.py takes"""
    rows = [r for b in blocks for r in b]
    first = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint32)
    a = {"block_first": first, "price": be32([p for p, _ in rows]), "base_fee": None if base is None else be32(base),
         "gas_used": np.asarray([g for _, g in rows], np.uint64)}
    return a, (first.tolist(), [p for p, _ in rows], [g for _, g in rows], base)


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawFH:
    """phant_fee_history_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, rows, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.rows = L, dev, torch, rows
        self.nb, self.n = len(rows["block_first"]) - 1, len(rows["gas_used"])

    _up, _buf = RawReq._up, RawReq._buf

    def call(self, ctx, pct, want=None, guard=64, sizes=None, reserved=(0, 0), skew=None, in_skew=0, over=None):
        """-> (rc, {output: bytes}, first_bad_block); every buffer has `guard` bytes of 0xEE in front of and behind its rows.  over: {a
        count or an input array: value} put in last (an array is uploaded, None passes NULL); in_skew: bytes the byte arrays of the inputs
        are moved up by; skew: {output: bytes its pointer is moved up by}"""
        L = self.L
        want = R.OUTPUTS if want is None else want
        ins = dict(self.rows, percentile=np.asarray(pct, np.uint32))
        counts = dict(n_blocks=self.nb, n=self.n, n_percentiles=len(pct))
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k, dt, _ in L.FEEHIST_INPUTS:
            a = None if ins[k] is None else np.ascontiguousarray(ins[k], dt)
            if k == "percentile":  # (host memory in both forms)
                keep[k], ptr[k] = (None, None) if a is None else (a if len(a) else np.zeros(1, np.uint32), None)
                ptr[k] = None if a is None else keep[k].ctypes.data
            else:
                keep[k], ptr[k] = self._up(a, in_skew if dt == "u1" else 0)
        arg = L.PhantFeeHistoryIn(C.sizeof(L.PhantFeeHistoryIn), counts["n_blocks"], counts["n"], counts["n_percentiles"], *[ptr[k] for k, _, _ in L.FEEHIST_INPUTS], reserved[0])
        rows = {"reward": self.nb * len(pct), "tip": self.n, "order": self.n, "block_gas_used": self.nb, "block_flags": self.nb}
        size = {k: WIDTH[k] * rows[k] for k in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out_ptr = lambda k: (bufs[k].data_ptr() if self.dev else bufs[k].ctypes.data) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        out = L.PhantFeeHistoryOut(C.sizeof(L.PhantFeeHistoryOut), UNTOUCHED, *[out_ptr(k) for k, _, _ in L.FEEHIST_OUTPUTS], reserved[1])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_fee_history_dev if self.dev else ctx._lib.phant_block_fee_history
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        del keep
        return rc, got, int(out.first_bad_block)


_EXPECTED = {}


def check(P, blocks, pct, base=None, forms=(False, True), key=None, ctx=None, **kw):
    """every answer of the call against the definition, in both forms -> the definition's outputs as integers"""
    a, ints = pack(blocks, base)
    if key is None or (key, tuple(pct)) not in _EXPECTED:
        exp = R.expected(ints[0], ints[1], ints[2], pct, ints[3])
        if key is not None:
            _EXPECTED[key, tuple(pct)] = exp
    else:
        exp = _EXPECTED[key, tuple(pct)]
    exp, first_bad = exp
    ctx = ctx or _ctx(P)
    for dev in forms:
        rc, got, fb = RawFH(a, dev=dev).call(ctx, pct, **kw)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert fb == first_bad, (dev, fb, first_bad)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    nb, np_ = len(blocks), len(pct)
    reward = [[int.from_bytes(exp["reward"][32 * (b * np_ + k):32 * (b * np_ + k) + 32], "big") for k in range(np_)] for b in range(nb)]
    return {"reward": reward, "order": np.frombuffer(exp["order"], "<u4").tolist(), "gas": np.frombuffer(exp["block_gas_used"], "<u8").tolist(),
            "flags": np.frombuffer(exp["block_flags"], "<u4").tolist(), "first_bad": first_bad}


# ------------------------------------------------------------------------------------------------------ the known answer
KNOWN = {0: 1, 2000: 1, 2001: 1, 2100: 3, 9000: 3, 9100: 5, 10000: 5}


def test_the_known_answer(P):
    """derived by hand: prices 5, 1, 3 at base fee 0 with gas 10, 20, 70 -> order rows 1, 2, 0, sums 20, 90, 100"""
    a, _ = pack([[(5, 10), (1, 20), (3, 70)]])
    for dev in (False, True):
        rc, got, fb = RawFH(a, dev=dev).call(_ctx(P), list(KNOWN))
        assert rc == OK and fb == 1
        assert np.frombuffer(got["order"], "<u4").tolist() == [1, 2, 0]
        assert [int.from_bytes(got["reward"][32 * k:32 * k + 32], "big") for k in range(len(KNOWN))] == list(KNOWN.values())
        assert np.frombuffer(got["block_gas_used"], "<u8").tolist() == [100] and got["block_flags"] == bytes(4)
    r = check(P, [[(5, 10), (1, 20), (3, 70)]], list(KNOWN), base=[0])
    assert r["reward"] == [list(KNOWN.values())]


# ------------------------------------------------------------------------------------------------------------- sizes
SIZES = (256, 0, 1, 255, 2, 63, 64, 65, 257, 600)  # blocks 2 and 4 start on the tile edges 256 and 512; 1 923 rows


def big_segment():
    rng = random.Random(5)
    base = [rng.choice((0, 7, 10**9, 1 << 200)) for _ in SIZES]
    blocks = []
    for b, size in enumerate(SIZES):
        kind = b % 3  # few distinct tips (ties everywhere), wide tips, or both
        rows = []
        for _ in range(size):
            tip = rng.randrange(4) if kind == 0 else rng.randrange(1 << 250) if kind == 1 else rng.choice((0, 1, rng.randrange(1 << 64), rng.randrange(1 << 250)))
            rows.append((base[b] + tip, rng.choice((0, 21000, rng.randrange(1 << 24), rng.randrange(1 << 40)))))
        blocks.append(rows)
    return blocks, base


def test_blocks_that_straddle_the_waves_and_the_tiles(P):
    """blocks of 256, 0, 1, 255, 2, 63, 64, 65, 257 and 600 rows: blocks inside one wave of the ranking, blocks over many, boundaries on
    and off the scan's 256-row tiles; ten percentiles, unordered and repeated, then a single one and a hundred"""
    blocks, base = big_segment()
    r = check(P, blocks, PCT, base, key="big")
    assert sorted(r["order"]) == list(range(sum(SIZES))) and r["first_bad"] == len(SIZES)
    assert all(row[1] <= row[0] <= row[2] and row[2] == row[6] and row[1] == row[7] for row in r["reward"])
    check(P, blocks, [3333], base, key="big", want=("reward", "block_gas_used"))
    check(P, blocks, [(101 * k) % 10001 for k in range(100)], base, key="big", want=("reward",))
    check(P, blocks, PCT, None, key="big, no base fee")  # base_fee NULL: the prices are the tips


# --------------------------------------------------------------------------------------------------------------- ties
def test_ties_and_tips_that_differ_in_one_limb(P):
    """all tips of a block equal: order is the identity; tips that differ only in the top limb, only in the lowest limb; 2^256 - 1"""
    same = [(1000, 10 + i) for i in range(70)]
    top = [((70 - i) << 224 | 5, 1) for i in range(70)]       # descending in the top limb alone
    low = [(1 << 255 | (i * 37) % 70, 1) for i in range(70)]  # a permutation in the lowest limb alone
    edge = [(M256, 5), (0, 5), (M256 - 1, 5), (M256, 5), (1 << 128, 5)]
    r = check(P, [same, top, low, edge], PCT)
    assert r["order"][:70] == list(range(70))
    assert r["order"][70:140] == list(range(139, 69, -1))
    assert r["order"][140:210] == [140 + [(i * 37) % 70 for i in range(70)].index(v) for v in range(70)]
    assert r["order"][210:] == [211, 214, 212, 210, 213] and r["reward"][3][2] == M256 and r["reward"][3][1] == 0
    r = check(P, [same, top, low, edge], [0, 10000], base=[1000, 5, 1 << 255, 0])
    assert r["order"][:70] == list(range(70)) and r["reward"][0] == [0, 0] and r["flags"] == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------- below the base fee
def test_rows_below_the_base_fee(P):
    """one row below its block's base fee, and a whole block of them: tip 0, the block's flag, first_bad_block; a price equal to the base
    fee is no flag"""
    blocks = [[(10, 1), (12, 1)], [(10, 5), (9, 5), (30, 5)], [], [(1, 1)] * 65, [(1 << 200, 3), (1 << 199, 3)]]
    r = check(P, blocks, PCT, base=[10, 10, 99, 2, (1 << 200) + 1])
    assert r["flags"] == [0, 1, 0, 1, 1] and r["first_bad"] == 1
    assert r["order"][2:5] == [2, 3, 4] and r["order"][5:70] == list(range(5, 70))
    assert r["reward"][3] == [0] * len(PCT) and r["reward"][4] == [0] * len(PCT)
    assert check(P, blocks[3:], [5000], base=[2, 0])["first_bad"] == 0
    assert check(P, blocks[:1] + blocks[2:3], [5000], base=[10, 99])["first_bad"] == 2


# ----------------------------------------------------------------------------------------------------------- the gas rows
def test_gas_of_zero_and_sums_beyond_64_bits(P):
    """a block whose rows used no gas: G = 0 and every percentile picks rank 0; rows of 2^64 - 1: the sum passes 2^64, block_gas_used
    clamps and the rewards stay exact"""
    zero = [(50 - i, 0) for i in range(40)]
    huge = [(i, M64) for i in range(300)]  # G = 300 (2^64 - 1): every row a three-hundredth
    mixed = [(7, M64), (3, 1), (5, M64)]
    r = check(P, [zero, huge, mixed], PCT + [3334, 5000, 5001])  # (mixed: sums 1, 2^64, 2^65 - 1; half of G is 2^64 - 1)
    assert r["gas"] == [0, M64, M64] and r["reward"][0] == [11] * (len(PCT) + 3)
    assert r["reward"][1][:3] == [149, 0, 299] and r["reward"][2][-3:] == [5, 5, 7]


def test_thresholds_that_a_sum_meets_exactly(P):
    """four rows of 25 gas: 2500 basis points are met by the first row's sum exactly, 2501 are not (floor(100 x 0.2501) = 25 still is),
    2600 need the second row"""
    rows = [(40, 25), (10, 25), (30, 25), (20, 25)]
    r = check(P, [rows], [2500, 2501, 2600, 5000, 5001, 5100, 7500, 7600, 10000])
    assert r["reward"] == [[10, 10, 20, 20, 20, 30, 30, 40, 40]]
    r = check(P, [[(p, 2500) for p, _ in rows]], [2500, 2501, 2600])  # G = 10000: a basis point is a unit of gas
    assert r["reward"] == [[10, 20, 20]]


# --------------------------------------------------------------------------------------------------- outputs and buffers
def test_subsets_of_the_outputs_and_odd_addresses(P):
    """every subset of the outputs NULL, guard bytes around every buffer; the byte arrays of the inputs at odd addresses in allocations
    that end with them; the byte outputs at odd addresses in both forms, the word outputs in the host form (which copies bytes)"""
    rng = random.Random(9)
    blocks = [[(rng.randrange(1 << 70), rng.randrange(1 << 30)) for _ in range(size)] for size in (70, 0, 3, 200)]
    base = [5, 6, 7, 1 << 69]
    a, ints = pack(blocks, base)
    exp, first_bad = R.expected(ints[0], ints[1], ints[2], PCT, ints[3])
    ctx = _ctx(P)
    for dev in (False, True):
        raw = RawFH(a, dev=dev)
        for mask in range(32):
            want = tuple(k for i, k in enumerate(R.OUTPUTS) if mask >> i & 1)
            rc, got, fb = raw.call(ctx, PCT, want=want)
            assert rc == OK and fb == first_bad, (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
        for in_skew in (1, 3):
            rc, got, fb = raw.call(ctx, PCT, in_skew=in_skew, skew={"reward": 1, "tip": 3})
            assert rc == OK and fb == first_bad and all(got[k, "guards"] and got[k] == exp[k] for k in R.OUTPUTS), (dev, in_skew)
    rc, got, fb = RawFH(a).call(ctx, PCT, skew={"order": 1, "block_gas_used": 3, "block_flags": 2})
    assert rc == OK and all(got[k, "guards"] and got[k] == exp[k] for k in R.OUTPUTS)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments(P):
    """each returns PHANT_E_INVALID_ARG and touches nothing; in the device form block_first is caught by the checking kernel"""
    ctx = _ctx(P)
    blocks = [[(9, 1), (8, 2)], [], [(7, 3), (6, 4), (5, 5)], [(4, 6)]]
    a, ints = pack(blocks, [1, 2, 3, 4])
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantFeeHistoryIn), C.sizeof(L.PhantFeeHistoryOut))
    pct = [0, 5000, 10000]

    def refused(raw, pct=pct, code=E_INVALID_ARG, **kw):
        rc, got, fb = raw.call(ctx, pct, **kw)
        assert rc == code, (rc, kw)
        assert fb == UNTOUCHED, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawFH(a, dev=dev)
        rc, _, fb = raw.call(ctx, pct)
        assert rc == OK and fb == 4
        for k in range(2):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        refused(raw, reserved=(1, 0))
        refused(raw, reserved=(0, 1 << 33))
        for k in ("block_first", "price", "gas_used", "percentile"):
            refused(raw, over={k: None})
        refused(raw, over={"n_blocks": 0})  # (rows without a block)
        refused(raw, over={"n": raw.n - 1})
        refused(raw, over={"n": raw.n + 1})
        for at in range(3):
            for v in (10001, 0xFFFFFFFF):
                refused(raw, pct=[v if i == at else p for i, p in enumerate(pct)])
        for at, by in ((0, 1), (1, 100), (2, -1), (-1, 1), (-1, -1)):
            lie = np.array(a["block_first"]).copy()
            lie[at] = (int(lie[at + 1]) + 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
            refused(raw, over={"block_first": lie})
    dev = RawFH(a, dev=True)
    for k, by in (("order", 2), ("block_flags", 1), ("block_gas_used", 4)):
        refused(dev, skew={k: by})
    for form_dev in (False, True):
        # no block: the scalar alone; no percentile: everything but reward; no row: zero rewards
        rc, got, fb = RawFH(pack([])[0], dev=form_dev).call(ctx, pct)
        assert rc == OK and fb == 0 and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str))
        exp, first_bad = R.expected(ints[0], ints[1], ints[2], [], ints[3])
        rc, got, fb = RawFH(a, dev=form_dev).call(ctx, [])
        assert rc == OK and fb == first_bad == 4 and all(got[k, "guards"] and got[k] == exp[k] for k in R.OUTPUTS)
        rc, got, fb = RawFH(a, dev=form_dev).call(ctx, [], over={"percentile": None})
        assert rc == OK and fb == 4 and got["order"] == exp["order"]
        rc, got, fb = RawFH(pack([[], [], []], [1, 2, 3])[0], dev=form_dev).call(ctx, pct)
        assert rc == OK and fb == 3 and got["reward"] == bytes(32 * 9) and got["block_gas_used"] == bytes(24) and got["block_flags"] == bytes(12)


def test_too_many_rewards_is_unsupported(P):
    """n_blocks x n_percentiles >= 2^31: refused from the counts alone, before block_first is read or anything is sized"""
    ctx = _ctx(P)
    L = __import__("phant_amd")._lib
    one = np.zeros(4, np.uint32)
    for fn, n_blocks, rc in ((ctx._lib.phant_block_fee_history, 1 << 30, E_UNSUPPORTED), (ctx._lib.phant_block_fee_history_dev, 1 << 30, E_UNSUPPORTED)):
        arg = L.PhantFeeHistoryIn(C.sizeof(L.PhantFeeHistoryIn), n_blocks, 0, 2, one.ctypes.data, None, None, None, one.ctypes.data, 0)
        out = L.PhantFeeHistoryOut(C.sizeof(L.PhantFeeHistoryOut), UNTOUCHED, None, None, None, None, None, 0)
        assert fn(ctx.handle, C.byref(arg), C.byref(out)) == rc and out.first_bad_block == UNTOUCHED


def test_the_cap_on_a_blocks_rows(P):
    """with the diag switch at 257 a block of 257 rows is answered and a block of 258 is PHANT_E_UNSUPPORTED with nothing written, in both
    forms; the product's cap is PHANT_FEEHIST_BLOCK_MAX, and the switch never raises it"""
    ctx = _ctx(P)
    L = __import__("phant_amd")._lib
    assert L.FEEHIST_BLOCK_MAX == 65536
    rng = random.Random(3)
    rows = [(rng.randrange(50), rng.randrange(1 << 20)) for _ in range(258)]
    with block_max(ctx, 257):
        check(P, [rows[:3], rows[:257], []], PCT, ctx=ctx)
        for dev in (False, True):
            for blocks in ([rows], [rows[:3], [], rows]):
                rc, got, fb = RawFH(pack(blocks)[0], dev=dev).call(ctx, PCT)
                assert rc == E_UNSUPPORTED and fb == UNTOUCHED and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)), dev
    check(P, [rows], PCT, ctx=ctx)  # (the switch is back at the product's value)
    with block_max(ctx, 1 << 20):
        check(P, [rows], [5000], ctx=ctx)


# ------------------------------------------------------------------------------------------------------- the layers above
def small_segment(P):
    """three London blocks through the real calls: -> (the packed bodies' answer, the receipts' answer, the prices and gas by hand)"""
    from tests import receipts_seg_ref as G
    from tests.test_gpu_receipt_segments import _enc, _plain
    from tests.test_gpu_transactions import raw_tx
    B, T = P.types.block, P.types.receipt
    base = [100, 0, 250]
    spec = [[(2, 1000, 30), (0, 170, 0), (2, 120, 50), (1, 100, 0), (2, 90, 5)],  # (type, gas price or max fee, priority fee); the last is below the base fee
            [],
            [(2, 300, 300), (2, 260, 3), (0, 251, 0)]]
    gas = [[21000, 50000, 21000, 90000, 30000], [], [40000, 21000, 60000]]
    txs = [[raw_tx(t, nonce=i, gas_price=price, gas=100000, max_priority=prio) for i, (t, price, prio) in enumerate(b)] for b in spec]
    bodies = B.block_bodies(B.pack_bodies(txs), 1, P._lib.TXS_FORK_LONDON, base_fee=base, recover=False, roots=False)
    receipts = [[_plain(i, gas=sum(g[:i + 1])) for i in range(len(g))] for g in gas]
    segs = T.receipt_segments(T.pack_receipt_segments(_enc(receipts, G.ETH69)), form=G.ETH69, roots=False, logs=False)
    price = [[0 if t == 2 and p < base[b] else min(prio, p - base[b]) + base[b] if t == 2 else p for t, p, prio in blk] for b, blk in enumerate(spec)]
    return bodies, segs, base, price, gas


def test_rows_from_the_real_calls_and_packed_by_hand(P):
    """effective_gas_price as block_bodies answers it and gas_used as receipt_segments answers it, fed to the call as they are; and the
    same rows packed by hand"""
    bodies, segs, base, price, gas = small_segment(P)
    blocks = [list(zip(p, g)) for p, g in zip(price, gas)]
    by_hand, ints = pack(blocks, base)
    assert np.asarray(bodies.effective_gas_price).tobytes() == by_hand["price"].tobytes() and np.asarray(segs.gas_used).tobytes() == by_hand["gas_used"].tobytes()
    assert np.asarray(bodies.block_first).tolist() == np.asarray(segs.block_first).tolist() == ints[0]
    real = {"block_first": bodies.block_first, "price": bodies.effective_gas_price, "base_fee": by_hand["base_fee"], "gas_used": segs.gas_used}
    exp, first_bad = R.expected(ints[0], ints[1], ints[2], PCT, base)
    assert first_bad == 0 and np.frombuffer(exp["block_flags"], "<u4").tolist() == [1, 0, 0]
    for rows in (real, by_hand):
        for dev in (False, True):
            rc, got, fb = RawFH(rows, dev=dev).call(_ctx(P), PCT)
            assert rc == OK and fb == first_bad and all(got[k, "guards"] and got[k] == exp[k] for k in R.OUTPUTS), dev
    assert np.frombuffer(exp["order"], "<u4").tolist() == [3, 4, 2, 0, 1, 7, 6, 5]  # (tips 30, 70, 20, 0, 0 and 50, 3, 1)


def test_reward_percentiles_on_host_arrays_and_device_tensors(P):
    import torch
    B = P.types.block
    blocks, base = big_segment()
    a, ints = pack(blocks[2:8], base[2:8])
    exp, first_bad = R.expected(ints[0], ints[1], ints[2], PCT, ints[3])
    h = B.reward_percentiles(a["block_first"], a["price"], a["gas_used"], PCT, base_fee=a["base_fee"])
    assert h.first_bad_block == first_bad and h.reward.shape == (6, len(PCT), 32)
    assert all(np.asarray(getattr(h, "flags" if k == "block_flags" else k)).tobytes() == exp[k] for k in R.OUTPUTS)
    assert h.rewards()[3][2] == int.from_bytes(exp["reward"][32 * (3 * len(PCT) + 2):][:32], "big")
    dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in a.items()}
    d = B.reward_percentiles(dev["block_first"], dev["price"], dev["gas_used"], PCT, base_fee=dev["base_fee"])
    assert d.first_bad_block == first_bad
    assert all(getattr(d, "flags" if k == "block_flags" else k).cpu().numpy().tobytes() == exp[k] for k in R.OUTPUTS)
    none = B.reward_percentiles(a["block_first"], a["price"], a["gas_used"], [], base_fee=None)
    assert none.reward.shape == (6, 0, 32) and none.order.tobytes() == R.expected(ints[0], ints[1], ints[2], [], None)[0]["order"]
    with pytest.raises(ValueError):
        B.reward_percentiles(a["block_first"], a["price"][:-1], a["gas_used"], PCT)
    with pytest.raises(P._lib.PhantError):
        B.reward_percentiles(a["block_first"], a["price"], a["gas_used"], [10001])


def test_fee_history_of_a_segment(P):
    """eth_feeHistory over three blocks: reward from the device, everything else host arithmetic on n + 1 numbers, against the ref"""
    from tests import tx_ref_forks as F
    from tests.test_gpu_headers import _objs, anchor, child
    B = P.types.block
    bodies, segs, base, price, gas = small_segment(P)
    rng = np.random.default_rng(4)
    hs = [anchor(rng, 21, base_fee_per_gas=base[0], gas_limit=30_000_000, gas_used=sum(gas[0]), blob_gas_used=3 * 131072, excess_blob_gas=5 * 131072)]
    for b in (1, 2):
        hs.append(child(rng, hs[-1], base_fee_per_gas=base[b], gas_used=sum(gas[b]), blob_gas_used=(9 * 131072, 131072)[b - 1], excess_blob_gas=(40 + b) * 131072))
    fork = P._lib.TXS_FORK_PRAGUE
    pcts = [0, 25.5, 50, 99.99, 100]
    bp = [0, 2550, 5000, 9999, 10000]
    fh = B.fee_history(_objs(P, hs), bodies, segs, pcts, fork)
    exp, _ = R.expected(np.asarray(segs.block_first).tolist(), [p for b in price for p in b], [g for b in gas for g in b], bp, base)
    assert fh["reward"] == [[int.from_bytes(exp["reward"][32 * (b * 5 + k):][:32], "big") for k in range(5)] for b in range(3)]
    assert fh["oldestBlock"] == hs[0]["block_number"]
    assert fh["baseFeePerGas"] == base + [R.next_base_fee(base[2], hs[2]["gas_used"], hs[2]["gas_limit"])]
    assert fh["gasUsedRatio"] == [h["gas_used"] / h["gas_limit"] for h in hs]
    excess = [h["excess_blob_gas"] for h in hs] + [R.next_excess_blob_gas(hs[2]["excess_blob_gas"], hs[2]["blob_gas_used"], 6 * 131072)]
    assert fh["baseFeePerBlobGas"] == [F.blob_base_fee(x, F.PRAGUE) for x in excess] and excess[3] == (42 + 1 - 6) * 131072
    assert fh["blobGasUsedRatio"] == [h["blob_gas_used"] / (9 * 131072) for h in hs] and fh["blobGasUsedRatio"][1] == 1.0
    as_dicts = B.fee_history(_objs(P, hs), {"block_first": bodies.block_first, "effective_gas_price": bodies.effective_gas_price},
                             {"block_first": segs.block_first, "gas_used": segs.gas_used}, pcts, fork)
    assert as_dicts == fh
    for bad in ([33.333], [101], [-1], [float("nan")]):
        with pytest.raises(ValueError):
            B.fee_history(_objs(P, hs), bodies, segs, bad, fork)
    with pytest.raises(ValueError):
        B.fee_history(_objs(P, hs), {"block_first": [0, 4, 5, 8], "effective_gas_price": bodies.effective_gas_price}, segs, pcts, fork)
    with pytest.raises(ValueError):
        B.fee_history(_objs(P, hs[:2]), bodies, segs, pcts, fork)
