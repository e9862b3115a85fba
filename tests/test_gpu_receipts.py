"""A block's receipts on the device (phant_block_receipts, phant_block_receipts_dev, phant_amd.types.receipt.block_receipts)
against tests/receipts_ref.py, which defines the answer for any block.  Every comparison is exact.  tests/test_emu_receipts.py
runs the same bodies over the kernel sources compiled for the host, at the sizes tests/suite.py gives it."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import golden, suite
from tests import receipts_ref as R

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG, E_UNSUPPORTED = 0, -1, -6


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _log(rng, topics=None, data_len=None):
    topics = int(rng.integers(0, 5)) if topics is None else topics
    data_len = int(rng.integers(0, 300)) if data_len is None else data_len
    return (_bytes(rng, 20), [_bytes(rng, 32) for _ in range(topics)], _bytes(rng, data_len))


def _receipt(rng, logs=None, gas=None, tx_type=None, ok=None):
    if logs is None:
        logs = [_log(rng) for _ in range(int(rng.integers(0, 4)))]
    return (int(rng.choice([0, 0, 1, 2, 3])) if tx_type is None else tx_type, bool(rng.integers(0, 2)) if ok is None else ok,
            int(rng.integers(21000, 30_000_000)) if gas is None else gas, logs)


def _objs(P, receipts):
    T = P.types.receipt
    return [T.Receipt.init(ok, gas, [T.Log(a, ts, d) for a, ts, d in logs], tx_type) for tx_type, ok, gas, logs in receipts]


def _oracle():
    from oracle import oracle as O
    return O


def check_block(P, receipts, other=(), at=0, second_route=False):
    """the new call's every answer for this block against the reference -> the call's result"""
    O = _oracle()
    res = P.types.receipt.block_receipts(_objs(P, receipts), other_lists=other, receipts_at=at)
    enc = [R.encode(r) for r in receipts]
    assert len(res.encoded) == len(enc)
    for i, (g, w) in enumerate(zip(res.encoded, enc)):
        assert g == w, (i, len(g), len(w))
    assert [row.tobytes() for row in res.blooms] == [R.bloom_of(r[3]) for r in receipts]
    assert res.logs_bloom == R.block_bloom(receipts)
    lists = [list(x) for x in other]
    lists.insert(at, enc)
    assert res.roots == [O.index_root_rlp(x) for x in lists]
    assert res.receipts_root == res.roots[at]
    if second_route:  # through code that was there before: the flattened bloom call and the root of host-made encodings
        assert np.array_equal(res.blooms, P.types.receipt.logs_blooms([[(a, ts) for a, ts, _ in r[3]] for r in receipts]))
        assert res.receipts_root == P.mpt.index_root_rlp(enc)
    return res


# ------------------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("n", [0, 1, 2, 127, 128, 129, 130, 256, 257, 300])
def test_receipt_counts(P, n):
    """where key 0x80 (index 0) sits in trie order, and where rlp(index) grows to two bytes and to three"""
    rng = np.random.default_rng(1000 + n)
    max_logs = suite.scale(4, 2)
    receipts = [_receipt(rng, logs=[_log(rng, data_len=int(rng.integers(0, suite.scale(300, 40)))) for _ in range(int(rng.integers(0, max_logs)))])
                for _ in range(n)]
    res = check_block(P, receipts, second_route=True)
    if n == 0:
        assert res.receipts_root == _oracle().index_root_rlp([]) and res.logs_bloom == bytes(256)


# -------------------------------------------------------------------------------------------------------- boundaries
def _search(make, measure, target):
    """smallest d with measure(make(d)) == target (measure is monotone in d)"""
    lo, hi = 0, 70000
    while lo < hi:
        mid = (lo + hi) // 2
        if measure(make(mid)) < target:
            lo = mid + 1
        else:
            hi = mid
    assert measure(make(lo)) == target, (target, lo)
    return lo


def _payload_len(b):
    """the payload length of the RLP list b"""
    return b[0] - 0xc0 if b[0] < 0xf8 else int.from_bytes(b[1:1 + b[0] - 0xf7], "big")


def _log_bytes(log):
    a, ts, d = log
    return R.rlp_list([R.rlp_str(a), R.rlp_list([R.rlp_str(t) for t in ts]), R.rlp_str(d)])


def test_rlp_boundaries(P):
    rng = np.random.default_rng(7)
    receipts = []
    # log data: empty, one byte on either side of 0x80, and both sides of every length-of-length step
    for d in (b"", b"\x00", b"\x7f", b"\x80", b"\xff"):
        receipts.append(_receipt(rng, logs=[(_bytes(rng, 20), [_bytes(rng, 32)], d)]))
    for dl in (54, 55, 56, 57, 255, 256, 65535, 65536):
        receipts.append(_receipt(rng, logs=[_log(rng, topics=1, data_len=dl)]))
    # topic counts: a topics list of 0, 33, 66 (long header), 132 and 297 bytes
    receipts.append(_receipt(rng, logs=[_log(rng, topics=t, data_len=3) for t in (0, 1, 2, 4, 9)]))
    # a log payload of exactly 55 and 56 bytes: no topics, 32 and 33 bytes of data
    for dl in (32, 33):
        log = _log(rng, topics=0, data_len=dl)
        assert _payload_len(_log_bytes(log)) == 23 + dl
        receipts.append(_receipt(rng, logs=[log]))
    # a logs list of 55 / 56, 255 / 256, 65 535 / 65 536 bytes: one log of that size
    for target in (55, 56, 255, 256, 65535, 65536):
        mk = lambda d: (b"\x5a" * 20, [], bytes(d))  # noqa: E731
        d = _search(mk, lambda lg: len(_log_bytes(lg)), target)
        r = _receipt(rng, logs=[(_bytes(rng, 20), [], b"\x80" + _bytes(rng, d - 1))])
        assert _payload_len(R.rlp_list([_log_bytes(r[3][0])])) == target
        receipts.append(r)
    # a receipt payload on both sides of 65 535 / 65 536
    for target in (65535, 65536):
        mk = lambda d: (0, True, 21000, [(b"\x5a" * 20, [bytes(32)], b"\x80" * d)])  # noqa: E731
        d = _search(mk, lambda r: _payload_len(R.encode(r)), target)
        for tx_type in (0, 2):
            r = (tx_type, True, 21000, [(_bytes(rng, 20), [_bytes(rng, 32)], b"\x81" + _bytes(rng, d - 1))])
            assert _payload_len(R.encode(r)[1 if tx_type else 0:]) == target
            receipts.append(r)
    # cumulative gas, status and type
    for gas in (0, 1, 0x7f, 0x80, 0xff, 0x100, 1 << 32, 1 << 63, (1 << 64) - 1):
        for ok in (False, True):
            receipts.append(_receipt(rng, gas=gas, ok=ok, logs=[] if gas & 1 else [_log(rng, data_len=5)]))
    for tx_type in (0, 1, 2, 3, 4, 0x7f):
        receipts.append(_receipt(rng, tx_type=tx_type, logs=[]))
        receipts.append(_receipt(rng, tx_type=tx_type))
    res = check_block(P, receipts)
    assert [R.decode(e) for e in res.encoded] == receipts


# ------------------------------------------------------------------------------------------------------------ shapes
def test_receipts_without_logs_between_receipts_with_logs(P):
    rng = np.random.default_rng(8)
    receipts = [_receipt(rng, logs=[] if i % 3 else [_log(rng)]) for i in range(10)]
    res = check_block(P, receipts, second_route=True)
    for i, (row, e) in enumerate(zip(res.blooms, res.encoded)):
        assert row.any() == (i % 3 == 0)
        assert e.endswith(b"\xc0") == (i % 3 != 0)


def test_one_receipt_with_many_logs(P):
    """hundreds of lanes OR into one row, hundreds of log units write into one receipt"""
    rng = np.random.default_rng(9)
    k = suite.scale(600, 150)
    receipts = [_receipt(rng, logs=[]), _receipt(rng, logs=[_log(rng, data_len=int(rng.integers(0, 40))) for _ in range(k)]), _receipt(rng, logs=[_log(rng)])]
    check_block(P, receipts, second_route=True)


def test_a_block_without_any_log(P):
    rng = np.random.default_rng(10)
    res = check_block(P, [_receipt(rng, logs=[]) for _ in range(5)])
    assert res.logs_bloom == bytes(256) and not res.blooms.any()


def test_a_large_payload_at_an_odd_offset(P):
    rng = np.random.default_rng(11)
    receipts = [_receipt(rng, logs=[_log(rng, topics=1, data_len=3), _log(rng, topics=3, data_len=40 * 1024 + 1), _log(rng, topics=2, data_len=7)]),
                _receipt(rng, logs=[_log(rng, data_len=13)])]
    assert sum(len(d) for _, _, d in receipts[0][3][:1]) % 2 == 1  # the payload starts at an odd offset of the data blob
    check_block(P, receipts)


def test_a_block_beyond_the_pinned_stage(P):
    """more than 8 MiB in and out: the caller's arrays and the answers cross the bus array by array, not through the pinned stage"""
    rng = np.random.default_rng(12)
    receipts = [_receipt(rng, logs=[_log(rng, topics=1, data_len=suite.scale(3 * 1024 * 1024, 3000) + k) for k in range(3)]), _receipt(rng, logs=[_log(rng)])]
    check_block(P, receipts, other=[[_bytes(rng, 50)]], at=1)


# ---------------------------------------------------------------------------------------------------------- fixtures
def _tx_type(tx_hex):
    first = bytes.fromhex(tx_hex)[0]
    return first if first < 0x80 else 0


def test_fixture_receipt_tries(P):
    """The fixtures' 87 receiptTrie values through the new call, from FIELDS: 19 empty blocks; 66 blocks of one transaction
    (type from the transaction's first byte, gas from the header: exactly one of the two statuses hits the header's root);
    the two blocks of two transactions (the receipts tests/golden.py finds, decoded to fields); and the three roots of a
    header -- transactions, receipts, withdrawals -- from ONE call."""
    O = _oracle()
    T = P.types.receipt
    blocks = [b for c in golden.fixtures()["cases"] for b in c["blocks"]]
    if suite.EMULATED and not suite.FULL:
        blocks = [b for b in blocks if len(b["tx_values"]) != 1][:6] + [b for b in blocks if len(b["tx_values"]) == 1][::6]
    seen = {0: 0, 1: 0, 2: 0}
    found = {}
    for b in blocks:
        txs = [bytes.fromhex(t) for t in b["tx_values"]]
        wds = [bytes.fromhex(w) for w in b["withdrawal_values"]]
        seen[len(txs)] += 1
        if not txs:
            res = T.block_receipts([], other_lists=[txs, wds], receipts_at=1)
            assert res.receipts_root.hex() == b["receipt_trie"] and res.logs_bloom == bytes(256)
        elif len(txs) == 1:
            cand = golden.one_transaction_receipts(b)
            assert cand is not None
            hits = 0
            for ok, want in zip((True, False), cand):
                res = T.block_receipts([T.Receipt.init(ok, b["gas_used"], [], _tx_type(b["tx_values"][0]))], other_lists=[txs, wds], receipts_at=1)
                assert res.encoded == [want]
                hits += res.receipts_root.hex() == b["receipt_trie"]
            assert hits == 1
        else:
            key = (b["receipt_trie"], b["gas_used"])
            if key not in found:
                found[key] = [R.decode(r) for r in golden.two_transaction_receipts(b, O.index_root_rlp)]
            res = T.block_receipts(_objs(P, found[key]), other_lists=[txs, wds], receipts_at=1)
            assert res.receipts_root.hex() == b["receipt_trie"]
        assert (res.roots[0].hex(), res.roots[2].hex()) == (b["transactions_trie"], b["withdrawals_root"])  # the same call's other two roots
    if not (suite.EMULATED and not suite.FULL):
        assert seen == {0: 19, 1: 66, 2: 2}


# ------------------------------------------------------------------------------------------------------ riding lists
@pytest.mark.parametrize("k", [0, 1, 128, 400])
def test_riding_lists(P, k):
    rng = np.random.default_rng(20 + k)
    k = k if k < 400 else suite.scale(400, 140)
    txs = [bytes([2]) + _bytes(rng, int(rng.integers(60, 200))) for _ in range(k)]
    wds = [_bytes(rng, int(rng.integers(20, 60))) for _ in range((k * 3 + 1) // 4)]
    receipts = [_receipt(rng, logs=[_log(rng, data_len=int(rng.integers(0, 50))) for _ in range(int(rng.integers(0, 2)))]) for _ in range(k)]
    for at in (0, 1, 2):
        res = check_block(P, receipts, other=[txs, wds], at=at)
        lists = [txs, wds]
        lists.insert(at, res.encoded)
        if at == 1:
            assert res.roots == P.mpt.block_roots(lists)
    check_block(P, receipts[:3], other=[[], txs[:2], []], at=3)


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_receipts_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""
    FIELDS = ("tx_type", "status", "cum_gas", "log_first", "address", "topic_first", "data_off", "topics", "data")
    OUTS = ("receipts_root", "logs_bloom", "blooms", "encoded", "encoded_off", "roots_out")

    def __init__(self, P, receipts, dev=False, other=(), at=0):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        a, self.n, self.n_logs, self.n_topics, self.data_bytes = P.types.receipt.pack_receipts(_objs(P, receipts))
        self.arr = {k: self._up(v) for k, v in a.items()}
        self.counts = dict(n_receipts=self.n, n_logs=self.n_logs, n_topics=self.n_topics, data_bytes=self.data_bytes)
        self.other = [self._up(np.frombuffer(b"".join(x) or b"\x00", np.uint8).copy()) for x in other]
        self.other_off = [self._up(np.cumsum([0] + [len(i) for i in x]).astype(np.uint64)) for x in other]
        self.list_n = np.array([len(x) for x in other] or [0], np.uint32)
        self.list_bytes = np.array([sum(map(len, x)) for x in other] or [0], np.uint64)
        self.at = at
        self.null = set()

    def _up(self, a):
        if not self.dev:
            return a
        t = self.torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a)
        return t.cuda()

    def _ptr(self, x):
        return x.data_ptr() if self.dev else x.ctypes.data

    def _down(self, x):
        if not self.dev:
            return x
        self.torch.cuda.synchronize()
        return x.cpu().numpy()

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, want=OUTS, encoded_cap=None, off_cap=None, guard=64):
        """-> (rc, {output: bytes}, encoded_len); every buffer has `guard` bytes of 0xEE behind its capacity"""
        L = self.L
        nl = len(self.other)
        lists_p = (C.c_void_p * max(nl, 1))(*[self._ptr(b) for b in self.other])
        offs_p = (C.c_void_p * max(nl, 1))(*[self._ptr(o) for o in self.other_off])
        ptr = {k: (None if k in self.null else self._ptr(self.arr[k])) for k in self.FIELDS}
        arg = L.PhantReceiptsIn(C.sizeof(L.PhantReceiptsIn), self.counts["n_receipts"], self.counts["n_logs"], self.counts["n_topics"],
                                self.counts["data_bytes"], *[ptr[k] for k in self.FIELDS], C.cast(lists_p, C.c_void_p) if nl else None,
                                C.cast(offs_p, C.c_void_p) if nl else None, self.list_n.ctypes.data if nl else None,
                                self.list_bytes.ctypes.data if nl else None, nl, self.at)
        enc_total = getattr(self, "enc_total", 0)
        encoded_cap = enc_total if encoded_cap is None else encoded_cap
        off_cap = self.n + 1 if off_cap is None else off_cap
        size = dict(receipts_root=32, logs_bloom=256, blooms=256 * self.n, encoded=encoded_cap, encoded_off=8 * off_cap, roots_out=32 * (nl + 1))
        bufs = {k: self._buf((size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantReceiptsOut(C.sizeof(L.PhantReceiptsOut), off_cap, encoded_cap, *[self._ptr(bufs[k]) if k in bufs else None for k in self.OUTS], 0)
        fn = ctx._lib.phant_block_receipts_dev if self.dev else ctx._lib.phant_block_receipts
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            h = self._down(b)
            assert (h[(size[k] + 7) // 8 * 8:] == 0xEE).all(), k  # nothing behind the capacity
            got[k] = h[:size[k]].tobytes()
        return rc, got, int(out.encoded_len)


def _expected(receipts, other=(), at=0):
    O = _oracle()
    enc = [R.encode(r) for r in receipts]
    lists = [list(x) for x in other]
    lists.insert(at, enc)
    roots = [O.index_root_rlp(x) for x in lists]
    off = np.cumsum([0] + [len(e) for e in enc]).astype(np.uint64)
    return dict(receipts_root=roots[at], logs_bloom=R.block_bloom(receipts), blooms=b"".join(R.bloom_of(r[3]) for r in receipts),
                encoded=b"".join(enc), encoded_off=off.tobytes(), roots_out=b"".join(roots))


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def test_every_subset_of_outputs(P):
    rng = np.random.default_rng(30)
    receipts = [_receipt(rng) for _ in range(5)] + [_receipt(rng, logs=[_log(rng), _log(rng, data_len=1)])]
    txs = [_bytes(rng, 70) for _ in range(3)]
    want = _expected(receipts, [txs], 1)
    for dev in (False, True):
        raw = Raw(P, receipts, dev=dev, other=[txs], at=1)
        raw.enc_total = len(want["encoded"])
        subsets = [s for k in range(7) for s in itertools.combinations(Raw.OUTS, k)]
        if suite.EMULATED and not suite.FULL:  # (the emulated run alone thins them; a GPU runs all 64 in both forms)
            subsets = subsets[::5] + [Raw.OUTS]
        for s in subsets:
            rc, got, enc_len = raw.call(_ctx(P), want=s)
            assert rc == OK and enc_len == len(want["encoded"]), (s, rc, _ctx(P)._lib.phant_last_error(_ctx(P).handle))
            assert got == {k: want[k] for k in s}, s


def test_capacity_one_byte_short(P):
    """encoded_len is right, nothing is written past (or into) a buffer that is too small, the other outputs still arrive"""
    rng = np.random.default_rng(31)
    receipts = [_receipt(rng) for _ in range(4)]
    want = _expected(receipts)
    total = len(want["encoded"])
    for dev in (False, True):
        raw = Raw(P, receipts, dev=dev)
        rc, got, enc_len = raw.call(_ctx(P), encoded_cap=total - 1)
        assert rc == OK and enc_len == total
        assert got["encoded"] == b"\xEE" * (total - 1) and got["encoded_off"] == b"\xEE" * (8 * 5)
        assert got["receipts_root"] == want["receipts_root"] and got["blooms"] == want["blooms"] and got["logs_bloom"] == want["logs_bloom"]
        rc, got, enc_len = raw.call(_ctx(P), encoded_cap=total, off_cap=4)  # one offset short
        assert rc == OK and enc_len == total and got["encoded"] == b"\xEE" * total and got["encoded_off"] == b"\xEE" * 32
        rc, got, enc_len = raw.call(_ctx(P), want=("encoded_off",), encoded_cap=0)  # (a buffer nobody wants has no capacity to exceed)
        assert rc == OK and got["encoded_off"] == want["encoded_off"]
        rc, got, enc_len = raw.call(_ctx(P), encoded_cap=total)
        assert rc == OK and got == want


def test_device_form_and_one_context_small_large_small(P):
    rng = np.random.default_rng(32)
    small = [_receipt(rng) for _ in range(3)]
    large = [_receipt(rng) for _ in range(suite.scale(2500, 2100))]  # (beyond what one workgroup plans: the tiled scan and its neighbours)
    txs = [_bytes(rng, 80) for _ in range(5)]
    ctx = _ctx(P)
    for receipts in (small, large, small):
        want = _expected(receipts, [txs, []], 0)
        for dev in (True, False):
            raw = Raw(P, receipts, dev=dev, other=[txs, []], at=0)
            raw.enc_total = len(want["encoded"])
            rc, got, enc_len = raw.call(ctx)
            assert rc == OK and enc_len == raw.enc_total, ctx._lib.phant_last_error(ctx.handle)
            assert got == want


def test_refused_arguments(P):
    rng = np.random.default_rng(33)
    receipts = [_receipt(rng, logs=[_log(rng, topics=2, data_len=9), _log(rng, topics=1, data_len=4)]), _receipt(rng, logs=[]),
                _receipt(rng, logs=[_log(rng, topics=0, data_len=0)])]
    txs = [_bytes(rng, 40) for _ in range(3)]
    ctx = _ctx(P)
    L = ctx._lib

    def refused(dev, code, mutate, other=()):
        raw = Raw(P, receipts, dev=dev, other=other)
        if not dev:
            raw.arr = {k: v.copy() for k, v in raw.arr.items()}
        mutate(raw)
        rc, got, _ = raw.call(ctx, encoded_cap=4096)
        assert rc == code, (dev, rc)
        assert all(v == b"\xEE" * len(v) for v in got.values())  # a refused call writes nothing

    def poke(name, index, value):
        def f(raw):
            if raw.dev:
                raw.arr[name][index] = value if value < 1 << 31 else value - (1 << 32)
            else:
                raw.arr[name][index] = value
        return f

    def count(name, value):
        return lambda raw: raw.counts.__setitem__(name, value)

    for dev in (False, True):
        rc, got, _ = Raw(P, receipts, dev=dev).call(ctx, encoded_cap=4096)  # the block itself is fine
        assert rc == OK
        for name in Raw.FIELDS:  # null pointers where counts are non-zero
            refused(dev, E_INVALID_ARG, lambda raw, name=name: raw.null.add(name))
        refused(dev, E_INVALID_ARG, poke("status", 1, 2))
        refused(dev, E_INVALID_ARG, poke("tx_type", 2, 0x80))
        refused(dev, E_INVALID_ARG, poke("log_first", 1, 3))      # 0 3 2 3: goes backwards
        refused(dev, E_INVALID_ARG, poke("log_first", 0, 1))      # does not start at 0
        refused(dev, E_INVALID_ARG, poke("log_first", 3, 2))      # does not end at n_logs
        refused(dev, E_INVALID_ARG, count("n_logs", 2))
        refused(dev, E_INVALID_ARG, poke("topic_first", 1, 4))    # 0 4 3 3
        refused(dev, E_INVALID_ARG, poke("topic_first", 3, 2))
        refused(dev, E_INVALID_ARG, count("n_topics", 4))
        refused(dev, E_INVALID_ARG, poke("data_off", 1, 14))      # 0 14 13 13
        refused(dev, E_INVALID_ARG, poke("data_off", 3, 12))
        refused(dev, E_INVALID_ARG, count("data_bytes", 14))
        refused(dev, E_INVALID_ARG, lambda raw: setattr(raw, "at", 2), other=[txs])  # receipts_at > n_lists
        if dev:
            refused(dev, E_INVALID_ARG, lambda raw: raw.list_bytes.__setitem__(0, 119), other=[txs])
            refused(dev, E_INVALID_ARG, lambda raw: raw.other_off[0].__setitem__(1, 90), other=[txs])  # 0 90 80 120
        else:
            refused(dev, E_INVALID_ARG, lambda raw: raw.other_off[0].__setitem__(1, 90), other=[txs])

        # a receipt beyond 2^32 - 1 bytes: one log whose data_off claims 4 GiB (refused from the offsets alone; nothing is read)
        def huge(raw):
            one = [(0, True, 21000, [(b"\x11" * 20, [], b"\x80")])]
            fresh = Raw(P, one, dev=raw.dev)
            raw.arr, raw.n = fresh.arr, 1
            if not raw.dev:
                raw.arr = {k: v.copy() for k, v in raw.arr.items()}
            raw.counts = dict(fresh.counts, data_bytes=1 << 32)
            if raw.dev:
                raw.arr["data_off"][1] = 1 << 32
            else:
                raw.arr["data_off"][1] = 1 << 32
        refused(dev, E_UNSUPPORTED, huge)
    # the structs themselves
    from phant_amd import _lib as Lb
    arg = Lb.PhantReceiptsIn(C.sizeof(Lb.PhantReceiptsIn) - 4)
    out = Lb.PhantReceiptsOut(C.sizeof(Lb.PhantReceiptsOut))
    for fn in (L.phant_block_receipts, L.phant_block_receipts_dev):
        assert fn(ctx.handle, C.byref(arg), C.byref(out)) == E_INVALID_ARG
        assert fn(ctx.handle, None, C.byref(out)) == E_INVALID_ARG
        assert fn(ctx.handle, C.byref(Lb.PhantReceiptsIn(C.sizeof(Lb.PhantReceiptsIn))), None) == E_INVALID_ARG
        assert fn(ctx.handle, C.byref(Lb.PhantReceiptsIn(C.sizeof(Lb.PhantReceiptsIn))), C.byref(out)) == OK  # an empty block, nothing wanted
