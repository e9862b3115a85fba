"""Log filters over chain segments on the device (phant_block_log_filters, phant_block_log_filters_dev,
phant_amd.types.receipt.filter_logs) against tests/filters_ref.py, which defines every output from the rules of include/phant_gpu.h with
set membership on bytes.  Every comparison is exact, in the host and the device form.  The rows of the logs come out of a real
receipt_segments call over receipts in both wire forms, and once they are packed by hand.  tests/test_emu_log_filters.py runs the same
bodies over the kernel sources compiled for the host."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import filters_ref as F
from tests import receipts_seg_ref as G
from tests import requests_ref as Q
from tests.test_gpu_requests import CONTRACT, RawReq, dlog, rows_by_hand, rows_of
from tests.test_gpu_transactions import OK, E_INVALID_ARG, E_UNSUPPORTED, _ctx, _first_difference

pytestmark = pytest.mark.gpu
FORMS = (G.CONSENSUS, G.ETH69)
ROWS = ("block_first", "log_first", "address", "topic_first", "topics")
UNTOUCHED = 0xEEEEEEEE
SETS = {"default": 0, "table": 1, "linear": 2}  # PHANT_DIAG_LOGFILTER_SETS


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def LINEAR_MAX():
    from phant_amd import _lib as L
    return L.LOGFILTER_LINEAR_MAX


@contextlib.contextmanager
def forced(ctx, sets):
    ctx.diag_set("logfilter_sets", SETS[sets])
    try:
        yield
    finally:
        ctx.diag_set("logfilter_sets", 0)


# ------------------------------------------------------------------------------------------------------------- the logs
def addr(k):
    return bytes((7 * k + 3 * i + 1) % 256 for i in range(20))


def topic(k, p=0):
    return bytes((13 * k + 5 * p + 11 * i + 2) % 256 for i in range(32))


def log(k, n_topics=None):
    """log k: its own address, k % 5 topics (or n_topics) of its own"""
    return (addr(k), [topic(k, p) for p in range(k % 5 if n_topics is None else n_topics)], b"d" * (k % 3))


def in_blocks(logs, sizes):
    """the logs as blocks of one receipt each (a size of None: a block without a receipt; 0: a receipt without logs)"""
    out, at = [], 0
    for s in sizes:
        out.append([] if s is None else [logs[at:at + s]])
        at += s or 0
    assert at == len(logs)
    return out


def spread(logs):
    """... in blocks of 0, 1, 2, ... logs until they are used up"""
    sizes, left = [], len(logs)
    while left:
        sizes.append(min(left, len(sizes) % 7 * 5))
        left -= sizes[-1]
    return in_blocks(logs, sizes + [None, 0])


_ROWS = {}


def feeds(P, blocks, key=None):
    """the rows of the logs three times: from a real receipt_segments call in both wire forms, and packed by hand (kept per key)"""
    if key is not None and key in _ROWS:
        return _ROWS[key]
    out = [{k: v for k, v in rows_of(P, blocks, form).items() if k in ROWS} for form in FORMS] + [{k: v for k, v in rows_by_hand(blocks).items() if k in ROWS}]
    for r in out[:2]:
        assert all(np.asarray(r[k]).tobytes() == np.asarray(out[2][k]).tobytes() for k in ROWS)
    if key is not None:
        _ROWS[key] = out
    return out


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawLF:
    """phant_logmatch_in / phant_log_filters / phant_logmatch_out over numpy arrays (host form) or torch tensors on the device"""

    def __init__(self, rows, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.rows = L, dev, torch, rows
        self.nb, self.n, self.nl, self.nt = len(rows["block_first"]) - 1, len(rows["log_first"]) - 1, len(rows["topic_first"]) - 1, len(np.asarray(rows["topics"]).reshape(-1, 32))

    _up, _buf = RawReq._up, RawReq._buf

    def call(self, ctx, filters, want=None, match_cap=None, guard=64, sizes=None, reserved=(0, 0, 0, 0, 0), skew=None, in_skew=0, over=None, ranges=True):
        """-> (rc, {output: bytes}, n_matches); every buffer has `guard` bytes of 0xEE in front of and behind its rows.  over: {a count, a
        row array, or "f." + an array of the filters: value} put in last (an array is uploaded, None passes NULL); ranges=False: NULL
        block_lo / block_hi; in_skew: bytes the byte arrays of the inputs are moved up by"""
        L = self.L
        want = F.MATCH_OUTPUTS if want is None else want
        fa, nf, n_addr, n_topic = F.pack(filters)
        if ranges:
            fa["block_lo"], fa["block_hi"] = F.ranges(filters, self.nb)
        ins = dict(self.rows, **{"f." + k: v for k, v in fa.items()})
        counts = dict(n_blocks=self.nb, n=self.n, n_logs=self.nl, n_topics=self.nt, n_filters=nf, n_addr=n_addr, n_topic=n_topic,
                      match_cap=F.expected_matches(self.rows, filters)[1] if match_cap is None else match_cap)
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k, dt in [(k, dt) for k, dt in L.LOGMATCH_INPUTS] + [("f." + k, dt) for k, dt in L.LOG_FILTER_ARRAYS]:
            a = None if ins[k] is None else np.ascontiguousarray(ins[k], dt)
            keep[k], ptr[k] = self._up(a, in_skew if dt == "u1" else 0)
        flt = L.PhantLogFilters(C.sizeof(L.PhantLogFilters), counts["n_filters"], counts["n_addr"], counts["n_topic"], *[ptr["f." + k] for k, _ in L.LOG_FILTER_ARRAYS], reserved[4])
        arg = L.PhantLogMatchIn(C.sizeof(L.PhantLogMatchIn), counts["n_blocks"], counts["n"], counts["n_logs"], counts["n_topics"], counts["match_cap"], reserved[0], reserved[1],
                                *[ptr[k] for k, _ in L.LOGMATCH_INPUTS])
        rows = {"filter_first": nf + 1, "match_log": counts["match_cap"], "filter_count": nf}
        size = {k: 4 * rows[k] for k in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out_ptr = lambda k: (bufs[k].data_ptr() if self.dev else bufs[k].ctypes.data) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        out = L.PhantLogMatchOut(C.sizeof(L.PhantLogMatchOut), UNTOUCHED, reserved[2], reserved[3], *[out_ptr(k) for k in L.LOGMATCH_OUTPUTS])
        if sizes:
            arg.struct_size, flt.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_log_filters_dev if self.dev else ctx._lib.phant_block_log_filters
        rc = fn(ctx.handle, C.byref(arg), C.byref(flt), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        del keep
        return rc, got, int(out.n_matches)


def check(P, rows, filters, forms=(False, True), sets=("default",), ctx=None, **kw):
    """every answer of the call against the definition, in both forms and under each way to compare a set -> (match_log, filter_first)"""
    exp, nm = F.expected_matches(rows, filters)
    ctx = ctx or _ctx(P)
    for how in sets:
        with forced(ctx, how):
            for dev in forms:
                rc, got, n_matches = RawLF(rows, dev=dev).call(ctx, filters, **kw)
                assert rc == OK, (dev, how, ctx._lib.phant_last_error(ctx.handle))
                assert n_matches == nm, (dev, how, n_matches, nm)
                for k in (k for k in got if isinstance(k, str)):
                    assert got[k, "guards"], (dev, how, k)
                    assert got[k] == exp[k], (dev, how, k, _first_difference(got[k], exp[k], 4))
    return np.frombuffer(exp["match_log"], "<u4").tolist(), np.frombuffer(exp["filter_first"], "<u4").tolist()


# ------------------------------------------------------------------------------------------------------------- sizes
def filters_for(logs, nf, nb):
    """nf filters over these logs: wildcards, single addresses, topic sets, both, ranges -- each selects something where there are logs"""
    out = []
    for i in range(nf):
        k = (5 * i + 1) % max(len(logs), 1)
        some = logs[k] if logs else log(0, 2)
        kind = i % 6
        if kind == 0:
            out.append(F.Filter())
        elif kind == 1:
            out.append(F.Filter([some[0]]))
        elif kind == 2:
            out.append(F.Filter([], [[topic(j, 0) for j in range(k, k + 3)]]))
        elif kind == 3:
            out.append(F.Filter([addr(j) for j in range(k, k + 4)], [[], [topic(j, 1) for j in range(k, k + 4)]]))
        elif kind == 4:
            out.append(F.Filter(lo=i % (nb + 1), hi=nb))
        else:
            out.append(F.Filter([addr(j) for j in range(0, len(logs), 2)], lo=0, hi=(i + 1) % (nb + 1)))
    return out


@pytest.mark.parametrize("nf", (1, 2, 65))
@pytest.mark.parametrize("nl", (0, 1, 63, 64, 65, 129))
def test_logs_against_filters(P, nl, nf):
    """n_logs around the 64 logs of a wave against one, two and more filters than a wave has lanes; the rows from a real call over both
    wire forms and packed by hand"""
    logs = [log(k) for k in range(nl)]
    blocks = spread(logs)
    filters = filters_for(logs, nf, len(blocks))
    for rows in feeds(P, blocks, key=("sizes", nl)):
        match, first = check(P, rows, filters)
        assert first[1] == nl and len(match) >= nl  # (the first filter is the wildcard)


def test_matches_on_wave_edges_and_filter_boundaries(P):
    """matches in the first and the last lane of each wave of 130 logs, a filter without a match between two with matches, and a filter
    whose only match is the call's last log"""
    logs = [log(k) for k in range(130)]
    edge = [0, 63, 64, 127, 128, 129]
    filters = [F.Filter([addr(k) for k in edge]), F.Filter([addr(500)]), F.Filter([addr(63), addr(64)]), F.Filter([], [[], [], [], [topic(129, 3)]]),
               F.Filter([addr(0)]), F.Filter([addr(129)], [[topic(129, 0)]])]
    for rows in feeds(P, spread(logs), key="edges"):
        match, first = check(P, rows, filters, sets=SETS)
        assert match == edge + [63, 64, 129, 0, 129] and first == [0, 6, 6, 8, 9, 10, 11]


def test_blocks_ranges_and_waves_that_leave_early(P):
    """192 logs: a block that ends on log 64, an empty block, one of 63 logs, one of a single log (the last lane of the second wave), a block
    with an empty receipt, 64 logs.  Ranges of one block, of the empty block alone, lo == hi, ranges that end on an empty block, the
    whole segment: for [3, 4) the first and the third wave leave early and the second keeps a single lane"""
    logs = [log(k) for k in range(192)]
    blocks = in_blocks(logs, [64, None, 63, 1, 0, 64])
    ranges_ = [(0, 1), (3, 4), (1, 2), (2, 2), (0, 5), (3, 5), (4, 5), (5, 6), (0, 6), (6, 6), (0, 0), (2, 4)]
    filters = [F.Filter(lo=lo, hi=hi) for lo, hi in ranges_] + [F.Filter([addr(127), addr(5), addr(128)], lo=3, hi=4), F.Filter([addr(127), addr(5), addr(128)], lo=0, hi=3)]
    for rows in feeds(P, blocks, key="ranges"):
        match, first = check(P, rows, filters, sets=SETS)
        counts = np.diff(first).tolist()
        assert counts == [64, 1, 0, 0, 128, 1, 0, 64, 192, 0, 0, 64, 1, 1]
        assert match[64] == 127 and match[-2:] == [127, 5]
    # NULL ranges: every block
    rows = feeds(P, blocks, key="ranges")[2]
    for dev in (False, True):
        rc, got, nm = RawLF(rows, dev=dev).call(_ctx(P), [F.Filter(), F.Filter([addr(191)])], ranges=False, match_cap=193)
        assert rc == OK and nm == 193 and np.frombuffer(got["filter_first"], "<u4").tolist() == [0, 192, 193]


# ---------------------------------------------------------------------------------------------------- what must not match
def test_near_misses_positions_and_wildcards(P):
    """entries that differ from a log's address or topic in the first byte only and in the last byte only; an address entry equal to the
    first 20 bytes of a topic; a position-1 topic offered to the position-0 set; a log with p topics against a filter that constrains
    position p; the all-wildcard filter -- under each way to compare a set"""
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]  # noqa: E731
    logs = [log(k, n_topics=k % 5) for k in range(10)] + [(topic(3, 0)[:20], [topic(3, 0), topic(3, 1)], b"")]
    a, t0, t1 = addr(7), topic(7, 0), topic(7, 1)  # (log 7 has two topics)
    filters = [F.Filter([a]), F.Filter([flip(a, 0)]), F.Filter([flip(a, 19)]), F.Filter([flip(a, 0), a, flip(a, 19)]),
               F.Filter([], [[t0]]), F.Filter([], [[flip(t0, 0)]]), F.Filter([], [[flip(t0, 31)]]), F.Filter([], [[flip(t0, 0), flip(t0, 31)], [t1]]),
               F.Filter([topic(3, 0)[:20]]),                       # the address that is a topic's first 20 bytes: log 10 alone, not log 3
               F.Filter([], [[addr(3) + bytes(12)]]),              # a topic entry that begins with an address
               F.Filter([], [[t1]]), F.Filter([], [[], [t1]]),     # a position-1 topic offered to position 0, and to position 1
               F.Filter([], [[t1, t0]]), F.Filter([], [[t0], [t0]]),
               F.Filter()]
    filters += [F.Filter([addr(k)], [[]] * p + [[topic(k, p)]]) for p in range(4) for k in (p, p + 1, p + 5)]  # (k % 5 == p: the log has p topics)
    for rows in feeds(P, [[logs[:4], logs[4:]]], key="near"):
        match, first = check(P, rows, filters, sets=SETS)
        counts = np.diff(first).tolist()
        assert counts[:15] == [1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1, 1, 0, 11]
        assert match[first[8]] == 10
        assert counts[15:] == [0, 1, 0] * 4


def test_set_sizes_around_the_threshold_and_a_set_of_copies(P):
    """sets of LINEAR_MAX - 1, LINEAR_MAX and LINEAR_MAX + 1 entries, addresses and topics, the value that matches last, first or absent;
    a set of 200 copies of one value -- each with every set through the table, every set entry by entry, and the default"""
    m = LINEAR_MAX()
    logs = [log(k, n_topics=2) for k in range(70)]
    filters = []
    for size in (m - 1, m, m + 1):
        others = [addr(1000 + j) for j in range(size - 1)]
        tothers = [topic(1000 + j, 1) for j in range(size - 1)]
        filters += [F.Filter(others + [addr(69)]), F.Filter([addr(0)] + others), F.Filter(others + [addr(2000)]), F.Filter([], [[], tothers + [topic(64, 1)]]),
                    F.Filter(others + [addr(5)], [[topic(5, 0)] + [topic(3000 + j, 0) for j in range(size - 1)], tothers + [topic(5, 1)]]),
                    F.Filter(others + [addr(5)], [tothers + [topic(5, 1)]])]  # (position 1's value in position 0's set)
    filters += [F.Filter([addr(33)] * 200), F.Filter([addr(34)] * 200, [[topic(34, 0)] * 200]), F.Filter([], [[], [b"\xab" * 32] * 200]),
                F.Filter([addr(j) for j in range(40, 240)])]
    for rows in feeds(P, spread(logs), key="sets")[1:]:
        match, first = check(P, rows, filters, sets=SETS)
        assert np.diff(first).tolist() == [1, 1, 0, 1, 1, 0] * 3 + [1, 1, 0, 30]


def test_the_deposit_filter_selects_the_candidates_of_block_requests(P):
    """the deposit contract's address plus the DepositEvent topic: exactly the logs phant_block_requests turns into deposit rows on the
    same rows (every candidate here is well-formed)"""
    logs = [dlog(k) if k % 4 == 1 else dlog(k, address=b"\x22" * 20) if k % 4 == 2 else dlog(k, topics=[b"\x11" * 32, Q.DEPOSIT_TOPIC]) if k % 4 == 3 else log(k) for k in range(70)]
    blocks = in_blocks(logs, [30, 0, 40])
    full = rows_of(P, blocks)
    rc, got, (nd, _) = RawReq(full).call(_ctx(P), want=("deposit_log",))
    assert rc == OK and nd == 18
    match, first = check(P, {k: full[k] for k in ROWS}, [F.Filter([CONTRACT], [[Q.DEPOSIT_TOPIC]])], sets=SETS)
    assert match == np.frombuffer(got["deposit_log"], "<u4")[:nd].tolist() == list(range(1, 70, 4))


# --------------------------------------------------------------------------------------------------- outputs and buffers
def test_subsets_of_the_outputs_a_short_cap_and_odd_addresses(P):
    """every subset of the outputs NULL; match_cap one short and 0: match_log keeps its 0xEE bytes and the counts are complete; the byte
    arrays of the inputs at odd addresses in allocations that end with them; the word outputs cannot be odd in the device form only"""
    logs = [log(k) for k in range(70)]
    filters = [F.Filter([addr(3), addr(64)]), F.Filter(lo=1, hi=2), F.Filter([], [[topic(k, 0) for k in range(60, 80)]])]
    rows = feeds(P, in_blocks(logs, [10, 50, 10]), key="outputs")[0]
    exp, nm = F.expected_matches(rows, filters)
    assert nm == 2 + 50 + 8
    ctx = _ctx(P)
    for dev in (False, True):
        raw = RawLF(rows, dev=dev)
        for mask in range(8):
            want = tuple(k for i, k in enumerate(F.MATCH_OUTPUTS) if mask >> i & 1)
            rc, got, n_matches = raw.call(ctx, filters, want=want)
            assert rc == OK and n_matches == nm, (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
        for cap in (nm - 1, 0):
            rc, got, n_matches = raw.call(ctx, filters, match_cap=cap)
            assert rc == OK and n_matches == nm, (dev, cap)
            assert all(got[k, "guards"] for k in F.MATCH_OUTPUTS) and set(got["match_log"]) <= {0xEE}, (dev, cap)
            assert got["filter_first"] == exp["filter_first"] and got["filter_count"] == exp["filter_count"], (dev, cap)
        rc, got, n_matches = raw.call(ctx, filters, match_cap=nm + 5)  # (room to spare: the rows behind n_matches stay untouched)
        assert rc == OK and n_matches == nm and got["match_log"] == exp["match_log"] + b"\xee" * 20 and got["match_log", "guards"]
        for in_skew in (1, 3):
            for how in SETS:
                with forced(ctx, how):
                    rc, got, n_matches = raw.call(ctx, filters, in_skew=in_skew)
                    assert rc == OK and n_matches == nm and all(got[k, "guards"] and got[k] == exp[k] for k in F.MATCH_OUTPUTS), (dev, in_skew, how)
    rc, got, n_matches = RawLF(rows).call(ctx, filters, skew={"match_log": 1, "filter_first": 3, "filter_count": 2})  # (the host form copies bytes)
    assert rc == OK and all(got[k, "guards"] and got[k] == exp[k] for k in F.MATCH_OUTPUTS)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments(P):
    """each returns PHANT_E_INVALID_ARG and touches nothing; in the device form the firsts and the ranges are caught by the checking kernel"""
    ctx = _ctx(P)
    logs = [log(k) for k in range(9)]
    rows = feeds(P, in_blocks(logs, [4, None, 0, 5]), key="refused")[0]
    filters = [F.Filter([addr(1), addr(2)], [[topic(1, 0)], [], [topic(2, 2), topic(3, 2)]]), F.Filter(lo=1, hi=3), F.Filter([addr(8)], [[], [topic(8, 1)]])]
    fa, nf, n_addr, n_topic = F.pack(filters)
    lo, hi = F.ranges(filters, 4)
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantLogMatchIn), C.sizeof(L.PhantLogFilters), C.sizeof(L.PhantLogMatchOut))

    def refused(raw, **kw):
        rc, got, n_matches = raw.call(ctx, filters, match_cap=20, **kw)
        assert rc == E_INVALID_ARG, (rc, kw)
        assert n_matches == UNTOUCHED, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawLF(rows, dev=dev)
        rc, _, nm = raw.call(ctx, filters)
        assert rc == OK and nm == F.expected_matches(rows, filters)[1]
        for k in range(3):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        for k in range(5):
            refused(raw, reserved=tuple(1 if i == k else 0 for i in range(5)))
        for k in ROWS + ("f.addr_first", "f.addr", "f.topic_first", "f.topic"):
            refused(raw, over={k: None})
        refused(raw, over={"n_blocks": 0})
        refused(raw, over={"n": raw.n - 1})
        refused(raw, over={"n_logs": raw.nl - 1})
        refused(raw, over={"n_topics": raw.nt + 1})
        refused(raw, over={"n_addr": n_addr - 1})
        refused(raw, over={"n_topic": n_topic + 1})
        refused(raw, over={"n_filters": 0})  # (entries without a filter)
        for k, a in (("block_first", rows["block_first"]), ("log_first", rows["log_first"]), ("topic_first", rows["topic_first"]), ("f.addr_first", fa["addr_first"]),
                     ("f.topic_first", fa["topic_first"])):
            for at, by in ((0, 1), (1, 100), (-1, 1), (-1, -1)):
                lie = np.array(a).copy()
                lie[at] = (int(lie[at + 1]) + 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
                refused(raw, over={k: lie})
        for i in range(nf):
            refused(raw, over={"f.block_hi": np.where(np.arange(nf) == i, 5, hi)})          # above n_blocks
            refused(raw, over={"f.block_lo": np.where(np.arange(nf) == i, hi[i] + 1, lo)})  # above its block_hi
        refused(raw, over={"f.block_lo": np.full(nf, 5), "f.block_hi": None})
    dev = RawLF(rows, dev=True)
    for k, by in (("match_log", 2), ("filter_first", 1), ("filter_count", 3)):
        refused(dev, skew={k: by})
    for form_dev in (False, True):
        # no filter: the scalar alone; no block and no log: zero counts
        rc, got, nm = RawLF(rows, dev=form_dev).call(ctx, [], match_cap=4)
        assert rc == OK and nm == 0 and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str))
        for empty in (rows_by_hand([]), rows_by_hand([[], [[]]])):
            rc, got, nm = RawLF({k: empty[k] for k in ROWS}, dev=form_dev).call(ctx, [F.Filter(), F.Filter([addr(1)])], match_cap=4)
            assert rc == OK and nm == 0 and got["filter_first"] == bytes(12) and got["filter_count"] == bytes(8) and set(got["match_log"]) <= {0xEE}


def test_too_many_ballots_is_unsupported(P):
    """n_filters x ceil(n_logs / 64) >= 2^31: refused from the counts alone, before anything is read or sized"""
    ctx = _ctx(P)
    L = __import__("phant_amd")._lib
    one = np.zeros(4, np.uint32)
    flt = L.PhantLogFilters(C.sizeof(L.PhantLogFilters), 1 << 29, 0, 0, one.ctypes.data, None, one.ctypes.data, None, None, None, 0)
    arg = L.PhantLogMatchIn(C.sizeof(L.PhantLogMatchIn), 1, 1, 256, 0, 0, 0, 0, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, None)
    out = L.PhantLogMatchOut(C.sizeof(L.PhantLogMatchOut), UNTOUCHED, 0, 0, None, None, None)
    assert ctx._lib.phant_block_log_filters_dev(ctx.handle, C.byref(arg), C.byref(flt), C.byref(out)) == E_UNSUPPORTED and out.n_matches == UNTOUCHED


# ------------------------------------------------------------------------------------------------------- the layers above
def test_filter_logs_on_host_arrays_and_device_tensors(P):
    """receipt.filter_logs over what receipt_segments returns, and over the same rows as tensors on the device: each filter's logs in
    chain order; a cap that the first call outgrows"""
    import torch
    T = P.types.receipt
    logs = [log(k % 7) for k in range(400)]
    blocks = in_blocks(logs, [100, 300])
    from tests.test_gpu_receipt_segments import _enc, _plain
    segs = T.receipt_segments(T.pack_receipt_segments(_enc([[_plain(i, logs=ls) for i, ls in enumerate(b)] for b in blocks], G.ETH69)), form=G.ETH69, roots=False, logs=True)
    filters = [T.LogFilter([addr(1)]), T.LogFilter([], [[topic(2, 0), topic(3, 0)]], from_block=1), T.LogFilter(to_block=1), T.LogFilter([addr(9)])] + [T.LogFilter()] * 9
    ref = [F.Filter(f.addresses, f.topics, f.from_block, f.to_block) for f in filters]
    exp, nm = F.expected_matches({k: getattr(segs, k) for k in ROWS}, ref)
    m = T.filter_logs(segs, filters)
    assert m.n_matches == nm > 4 * 400 and m.match_log.tobytes() == exp["match_log"] and m.filter_first.tobytes() == exp["filter_first"]
    assert m.logs(0).tolist() == list(range(1, 400, 7)) and m.logs(3).tolist() == []
    dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(segs, k))).cuda() for k in ROWS}
    d = T.filter_logs(dev, filters)
    assert d.n_matches == nm and d.match_log.cpu().numpy().view(np.uint32).tobytes() == exp["match_log"]
    assert d.filter_count.cpu().numpy().view(np.uint32).tobytes() == exp["filter_count"]
    with pytest.raises(ValueError):
        T.filter_logs(T.receipt_segments(T.pack_receipt_segments([[]]), roots=False, logs=False), filters)
