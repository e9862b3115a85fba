"""Bloom screening of log filters on the device (phant_log_filters_bloom, phant_log_filters_bloom_dev,
phant_amd.types.receipt.bloom_candidates, phant_amd.types.block.candidate_blocks) against tests/filters_ref.py, which takes an entry's
three bits from the oracle's Keccak-256.  Every comparison is exact, in the host and the device form.  tests/test_emu_bloom_filters.py
runs the same bodies over the kernel sources compiled for the host."""
import ctypes as C

import numpy as np
import pytest

from tests import filters_ref as F
from tests import receipts_seg_ref as G
from tests.test_gpu_log_filters import ROWS, RawLF, addr, in_blocks, log, topic
from tests.test_gpu_requests import RawReq
from tests.test_gpu_transactions import OK, E_INVALID_ARG, E_UNSUPPORTED, _ctx

pytestmark = pytest.mark.gpu
# found by a search over the topics int(i).to_bytes(32, "big"), i < 5000, with the oracle's Keccak-256 (tests/filters_ref.py bloom_values):
COLLIDING = (1313).to_bytes(32, "big")    # its values are 1375, 1375, 1998: two bits, not three
IN_BYTE_0 = (2).to_bytes(32, "big")       # 87, 2042, 680: 2042 lies in the bloom's byte 0
IN_BYTE_255 = (109).to_bytes(32, "big")   # 6, 56, 124: 6 lies in the bloom's byte 255


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


class RawBloom:
    """phant_log_filters_bloom[_dev] over numpy arrays (host form) or torch tensors on the device"""

    def __init__(self, blooms, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.blooms = L, dev, torch, [bytes(b) for b in blooms]

    _up, _buf = RawReq._up, RawReq._buf

    def call(self, ctx, filters, want=("may", "may_count"), guard=64, size=None, reserved=0, skew=None, in_skew=0, over=None, ranges=True):
        """-> (rc, {output: bytes}); over: {n_blooms, n_filters, n_addr, n_topic, "blooms" or "f." + an array of the filters: value}"""
        L, nbl = self.L, len(self.blooms)
        fa, nf, n_addr, n_topic = F.pack(filters)
        if ranges:
            fa["block_lo"], fa["block_hi"] = F.ranges(filters, nbl)
        ins = dict({"f." + k: v for k, v in fa.items()}, blooms=np.frombuffer(b"".join(self.blooms) or b"\x00", np.uint8))
        counts = dict(n_blooms=nbl, n_filters=nf, n_addr=n_addr, n_topic=n_topic)
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k, dt in [("blooms", "u1")] + [("f." + k, dt) for k, dt in L.LOG_FILTER_ARRAYS]:
            a = None if ins[k] is None else np.ascontiguousarray(ins[k], dt)
            keep[k], ptr[k] = self._up(a, in_skew if dt == "u1" else 0)
        flt = L.PhantLogFilters(C.sizeof(L.PhantLogFilters) if size is None else size, counts["n_filters"], counts["n_addr"], counts["n_topic"],
                                *[ptr["f." + k] for k, _ in L.LOG_FILTER_ARRAYS], reserved)
        sizes = {"may": 8 * nf * ((nbl + 63) // 64), "may_count": 4 * nf}
        bufs = {k: self._buf(guard + (sizes[k] + 7) // 8 * 8 + guard) for k in want}
        out_ptr = lambda k: (bufs[k].data_ptr() if self.dev else bufs[k].ctypes.data) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        fn = ctx._lib.phant_log_filters_bloom_dev if self.dev else ctx._lib.phant_log_filters_bloom
        rc = fn(ctx.handle, ptr["blooms"], counts["n_blooms"], C.byref(flt), out_ptr("may"), out_ptr("may_count"))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + sizes[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + sizes[k]:] == 0xEE).all())
        del keep
        return rc, got


def check(P, blooms, filters, forms=(False, True), **kw):
    """both outputs against the definition in both forms -> may as an (n_filters, n_blooms) array of 0 / 1"""
    may, count = F.expected_may(blooms, filters)
    ctx = _ctx(P)
    for dev in forms:
        for want in (("may", "may_count"), ("may",), ("may_count",), ()):
            rc, got = RawBloom(blooms, dev=dev).call(ctx, filters, want=want, **kw)
            assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
            for k, exp in (("may", may), ("may_count", count)):
                if k in want:
                    assert got[k, "guards"], (dev, k)
                    assert got[k] == exp, (dev, k, want)
    words = np.frombuffer(may, "<u8").reshape(len(filters), -1)
    bits = np.unpackbits(words.view(np.uint8).reshape(len(filters), -1), axis=1, bitorder="little") if words.size else np.zeros((len(filters), 0), np.uint8)
    assert not bits[:, len(blooms):].any()  # (the padding bits)
    return bits[:, :len(blooms)]


def bloom_of_log(k):
    a, ts, _ = log(k)
    return F.bloom_of([a] + ts)


# --------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("nf", (1, 2, 65))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 130))
def test_blooms_against_filters(P, n, nf):
    """bloom b holds log b's address and topics: filter f asks for the addresses of a few logs and, every other filter, a topic; the
    padding bits of the last word are zero"""
    blooms = [bloom_of_log(b) for b in range(n)]
    filters = []
    for f in range(nf):
        ks = [(3 * f + 7 * j) % max(n, 1) for j in range(1 + f % 3)]
        filters.append(F.Filter([addr(k) for k in ks], [[], [topic(k, 1) for k in ks]] if f % 2 else (), lo=None if f % 4 else f % (n + 1), hi=None if f % 5 else n))
    bits = check(P, blooms, filters)
    if n:
        assert bits[0, 0] == 1 and bits.sum() >= nf // 2  # (filter 0 asks for log 0's address)


def test_full_and_empty_blooms_and_two_bits_of_three(P):
    """an all-ones bloom passes every filter, a zero bloom only the all-wildcard ones; a bloom with exactly two of an entry's three bits
    does not pass; an entry whose positions collide needs its two bits only; bits in the bloom's bytes 0 and 255"""
    a, t = addr(5), topic(9, 2)
    two_of_three = []
    for drop in range(3):
        b = bytearray(256)
        for i, (byte, mask) in enumerate(F.bloom_bits(a)):
            if i != drop:
                b[byte] |= mask
        two_of_three.append(bytes(b))
    assert len(set(F.bloom_bits(a))) == 3 and len(set(F.bloom_bits(COLLIDING))) == 2
    assert any(byte == 0 for byte, _ in F.bloom_bits(IN_BYTE_0)) and any(byte == 255 for byte, _ in F.bloom_bits(IN_BYTE_255))
    one_bit = bytearray(256)
    one_bit[F.bloom_bits(COLLIDING)[0][0]] |= F.bloom_bits(COLLIDING)[0][1]
    blooms = [b"\xff" * 256, bytes(256), F.bloom_of([a])] + two_of_three + [F.bloom_of([a, t]), F.bloom_of([COLLIDING]), bytes(one_bit), F.bloom_of([IN_BYTE_0]),
                                                                           F.bloom_of([IN_BYTE_255]), F.bloom_of([IN_BYTE_0, IN_BYTE_255])]
    filters = [F.Filter(), F.Filter([a]), F.Filter([], [[], [], [t]]), F.Filter([a], [[t]]), F.Filter([addr(6), a]), F.Filter([], [[COLLIDING]]),
               F.Filter([], [[IN_BYTE_0]]), F.Filter([], [[], [], [], [IN_BYTE_255]]), F.Filter([], [[IN_BYTE_0], [IN_BYTE_255]]), F.Filter([], [[], []], lo=1, hi=2)]
    bits = check(P, blooms, filters)
    assert bits[:-1, 0].all() and bits[:, 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1] and bits[-1].sum() == 1
    assert bits[1].tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and bits[3].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert bits[5].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert bits[6, 9] and bits[7, 10] and bits[8].tolist() == [1] + [0] * 10 + [1]


def test_ranges_over_blooms(P):
    """all-ones blooms: a filter's candidates are exactly its range -- ranges inside one word, across words, empty, NULL"""
    blooms = [b"\xff" * 256] * 130
    ranges_ = [(0, 130), (0, 0), (63, 65), (64, 64), (64, 128), (129, 130), (130, 130), (1, 129), (None, None), (None, 64), (128, None)]
    filters = [F.Filter([addr(f)], lo=lo, hi=hi) for f, (lo, hi) in enumerate(ranges_)]
    bits = check(P, blooms, filters)
    for f, (lo, hi) in enumerate(ranges_):
        assert np.flatnonzero(bits[f]).tolist() == list(range(lo or 0, 130 if hi is None else hi)), f
    for dev in (False, True):
        rc, got = RawBloom(blooms, dev=dev).call(_ctx(P), [F.Filter(), F.Filter([addr(1)])], ranges=False)
        assert rc == OK and np.frombuffer(got["may_count"], "<u4").tolist() == [130, 130]
    for dev in (False, True):  # the blooms at an odd address, in an allocation that ends with them
        rc, got = RawBloom(blooms[:65], dev=dev).call(_ctx(P), filters[8:9], in_skew=1)
        assert rc == OK and np.frombuffer(got["may_count"], "<u4").tolist() == [65]


def test_no_false_negatives_against_the_exact_call(P):
    """a segment's block blooms as phant_block_receipt_segments computes them: every block that holds an exact match of
    phant_block_log_filters is a candidate of the same filter, through candidate_blocks and through the raw call"""
    T = P.types.receipt
    from tests.test_gpu_receipt_segments import _enc, _plain
    logs = [log(k) for k in range(90)]
    blocks = in_blocks(logs, [7, None, 0, 20, 1, 30, 32])
    segs = T.receipt_segments(T.pack_receipt_segments(_enc([[_plain(i, logs=ls) for i, ls in enumerate(b)] for b in blocks], G.ETH69)), form=G.ETH69, roots=False, logs=True)
    blooms = [bytes(b) for b in np.asarray(segs.logs_bloom, np.uint8).reshape(-1, 256)]
    assert blooms[0] == F.bloom_of([x for a, ts, _ in logs[:7] for x in [a] + ts]) and blooms[1] == blooms[2] == bytes(256)
    ref = [F.Filter([addr(k)]) for k in range(0, 90, 9)] + [F.Filter([], [[], [topic(k, 1) for k in (3, 44, 89)]]), F.Filter([addr(2), addr(50)], [[topic(2, 0), topic(50, 0)]]),
                                                            F.Filter(), F.Filter([b"\x99" * 20]), F.Filter([addr(8)], lo=0, hi=3), F.Filter([addr(8)], lo=3, hi=4)]
    rows = {k: getattr(segs, k) for k in ROWS}
    exp, _ = F.expected_matches(rows, ref)
    match, first = np.frombuffer(exp["match_log"], "<u4"), np.frombuffer(exp["filter_first"], "<u4")
    rc, got, _ = RawLF(rows).call(_ctx(P), ref)
    assert rc == OK and got["match_log"] == exp["match_log"]
    block_of_log = np.searchsorted(np.asarray(segs.log_first)[np.asarray(segs.block_first)], np.arange(90), side="right") - 1
    bits = check(P, blooms, ref)
    for f in range(len(ref)):
        hit = set(block_of_log[match[first[f]:first[f + 1]]].tolist())
        assert hit <= set(np.flatnonzero(bits[f]).tolist()), f
    assert bits[-4].tolist() == [1] * 7 and not bits[-3].any() and not bits[-2].any() and bits[-1].tolist() == [0, 0, 0, 1, 0, 0, 0]
    filters = [T.LogFilter(f.addresses, f.topics, f.lo, f.hi) for f in ref]
    cand = P.types.block.candidate_blocks({"logs_bloom": segs.logs_bloom}, filters)
    assert [c.tolist() for c in cand] == [np.flatnonzero(row).tolist() for row in bits]
    import torch
    may, count = T.bloom_candidates(torch.from_numpy(np.frombuffer(b"".join(blooms), np.uint8).copy()).cuda(), filters)
    assert count.cpu().numpy().view(np.uint32).tolist() == bits.sum(axis=1).tolist() and may.cpu().numpy().view(np.uint64).tobytes() == F.expected_may(blooms, ref)[0]


def test_refused_arguments(P):
    """each returns PHANT_E_INVALID_ARG and touches nothing; in the device form the firsts and the ranges are caught by the checking kernel"""
    ctx = _ctx(P)
    blooms = [bloom_of_log(b) for b in range(5)]
    filters = [F.Filter([addr(1), addr(2)], [[topic(1, 0)], [], [topic(2, 2), topic(3, 2)]]), F.Filter(lo=1, hi=3), F.Filter([addr(4)], [[], [topic(4, 1)]])]
    fa, nf, n_addr, n_topic = F.pack(filters)
    lo, hi = F.ranges(filters, 5)
    size = C.sizeof(__import__("phant_amd")._lib.PhantLogFilters)

    def refused(raw, **kw):
        rc, got = raw.call(ctx, filters, **kw)
        assert rc == E_INVALID_ARG, (rc, kw)
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawBloom(blooms, dev=dev)
        assert raw.call(ctx, filters)[0] == OK
        refused(raw, size=size - 8)
        refused(raw, size=size + 8)
        refused(raw, reserved=1)
        for k in ("blooms", "f.addr_first", "f.addr", "f.topic_first", "f.topic"):
            refused(raw, over={k: None})
        refused(raw, over={"n_addr": n_addr - 1})
        refused(raw, over={"n_topic": n_topic + 1})
        refused(raw, over={"n_filters": 0})
        for k, a in (("f.addr_first", fa["addr_first"]), ("f.topic_first", fa["topic_first"])):
            for at, by in ((0, 1), (1, 100), (-1, 1), (-1, -1)):
                lie = np.array(a).copy()
                lie[at] = (int(lie[at + 1]) + 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
                refused(raw, over={k: lie})
        for i in range(nf):
            refused(raw, over={"f.block_hi": np.where(np.arange(nf) == i, 6, hi)})          # above n_blooms
            refused(raw, over={"f.block_lo": np.where(np.arange(nf) == i, hi[i] + 1, lo)})  # above its block_hi
        refused(raw, over={"n_blooms": 2})  # (a range that ends behind the blooms)
    dev = RawBloom(blooms, dev=True)
    refused(dev, skew={"may": 4})
    refused(dev, skew={"may_count": 2})
    for form_dev in (False, True):
        rc, got = RawBloom(blooms, dev=form_dev).call(ctx, [])  # no filter: nothing at all
        assert rc == OK and got["may"] == got["may_count"] == b""
        rc, got = RawBloom([], dev=form_dev).call(ctx, [F.Filter(), F.Filter([addr(1)])])  # no bloom: zero counts
        assert rc == OK and got["may"] == b"" and got["may_count"] == bytes(8) and got["may_count", "guards"]
    one = np.zeros(4, np.uint32)
    L = __import__("phant_amd")._lib
    flt = L.PhantLogFilters(size, 1 << 29, 0, 0, one.ctypes.data, None, one.ctypes.data, None, None, None, 0)
    assert ctx._lib.phant_log_filters_bloom_dev(ctx.handle, one.ctypes.data, 256, C.byref(flt), None, None) == E_UNSUPPORTED
