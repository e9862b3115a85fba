"""Receipts of chain segments from raw messages on the device (phant_block_receipt_segments, phant_block_receipt_segments_dev,
phant_amd.types.receipt.receipt_segments, phant_amd.types.block.validate_receipts) against tests/receipts_seg_ref.py, which defines every
output from the rules of include/phant_gpu.h, and against phant_block_receipts for one block.  Every comparison is exact, in the host and
the device form and in both wire forms.  tests/test_emu_receipt_segments.py runs the same bodies over the kernel sources compiled for the
host."""
import ctypes as C

import numpy as np
import pytest

from tests import receipts_ref as R
from tests import receipts_seg_ref as G
from tests import suite
from tests.test_gpu_transactions import OK, E_INVALID_ARG, E_UNSUPPORTED, _ctx, _data, _first_difference

pytestmark = pytest.mark.gpu
WIDTH = G.WIDTH
FORMS = (G.CONSENSUS, G.ETH69)
SCALARS_UNTOUCHED = (0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE)
VALUES = (0x00, 0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8, 0xFF)


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawSegs:
    """phant_rcpt_segs_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, blocks, form, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.form = L, dev, torch, form
        self.host = P.types.receipt.pack_receipt_segments(blocks)
        self.nb, self.n, self.rc_bytes = len(blocks), len(self.host["rc_off"]) - 1, int(self.host["rc_off"][-1])
        self.host["receipts"] = self.host["receipts"][:self.rc_bytes]

    def _up(self, a, skew=0):
        """-> (something that keeps the memory alive, its address): the array `skew` bytes into an allocation that ENDS with it, so that a
        read behind the last byte leaves the allocation"""
        if a is None:
            return None, None
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.concatenate([np.zeros(skew, np.uint8), raw])
        if not len(buf):
            buf = np.zeros(1, np.uint8)
        if not self.dev:
            return buf, buf.ctypes.data + skew
        t = self.torch.from_numpy(buf).cuda()
        return t, t.data_ptr() + skew

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def _ptr(self, x):
        return x.data_ptr() if self.dev else x.ctypes.data

    def call(self, ctx, exp_root=None, exp_bloom=None, exp_gas=None, exp_count=None, want=None, log_cap=0, topic_cap=0, encoded_cap=0, guard=64, sizes=None,
             reserved=(0, 0), form=None, skew=None, in_skew=0, over=None):
        """-> (rc, {output: bytes}, (first_bad_block, n_logs, n_topics, encoded_len)); every buffer has `guard` bytes of 0xEE in front of and
        behind its rows.  The expected values are lists with a value per block.  over: {field of phant_rcpt_segs_in: value} put in last (an
        array value is uploaded); in_skew: bytes the byte arrays of the inputs are moved up by"""
        L, nb, n = self.L, self.nb, self.n
        want = G.OUTPUTS if want is None else want
        ins = dict(self.host)
        ins.update(receipts_root=None if exp_root is None else np.frombuffer(b"".join(exp_root) or bytes(32), np.uint8),
                   logs_bloom=None if exp_bloom is None else np.frombuffer(b"".join(exp_bloom) or bytes(256), np.uint8),
                   gas_used=None if exp_gas is None else np.asarray(list(exp_gas) or [0], np.uint64), tx_count=None if exp_count is None else np.asarray(list(exp_count) or [0], np.uint32))
        counts = dict(n=n, n_blocks=nb, rc_bytes=self.rc_bytes)
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k in L.RSEG_INPUTS:
            byte_array = ins[k] is not None and np.asarray(ins[k]).dtype == np.uint8
            keep[k], ptr[k] = self._up(ins[k], in_skew if byte_array else 0)
        for k in ("receipts", "rc_off"):  # (never-empty stand-ins: a zero count passes NULL)
            if not counts["n"] and k not in (over or {}):
                ptr[k] = None
        arg = L.PhantRcptSegsIn(C.sizeof(L.PhantRcptSegsIn), self.form if form is None else form, counts["n_blocks"], counts["n"], log_cap, topic_cap,
                                (C.c_uint32 * 2)(*reserved), ptr["receipts"], ptr["rc_off"], counts["rc_bytes"], *[ptr[k] for k in L.RSEG_INPUTS[2:]])
        count = {"n": n, "n_blocks": nb, "n_logs": log_cap, "n_topics": topic_cap, "encoded_len": encoded_cap}
        rows = {name: count[r] + extra for name, _, _, r, extra in L.RSEG_OUTPUTS if name in want}
        size = {k: WIDTH[k] * rows[k] for k in rows}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in rows}
        out_ptr = lambda k: self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        out = L.PhantRcptSegsOut(C.sizeof(L.PhantRcptSegsOut), 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, encoded_cap, 0xEEEEEEEEEEEEEEEE,
                                 *[out_ptr(name) for name, _, _, _, _ in L.RSEG_OUTPUTS])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_receipt_segments_dev if self.dev else ctx._lib.phant_block_receipt_segments
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
        return rc, got, (int(out.first_bad_block), int(out.n_logs), int(out.n_topics), int(out.encoded_len))


def check(P, blocks, form, forms=(False, True), ctx=None, want=None, **kw):
    """every answer of the call against the definition, in both forms, with buffers of exactly the rows the definition has -> its arrays"""
    exp, *scalars = G.expected(blocks, form, kw.get("exp_root"), kw.get("exp_bloom"), kw.get("exp_gas"), kw.get("exp_count"))
    ctx = ctx or _ctx(P)
    for dev in forms:
        rc, got, sc = RawSegs(P, blocks, form, dev=dev).call(ctx, want=want, log_cap=scalars[1], topic_cap=scalars[2], encoded_cap=scalars[3], **kw)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert sc == tuple(scalars), (dev, sc, scalars)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    return {k: np.frombuffer(exp[k], "<u%d" % WIDTH[k]) for k in G.OUTPUTS if WIDTH[k] in (4, 8)} | {"raw": exp, "scalars": tuple(scalars)}


def _log(k, topics=1, data=b""):
    return (bytes([0x10 + k % 200]) * 20, [bytes([k % 251, t]) * 16 for t in range(topics)], bytes(data))


def _plain(i, gas=None, logs=(), tx_type=None, ok=True):
    """receipt i of a block: rising gas, a type that changes"""
    return ((0, 1, 2, 3, 4, 0x7F)[i % 6] if tx_type is None else tx_type, ok, 21000 * (i + 1) if gas is None else gas, list(logs))


def _enc(blocks, form):
    return [[G.encode(r, form) for r in b] for b in blocks]


# ------------------------------------------------------------------------------------------------------------- one block
@pytest.mark.parametrize("form", FORMS)
def test_one_block_equals_block_receipts_from_fields(P, form):
    """n_blocks == 1: root, blooms, the block's bloom and the encodings of phant_block_receipts over the same receipts from their fields"""
    T = P.types.receipt
    receipts = [_plain(i, logs=[_log(i + k, topics=(i + k) % 5, data=_data(3 * k + i, i)) for k in range(i % 4)]) for i in range(suite.scale(9, 5))]
    fields = T.block_receipts([T.Receipt.init(ok, gas, [T.Log(a, ts, d) for a, ts, d in logs], t) for t, ok, gas, logs in receipts])
    r = check(P, _enc([receipts], form), form)
    raw = r["raw"]
    assert raw["receipts_root"] == fields.receipts_root and raw["logs_bloom"] == fields.logs_bloom and raw["bloom"] == fields.blooms.tobytes()
    assert raw["encoded"] == b"".join(fields.encoded) and not r["flags"].any() and not r["block_flags"].any()


# ------------------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("form", FORMS)
def test_block_boundaries_on_wave_edges_and_empty_blocks(P, form):
    """blocks of 0, 1, 63, 64, 65, 127, 128, 129 and 257 receipts: boundaries on wave edges and on the key order's turn at 0x80, empty blocks
    first, last and adjacent"""
    counts = suite.scale((0, 0, 1, 63, 64, 0, 0, 65, 127, 128, 129, 257, 0), (0, 0, 1, 63, 0, 0, 65, 129, 0))
    blocks = [[_plain(i, logs=[_log(i + b)] if i % 7 == 3 else ()) for i in range(c)] for b, c in enumerate(counts)]
    r = check(P, _enc(blocks, form), form, exp_count=list(counts), exp_gas=[21000 * c for c in counts])
    assert not r["block_flags"].any() and r["block_first_bad"].tolist() == list(counts) and r["scalars"][0] == len(counts)
    assert r["raw"]["receipts_root"][:32] == r["raw"]["receipts_root"][-32:] == bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")


@pytest.mark.parametrize("form", FORMS)
def test_many_small_blocks(P, form):
    """300 blocks of 0 - 2 receipts: the bisection over block_first, more tries than a workgroup has lanes"""
    counts = [(5 * b + b // 7) % 3 for b in range(300)]
    blocks = [[_plain(k, gas=(5 if b % 5 == 4 and k == 1 else None), logs=[_log(b)] * (b % 2)) for k in range(c)] for b, c in enumerate(counts)]
    r = check(P, _enc(blocks, form), form, exp_count=counts)
    assert r["block_flags"].sum() == sum(1 for b, c in enumerate(counts) if b % 5 == 4 and c == 2) > 0


# ------------------------------------------------------------------------------------------------------------------ logs
@pytest.mark.parametrize("form", FORMS)
def test_logs_topics_and_data_lengths(P, form):
    """receipts without logs between receipts with logs; one receipt of 200 logs (a lane's walk longer than a wave is wide); 0, 1, 4 and 7
    topics; data of 0, 1 (below 0x80 and not), 55, 56, 255, 256 and 65536 bytes"""
    datas = [b"", b"\x7f", b"\x80", _data(55), _data(56), _data(255), _data(256), _data(65536)]
    shapes = [_log(k, topics=(0, 1, 4, 7)[k % 4], data=d) for k, d in enumerate(datas)]
    many = [_log(k, topics=k % 3, data=_data(k % 9, k)) for k in range(suite.scale(200, 70))]
    blocks = [[_plain(0), _plain(1, logs=shapes[:3]), _plain(2), _plain(3), _plain(4, logs=shapes[3:])], [_plain(0, logs=many), _plain(1)], [_plain(0, logs=shapes[::-1])]]
    r = check(P, _enc(blocks, form), form)
    assert not r["flags"].any() and r["scalars"][1] == 16 + len(many) and r["data_len"].tolist()[:8] == [len(d) for d in datas]
    assert r["log_first"].tolist() == [0, 0, 3, 3, 3, 8, 8 + len(many), 8 + len(many), 16 + len(many)]


def _payload_len(raw):
    raw = raw[1:] if raw[0] < 0x80 else raw
    return len(raw) - (1 if raw[0] < 0xF8 else 1 + raw[0] - 0xF7)


def _with_payload(target, form, built):
    """a receipt with one log whose data is as long as it takes for the list payload -- of its encoding in `form`, or (built) of the consensus
    encoding made from it -- to be `target` bytes, or None where no data length gives that"""
    log = lambda d: (b"\x33" * 20, [], bytes(d))  # noqa: E731
    bloom = R.bloom_of([log(0)])
    enc = lambda d: G.encode_consensus((1, True, 7, [log(d)]), bloom) if built or form == G.CONSENSUS else G.encode_eth69((1, True, 7, [log(d)]))  # noqa: E731
    base = _payload_len(enc(1))
    for d in range(max(target - base - 8, 0), max(target - base + 3, 1)):
        if _payload_len(enc(d)) == target:
            return (1, True, 7, [log(d)])
    return None


@pytest.mark.parametrize("form", FORMS)
def test_receipt_lengths_on_each_side_of_the_header_turns(P, form):
    """list payloads of 55 / 56, 255 / 256 and 65535 / 65536 bytes in the input AND in the built consensus encoding: the two turn at
    different data lengths, the bloom adds 259 bytes.  (A consensus receipt is longer than 256 bytes whatever its logs.)"""
    found = {(t, built): _with_payload(t, form, built) for t in (55, 56, 255, 256, 65535, 65536) for built in (False, True)}
    feasible = [k for k, v in found.items() if v is not None]
    assert {(65535, False), (65536, False), (65535, True), (65536, True)} <= set(feasible)
    assert form == G.CONSENSUS or {(55, False), (56, False), (255, False), (256, False)} <= set(feasible)
    receipts = [found[k] for k in feasible]
    blocks = [[(t, ok, 7 + i, logs) for i, (t, ok, _, logs) in enumerate(receipts)]]
    r = check(P, _enc(blocks, form), form)
    assert not r["flags"].any()
    lens = np.diff(r["encoded_off"]).tolist()
    assert len(set(lens)) >= 2 and min(lens) < 65536 + 259 < max(lens) + 300


# ---------------------------------------------------------------------------------------------------------------- fields
@pytest.mark.parametrize("form", FORMS)
def test_gas_types_and_a_post_state_root(P, form):
    blocks = [[_plain(0, gas=1, tx_type=0), _plain(1, gas=2**32, tx_type=1), _plain(2, gas=2**64 - 1, tx_type=2)],
              [_plain(0, tx_type=3, ok=False), (4, b"\xab" * 32, 50000, [_log(1)]), _plain(2, tx_type=0x7F)]]
    r = check(P, _enc(blocks, form), form)
    assert r["flags"].tolist() == [0, 0, 0, 0, G.POST_STATE, 0] and r["raw"]["tx_type"] == bytes([0, 1, 2, 3, 4, 0x7F]) and r["raw"]["status"] == bytes([1, 1, 1, 0, 2, 1])
    assert r["cum_gas"].tolist() == [1, 2**32, 2**64 - 1, 21000, 50000, 63000] and r["gas_used"].tolist() == [1, 2**32 - 1, 2**64 - 1 - 2**32, 21000, 29000, 13000]
    assert r["block_gas_used"].tolist() == [2**64 - 1, 63000] and not r["block_flags"].any()


# ----------------------------------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize("form", FORMS)
def test_each_flag_alone(P, form):
    """one flipped bit in an embedded bloom; equal cum_gas twice; a gas that goes down; a first row without gas; a wrong expected root, bloom,
    gas or count in exactly one block; the same bytes passing in one block and failing in its neighbour"""
    e = lambda r: G.encode(r, form)  # noqa: E731
    a, b2, c = _plain(0, gas=100, logs=[_log(1)]), _plain(1, gas=200), _plain(2, gas=150)
    flipped = bytearray(G.encode_consensus(a))
    flipped[40] ^= 0x10  # (inside the bloom: type byte, list header, status, gas, 0xb9 0x01 0x00 are in front of it)
    blocks = [[e(a), e(b2)], [bytes(flipped) if form == G.CONSENSUS else e(a)], [e(a), e(a)], [e(b2), e(c)], [e(_plain(0, gas=0))],
              [e(c)], [e(b2), e(c)], [e(a)], [e(a)], [e(a)], [e(a)]]
    good, *_ = G.expected(blocks, form)
    rows = lambda k, w: [good[k][w * i:w * i + w] for i in range(len(blocks))]  # noqa: E731
    roots, blooms, gas, counts = rows("receipts_root", 32), rows("logs_bloom", 256), np.frombuffer(good["block_gas_used"], "<u8").tolist(), [len(x) for x in blocks]
    roots[7], blooms[8], gas[9], counts[10] = roots[0], bytes(255) + b"\x01", gas[9] + 1, 2
    r = check(P, blocks, form, exp_root=roots, exp_bloom=blooms, exp_gas=gas, exp_count=counts)
    bloom_flag = G.BLOOM if form == G.CONSENSUS else 0
    assert r["flags"].tolist() == [0, 0, bloom_flag, 0, G.GAS_ORDER, 0, G.GAS_ORDER, G.GAS_ORDER, 0, 0, G.GAS_ORDER, 0, 0, 0, 0]
    assert r["block_flags"].tolist() == [0, G.RB_RECEIPT if bloom_flag else 0, G.RB_RECEIPT, G.RB_RECEIPT, G.RB_RECEIPT, 0, G.RB_RECEIPT, G.RB_ROOT, G.RB_BLOOM, G.RB_GAS_USED,
                                         G.RB_COUNT]
    assert r["block_first_bad"].tolist() == [2, 0 if bloom_flag else 1, 1, 1, 0, 1, 1, 1, 1, 1, 1] and r["scalars"][0] == (1 if bloom_flag else 2)
    # the least bad block, not the first in flag order; and no expectation, no flag
    rc, _, sc = RawSegs(P, blocks[5:], form).call(_ctx(P), exp_count=[1, 2, 1, 1, 1, 2], want=("block_flags",))
    assert rc == OK and sc[0] == 1
    rc, got, sc = RawSegs(P, blocks[7:], form).call(_ctx(P), want=("block_flags",))
    assert rc == OK and sc[0] == 4 and got["block_flags"] == bytes(16)


# ------------------------------------------------------------------------------------------------------------- malformed
def _variants(x):
    out = [x[:k] for k in range(len(x))] + [x + b"\x00"]
    for k in range(len(x)):
        out += [x[:k] + bytes([b]) + x[k + 1:] for b in VALUES if b != x[k]]
        out += [x[:k] + bytes([head]) + b"\xff" * 8 + x[k:] for head in (0xBF, 0xFF)]  # a length of 2^64 - 1 from here on
    return out


@pytest.mark.parametrize("form", FORMS)
def test_malformed_rows_all_in_one_call(P, form):
    """the truncations, single-byte replacements and 2^64 - 1 lengths of a legacy receipt, a typed one with two logs and one without logs, ALL
    as rows of a few blocks of one call, good rows between them: every flag, field, bloom, log row and root is the definition's.  The
    input ends flush with its allocation and every output sits between guards, so a lane that reads past a row's end reads its neighbour's
    bytes (a wrong answer) or leaves the buffer (the emulated run's sanitizer)."""
    seeds = [(0, True, 21000, [_log(1, topics=1, data=b"\x01")]), (2, True, 30000, [_log(2, topics=2, data=_data(60)), _log(3, topics=0)]), (1, False, 5, [])]
    rows = []
    for s in seeds:
        raw = G.encode(s, form)
        rows += [raw] + _variants(raw)
    stride = suite.scale(1, 23)
    rows = rows[::stride]
    cut = [0, 1, len(rows) // 3, len(rows) // 3, 2 * len(rows) // 3, len(rows)]
    blocks = [rows[cut[i]:cut[i + 1]] for i in range(5)]
    r = check(P, blocks, form)
    bad = (r["flags"] & G.UNDECODABLE) != 0
    # (a twelfth of the rows are truncations, none of which decodes; damage inside an address, a topic, data or an embedded bloom still does)
    assert bad.sum() > len(rows) // 12 and (~bad).sum() > suite.scale(100, 5) and r["block_flags"].tolist() == [0, 1, 0, 1, 1]


# --------------------------------------------------------------------------------------------------- outputs and buffers
@pytest.mark.parametrize("form", FORMS)
def test_subsets_of_the_outputs_unaligned_byte_arrays_and_short_caps(P, form):
    """each output alone, none of the per-log arrays, seeded subsets: the span the host form fetches ends at every position; the byte arrays
    of inputs and outputs at odd addresses; log_cap, topic_cap and encoded_cap one short"""
    blocks = _enc([[_plain(0, logs=[_log(0, 2, b"abc")]), _plain(1)], [], [_plain(0, logs=[_log(1, 0), _log(2, 3, _data(70))])]], form)
    exp, *scalars = G.expected(blocks, form, exp_gas=[42000, 0, 21000])
    _, nl, nt, el = scalars
    rng = np.random.default_rng(17)
    subsets = [(), G.PER_RECEIPT + G.ENCODINGS + G.PER_BLOCK] + [(k,) for k in G.OUTPUTS] + [tuple(k for k in G.OUTPUTS if rng.integers(0, 2)) for _ in range(suite.scale(12, 3))]
    ctx = _ctx(P)
    for dev in (False, True):
        raw = RawSegs(P, blocks, form, dev=dev)
        for want in subsets:
            rc, got, sc = raw.call(ctx, want=want, log_cap=nl, topic_cap=nt, encoded_cap=el, exp_gas=[42000, 0, 21000])
            assert rc == OK and sc == tuple(scalars), (dev, want, sc)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
        odd = {k: 1 for k in G.OUTPUTS if WIDTH[k] not in (4, 8)}
        rc, got, sc = raw.call(ctx, log_cap=nl, topic_cap=nt, encoded_cap=el, skew=odd, in_skew=1 if dev else 3, exp_root=[bytes(32)] * 3, exp_bloom=[bytes(256)] * 3)
        assert rc == OK and sc[1:] == tuple(scalars[1:]) and sc[0] == 0
        assert all(got[k, "guards"] and got[k] == exp[k] for k in G.OUTPUTS if k != "block_flags")
        assert np.frombuffer(got["block_flags"], "<u4").tolist() == [G.RB_ROOT | G.RB_BLOOM, G.RB_ROOT, G.RB_ROOT | G.RB_BLOOM]
        # a cap one short: the scalars say what is needed, the arrays of that kind are untouched, everything else is written
        for caps, untouched in (((nl - 1, nt, el), G.PER_LOG), ((nl, nt - 1, el), G.PER_LOG), ((nl, nt, el - 1), G.ENCODINGS)):
            rc, got, sc = raw.call(ctx, log_cap=caps[0], topic_cap=caps[1], encoded_cap=caps[2])
            assert rc == OK and sc == tuple(scalars), (dev, caps)
            for k in G.OUTPUTS:
                assert got[k, "guards"], (dev, caps, k)
                if k in untouched:
                    assert set(got[k]) <= {0xEE}, (dev, caps, k)
                else:
                    assert got[k] == exp[k], (dev, caps, k)


@pytest.mark.parametrize("form", FORMS)
def test_a_call_beyond_the_pinned_stage_between_small_ones(P, form):
    """small, large (more bytes than the 8 MiB stage holds: the same answers by plain copies), small again on one context"""
    ctx = _ctx(P)
    small = _enc([[_plain(0, logs=[_log(0)])], [_plain(0), _plain(1)]], form)
    large = _enc([[_plain(i, logs=[_log(i, 1, _data(65536 + i % 2, i))]) for i in range(suite.scale(140, 3))], [_plain(0)]], form)
    first = check(P, small, form, ctx=ctx)
    assert large and check(P, large, form, ctx=ctx)["scalars"][3] > suite.scale(8 << 20, 1 << 17)
    assert check(P, small, form, ctx=ctx)["raw"] == first["raw"]


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("form", FORMS)
def test_refused_arguments(P, form):
    """each returns PHANT_E_INVALID_ARG (PHANT_E_UNSUPPORTED for a receipt of 4 GiB) and touches nothing; in the device form the offsets are
    caught by the checking kernel"""
    ctx = _ctx(P)
    blocks = _enc([[_plain(0, logs=[_log(0)]), _plain(1)], [], [_plain(0), _plain(1), _plain(2)]], form)
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantRcptSegsIn), C.sizeof(L.PhantRcptSegsOut))

    def refused(raw, code=E_INVALID_ARG, **kw):
        rc, got, sc = raw.call(ctx, log_cap=4, topic_cap=4, encoded_cap=4096, **kw)
        assert rc == code, (rc, kw)
        assert sc == SCALARS_UNTOUCHED, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawSegs(P, blocks, form, dev=dev)
        a = raw.host
        for k in range(2):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        refused(raw, form=2)
        refused(raw, reserved=(1, 0))
        refused(raw, reserved=(0, 1))
        for k in ("receipts", "rc_off", "block_first"):
            refused(raw, over={k: None})
        refused(raw, over={"n_blocks": 0})
        for k in ("rc_off", "block_first"):
            for at, by in ((0, 1), (1, 100), (-1, 1), (-1, -1)):
                lie = a[k].copy()
                lie[at] = (int(lie[at - 1]) - 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
                if k == "rc_off" and at == -1 and not dev:
                    continue  # (the host form has no other total than the last offset: its last receipt is as long as that says)
                refused(raw, over={k: lie})
        if dev:
            refused(raw, over={"rc_bytes": raw.rc_bytes + 1})
            refused(raw, over={"rc_bytes": raw.rc_bytes - 1})
        refused(raw, over={"n": raw.n - 1})
        huge = a["rc_off"].copy()
        huge[-1] += 1 << 32
        if not dev:
            refused(raw, code=E_UNSUPPORTED, over={"rc_off": huge})
    dev = RawSegs(P, blocks, form, dev=True)
    for k, by in (("cum_gas", 4), ("gas_used", 2), ("log_first", 2), ("flags", 1), ("log_receipt", 3), ("topic_first", 2), ("data_at", 4), ("data_len", 1), ("encoded_off", 4),
                  ("block_gas_used", 4), ("block_first_bad", 2), ("block_flags", 1)):
        refused(dev, skew={k: by})
    for form_dev in (False, True):  # no block: nothing is written but the scalars
        rc, got, sc = RawSegs(P, [], form, dev=form_dev).call(ctx, want=("flags", "log_first", "block_flags", "receipts_root"))
        assert rc == OK and sc == (0, 0, 0, 0) and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str))


# -------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("eth69", (False, True))
def test_validate_receipts_on_the_fixture_segment(P, eth69):
    """the reference's 87 fixture blocks as one segment: the receipts of every block against its decoded header -- no flag; one receipt byte
    changed: that block and the reason; a truncated block: its split status"""
    from tests import headers_ref as H
    form = G.ETH69 if eth69 else G.CONSENSUS
    blocks, roots = G.fixture_receipts()
    raws = [c[3] for chain in H.load_vectors() for c in chain[1:]]
    if suite.EMULATED and not suite.FULL:
        pick = [i for i, b in enumerate(blocks) if len(b) == 2][:2] + list(range(0, 87, 9))
        blocks, roots, raws = [blocks[i] for i in pick], [roots[i] for i in pick], [raws[i] for i in pick]
    x = P.types.block
    ha, hstatus = x.decode_arrays(raws, from_blocks=True)
    assert not hstatus.any() and ha["receipts_root"][:len(raws)].tobytes() == b"".join(roots)
    items = [G.message_item([G.encode(r, form) for r in b], eth69) for b in blocks]
    counts = [len(b) for b in blocks]
    v = x.validate_receipts(ha, items, eth69=eth69, tx_counts=counts)
    assert v.first_bad == len(blocks) and v.reason == [] and not v.block_flags.any() and v.receipts.n == sum(counts)
    assert v.receipts.receipts_root.tobytes() == b"".join(roots)
    assert x.validate_receipts(x.unpack_headers(ha)[:len(raws)], items, eth69=eth69).first_bad == len(blocks)
    # the gas of one receipt changed: its block's root and gas used
    at = next(i for i, b in enumerate(blocks) if len(b) == 2)
    t, ok, gas, logs = blocks[at][1]
    wrong = list(items)
    wrong[at] = G.message_item([G.encode(blocks[at][0], form), G.encode((t, ok, gas + 1, logs), form)], eth69)
    v = x.validate_receipts(ha, wrong, eth69=eth69, tx_counts=counts)
    assert v.first_bad == at and v.reason == ["ReceiptsRoot", "GasUsed"] and int(np.count_nonzero(v.block_flags)) == 1
    # the status of one receipt changed: the root alone
    one = next(i for i, b in enumerate(blocks) if len(b) == 1)
    t, ok, gas, logs = blocks[one][0]
    wrong = list(items)
    wrong[one] = G.message_item([G.encode((t, not ok, gas, logs), form)], eth69)
    v = x.validate_receipts(ha, wrong, eth69=eth69)
    assert v.first_bad == one and v.reason == ["ReceiptsRoot"]
    # a byte of the receipt itself: undecodable
    broken = bytearray(items[one])
    broken[-1] = 0xC1
    wrong[one] = bytes(broken)
    v = x.validate_receipts(ha, wrong, eth69=eth69)
    assert v.first_bad == one and v.reason[0] == "Receipt" and v.receipts.flags[sum(counts[:one])] == G.UNDECODABLE
    # a block cut short: no rows, its split status, and the count says so
    wrong[one] = items[one][:-1]
    v = x.validate_receipts(ha, wrong, eth69=eth69, tx_counts=counts)
    assert v.first_bad == one and v.reason == ["BadRlp"] and v.receipts.n == sum(counts) - 1 and v.receipts.errors(one) == ["ReceiptsRoot", "GasUsed", "Count"]
