"""Execution requests of chain segments on the device (phant_block_requests, phant_block_requests_dev,
phant_amd.types.receipt.block_requests, phant_amd.types.block.validate_requests) against tests/requests_ref.py, which defines every output
from the rules of include/phant_gpu.h with hashlib.sha256.  Every comparison is exact, in the host and the device form.  The rows of the
logs come out of a real receipt_segments call over receipts in both wire forms, and once they are packed by hand.
tests/test_emu_requests.py runs the same bodies over the kernel sources compiled for the host."""
import ctypes as C

import numpy as np
import pytest

from tests import receipts_seg_ref as G
from tests import requests_ref as Q
from tests.test_gpu_receipt_segments import _enc, _plain
from tests.test_gpu_transactions import OK, E_INVALID_ARG, _ctx, _data, _first_difference

pytestmark = pytest.mark.gpu
FORMS = (G.CONSENSUS, G.ETH69)
WIDTH = Q.WIDTH
CONTRACT = bytes.fromhex("00000000219ab540356cbb839cbe05303d7705fa")
SCALARS_UNTOUCHED = (0xEEEEEEEE, 0xEEEEEEEE)
LOG_ROWS = ("receipts", "block_first", "log_first", "address", "topic_first", "topics", "data_at", "data_len")


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


# ------------------------------------------------------------------------------------------------------------- the logs
def dep(k):
    """the data of deposit k: every field its own bytes"""
    return Q.deposit_event(_data(48, k), _data(32, k + 1), _data(8, k + 2), _data(96, k + 3), int(k).to_bytes(8, "little"))


def dlog(k, data=None, address=CONTRACT, topics=None):
    return (address, [Q.DEPOSIT_TOPIC] if topics is None else topics, dep(k) if data is None else bytes(data))


def other_log(k, data=b"xyz"):
    return (bytes([0x10 + k % 200]) * 20, [bytes([k % 251, t]) * 16 for t in range(k % 3)], bytes(data))


def rows_of(P, blocks, form=G.CONSENSUS):
    """blocks: per block a list of receipts, each the list of its logs -> the rows of the logs as a real phant_block_receipt_segments call
    over the receipts in `form` answers them, and the packed receipts they point into"""
    T = P.types.receipt
    packed = T.pack_receipt_segments(_enc([[_plain(i, logs=logs) for i, logs in enumerate(b)] for b in blocks], form))
    s = T.receipt_segments(packed, form=form, roots=False, logs=True)
    assert s.first_bad_block == len(blocks)
    return {k: getattr(s, k) for k in LOG_ROWS}


def rows_by_hand(blocks):
    """the same rows packed by hand: `receipts` is nothing but the logs' data back to back, a byte between them, so that no data is aligned"""
    blob, a = b"", {k: [] for k in ("address", "topics", "data_at", "data_len")}
    block_first, log_first, topic_first = [0], [0], [0]
    for b in blocks:
        for logs in b:
            for address, topics, data in logs:
                blob += b"\xa5"
                a["address"].append(address), a["topics"].extend(topics), a["data_at"].append(len(blob)), a["data_len"].append(len(data))
                topic_first.append(topic_first[-1] + len(topics))
                blob += data
            log_first.append(len(a["data_at"]))
        block_first.append(len(log_first) - 1)
    return {"receipts": np.frombuffer(blob or b"\x00", np.uint8).copy()[:len(blob)], "block_first": np.asarray(block_first, np.uint32), "log_first": np.asarray(log_first, np.uint32),
            "address": np.frombuffer(b"".join(a["address"]), np.uint8).reshape(-1, 20), "topic_first": np.asarray(topic_first, np.uint32),
            "topics": np.frombuffer(b"".join(a["topics"]), np.uint8).reshape(-1, 32), "data_at": np.asarray(a["data_at"], np.uint64), "data_len": np.asarray(a["data_len"], np.uint32)}


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawReq:
    """phant_requests_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, rows, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.rows = L, dev, torch, rows
        self.nb, self.n, self.nl, self.nt = len(rows["block_first"]) - 1, len(rows["log_first"]) - 1, len(rows["data_at"]), len(rows["topics"])

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

    def call(self, ctx, contract=CONTRACT, other=None, active=None, exp_hash=None, want=None, deposit_cap=None, guard=64, sizes=None, reserved=(0, 0), skew=None, in_skew=0,
             over=None):
        """-> (rc, {output: bytes}, (n_deposits, first_bad_block)); every buffer has `guard` bytes of 0xEE in front of and behind its rows.
        over: {field of phant_requests_in: value} put in last (an array value is uploaded); in_skew: bytes the byte arrays of the inputs are
        moved up by"""
        L, nb = self.L, self.nb
        want = Q.OUTPUTS if want is None else want
        req, n_req = Q.pack_other(other, nb)
        ins = dict(self.rows, **req)
        ins.update(active=None if active is None else np.asarray([1 if x else 0 for x in active] or [0], np.uint8),
                   requests_hash=None if exp_hash is None else np.frombuffer(b"".join(exp_hash) or bytes(32), np.uint8))
        counts = dict(n_blocks=nb, n=self.n, n_logs=self.nl, n_topics=self.nt, n_req=n_req, rc_bytes=len(self.rows["receipts"]), req_total=int(req["req_off"][-1]),
                      deposit_cap=self.nl if deposit_cap is None else deposit_cap)
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k, dt in L.REQUESTS_INPUTS:
            a = None if ins[k] is None else np.ascontiguousarray(ins[k], dt)
            keep[k], ptr[k] = self._up(a, in_skew if dt == "u1" else 0)
        for k in ("req_block_first", "req_type", "req_bytes", "req_off"):  # (never-empty stand-ins: a zero count passes NULL)
            if not counts["n_req"] and k not in (over or {}):
                ptr[k] = None
        arg = L.PhantRequestsIn(C.sizeof(L.PhantRequestsIn), counts["n_blocks"], counts["n"], counts["n_logs"], counts["n_topics"], counts["n_req"], counts["deposit_cap"],
                                reserved[0], ptr["receipts"], counts["rc_bytes"], *[ptr[k] for k, _ in L.REQUESTS_INPUTS[1:12]], counts["req_total"], ptr["active"],
                                ptr["requests_hash"], (C.c_uint8 * 20)(*contract))
        count = {"n_blocks": nb, "n_deposits": counts["deposit_cap"]}
        rows = {name: count[r] + extra for name, _, _, r, extra in L.REQUESTS_OUTPUTS if name in want}
        size = {k: WIDTH[k] * rows[k] for k in rows}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in rows}
        out_ptr = lambda k: (bufs[k].data_ptr() if self.dev else bufs[k].ctypes.data) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        out = L.PhantRequestsOut(C.sizeof(L.PhantRequestsOut), 0xEEEEEEEE, 0xEEEEEEEE, reserved[1], *[out_ptr(name) for name, _, _, _, _ in L.REQUESTS_OUTPUTS])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_requests_dev if self.dev else ctx._lib.phant_block_requests
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
        return rc, got, (int(out.n_deposits), int(out.first_bad_block))


def check(P, rows, forms=(False, True), ctx=None, want=None, rc_bytes=None, **kw):
    """every answer of the call against the definition, in both forms, with buffers of exactly the rows the definition has -> its arrays"""
    exp, nd, first_bad = Q.expected(rows, kw.get("contract", CONTRACT), kw.get("other"), kw.get("active"), kw.get("exp_hash"), rc_bytes=rc_bytes)
    ctx = ctx or _ctx(P)
    if rc_bytes is not None:
        kw["over"] = dict(kw.get("over") or {}, rc_bytes=rc_bytes)
    for dev in forms:
        rc, got, sc = RawReq(rows, dev=dev).call(ctx, want=want, deposit_cap=nd, **kw)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert sc == (nd, first_bad), (dev, sc, nd, first_bad)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    return {k: np.frombuffer(exp[k], "<u4") for k in ("deposit_log", "deposit_first", "block_flags")} | {"raw": exp, "n_deposits": nd, "first_bad": first_bad}


def _hashes(r):
    return [r["raw"]["requests_hash"][32 * b:32 * b + 32] for b in range(len(r["block_flags"]))]


# ------------------------------------------------------------------------------------------------- blocks and deposits
@pytest.mark.parametrize("form", FORMS)
def test_blocks_without_logs_without_deposits_and_with_them(P, form):
    """a block without receipts, one whose receipts have no logs, one with logs but no deposit, one with deposits between other logs: the
    first three commit to nothing -- sha256("")"""
    blocks = [[], [[], []], [[other_log(1)], [other_log(2), other_log(3, dep(9))]], [[other_log(4), dlog(0)], [], [dlog(1), other_log(5), dlog(2)]]]
    r = check(P, rows_of(P, blocks, form))
    assert _hashes(r)[:3] == [Q.EMPTY_HASH] * 3 and r["deposit_first"].tolist() == [0, 0, 0, 0, 3] and r["deposit_log"].tolist() == [4, 5, 7]
    assert not r["block_flags"].any() and r["first_bad"] == 4
    assert _hashes(r)[3] == Q.sha256(Q.sha256(b"\x00" + b"".join(Q.deposit_row(dep(k)) for k in range(3))))


def test_logs_that_are_no_candidates_are_ignored(P):
    """each alone in a block between two deposits: the contract's address with another first topic (the event's as the second), the topic
    under another address, the contract's log without topics, an address that differs in the last byte only -- no row, no flag"""
    near = CONTRACT[:19] + bytes([CONTRACT[19] ^ 1])
    others = [dlog(7, topics=[b"\x11" * 32, Q.DEPOSIT_TOPIC]), dlog(7, address=b"\x22" * 20), dlog(7, topics=[]), dlog(7, address=near),
              dlog(7, topics=[Q.DEPOSIT_TOPIC[:31] + b"\xc4"])]
    blocks = [[[dlog(2 * i), x], [dlog(2 * i + 1)]] for i, x in enumerate(others)]
    r = check(P, rows_of(P, blocks))
    assert not r["block_flags"].any() and r["deposit_first"].tolist() == [0, 2, 4, 6, 8, 10] and r["deposit_log"].tolist() == [0, 2, 3, 5, 6, 8, 9, 11, 12, 14]


def _malformed():
    good = dep(5)
    word = lambda d, at, v: d[:at] + int(v).to_bytes(32, "big") + d[at + 32:]  # noqa: E731
    out = [good[:575], good + b"\x00"]
    out += [word(good, 32 * k, Q.OFFSETS[k] + 1) for k in range(5)] + [word(good, 32 * k, Q.OFFSETS[k] - 1) for k in (0, 4)]
    out += [word(good, Q.OFFSETS[k], Q.SIZES[k] + 1) for k in range(5)] + [word(good, Q.OFFSETS[k], Q.SIZES[k] - 1) for k in (1, 3)]
    out += [b"\x01" + good[1:], good[:Q.OFFSETS[2]] + b"\x80" + good[Q.OFFSETS[2] + 1:], good[:64 + 15] + b"\x01" + good[64 + 16:]]  # (a correct low byte under a set high one)
    return out


@pytest.mark.parametrize("form", FORMS)
def test_malformed_candidates_each_alone_and_all_in_one_call(P, form):
    """data_len 575 and 577, each offset and each size off by one, a correct low byte with a high byte of the word set, and an event whose
    last byte lies one past rc_bytes: each sets PHANT_QBLOCK_DEPOSIT_LAYOUT on its block and yields no row, while the block's other
    deposits still produce theirs"""
    bad = _malformed()
    assert all(not Q.well_formed(d, len(d), 0, len(d)) for d in bad) and Q.well_formed(dep(5), 576, 0, 576)
    for i, d in enumerate(bad):  # each alone
        r = check(P, rows_of(P, [[[dlog(1)]], [[dlog(2), dlog(3, d)], [dlog(4)]]], form))
        assert r["block_flags"].tolist() == [0, Q.LAYOUT] and r["deposit_first"].tolist() == [0, 1, 3] and r["first_bad"] == 1, i
    blocks = [[[dlog(2 * i), dlog(0, d)], [other_log(i), dlog(2 * i + 1)]] for i, d in enumerate(bad)] + [[[dlog(90)]], [[dlog(91), dlog(92)]]]
    rows = rows_of(P, blocks, form)
    r = check(P, rows)
    assert r["block_flags"].tolist() == [Q.LAYOUT] * len(bad) + [0, 0] and r["n_deposits"] == 2 * len(bad) + 3
    # the last event ends with the receipts: one byte fewer of them and it is no longer inside
    assert int(rows["data_at"][-1]) + 576 == len(rows["receipts"])
    r = check(P, rows, rc_bytes=len(rows["receipts"]) - 1)
    assert r["block_flags"].tolist() == [Q.LAYOUT] * len(bad) + [0, Q.LAYOUT] and r["n_deposits"] == 2 * len(bad) + 2
    r = check(P, rows_by_hand([[[dlog(1), dlog(2)]]]), rc_bytes=2 * 577 - 1)
    assert r["block_flags"].tolist() == [Q.LAYOUT] and r["deposit_log"].tolist() == [0]


def test_deposits_on_wave_edges_and_blocks_on_log_edges(P):
    """deposits as the 1st, 64th, 65th and last log of a block of 130 logs; then the same logs in blocks whose boundaries fall on log 63, 64
    and 65; the rows packed by hand give the same answers as the rows a receipt_segments call made"""
    logs = [dlog(k) if k in (0, 63, 64, 129) else other_log(k) for k in range(130)]
    one = [[logs[:40], logs[40:64], logs[64:]]]
    r = check(P, rows_of(P, one))
    assert r["deposit_log"].tolist() == [0, 63, 64, 129] and r["deposit_first"].tolist() == [0, 4]
    split = [[logs[:63]], [logs[63:64]], [logs[64:65]], [logs[65:]]]
    r = check(P, rows_of(P, split, G.ETH69))
    assert r["deposit_first"].tolist() == [0, 1, 2, 3, 4] and len(set(_hashes(r))) == 4
    by_hand = check(P, rows_by_hand(split))
    assert by_hand["raw"]["requests_hash"] == r["raw"]["requests_hash"] and by_hand["raw"]["deposit"] == r["raw"]["deposit"]


@pytest.mark.parametrize("form", FORMS)
def test_many_small_blocks(P, form):
    """300 blocks of 0 or 1 logs, every third log a deposit: the bisections over log_first and block_first, more blocks than a workgroup
    has lanes"""
    blocks = [[[dlog(b) if b % 3 == 0 else other_log(b)]] if (7 * b + b // 5) % 2 else [[]] for b in range(300)]
    r = check(P, rows_of(P, blocks, form), other=[[(1, b"\x01" * (b % 5))] if b % 4 == 0 else [] for b in range(300)])
    assert 30 < r["n_deposits"] < 100 and not r["block_flags"].any() and _hashes(r).count(Q.EMPTY_HASH) > 50


def test_one_block_with_seventy_deposits(P):
    """the type-0 message is 1 + 70 x 192 bytes: 211 compressions in one lane"""
    r = check(P, rows_of(P, [[[dlog(k) for k in range(30)], [dlog(k) for k in range(30, 70)]], [[dlog(99)]]]))
    assert r["deposit_first"].tolist() == [0, 70, 71] and not r["block_flags"].any()


# ---------------------------------------------------------------------------------------------- the caller's requests
def test_callers_requests_order_and_the_active_mask(P):
    """type 1 only; types 1 and 2; an empty row, which is skipped; types 2, 1 and a type 0 row, which set PHANT_QBLOCK_ORDER; a block with
    no requests at all, whose hash is the constant; equal types; then an `active` mask that splits the segment"""
    w, c = _data(76, 1), _data(116, 2)
    other = [[(1, w)], [(1, w), (2, c)], [(1, b""), (2, c)], [(2, c), (1, w)], [(0, w)], [], [(1, w), (1, c)], [(1, w), (2, b""), (255, c)], [(2, c)]]
    blocks = [[[dlog(b)]] if b in (1, 3, 5, 8) else [[other_log(b)]] for b in range(9)]
    blocks[5] = [[other_log(5)]]
    rows = rows_of(P, blocks)
    r = check(P, rows, other=other)
    assert r["block_flags"].tolist() == [0, 0, 0, Q.ORDER, Q.ORDER, 0, Q.ORDER, 0, 0] and r["first_bad"] == 3
    h = _hashes(r)
    assert h[5] == Q.EMPTY_HASH and h[0] == Q.sha256(Q.sha256(b"\x01" + w)) and h[2] == Q.sha256(Q.sha256(b"\x02" + c))
    assert h[1] == Q.sha256(Q.sha256(b"\x00" + Q.deposit_row(dep(1))) + Q.sha256(b"\x01" + w) + Q.sha256(b"\x02" + c))
    active = [False, False, False, False, True, True, False, True, True]
    r = check(P, rows, other=other, active=active, exp_hash=[b"\x77" * 32] * 4 + h[4:])
    assert r["block_flags"].tolist() == [0, 0, 0, 0, Q.ORDER, 0, 0, 0, 0] and r["deposit_first"].tolist() == [0] * 9 + [1]
    assert _hashes(r)[:4] == [bytes(32)] * 4 and _hashes(r)[4:6] == h[4:6] and _hashes(r)[6] == bytes(32)
    r = check(P, rows, other=other, active=[False] * 9)
    assert r["n_deposits"] == 0 and r["first_bad"] == 9 and r["raw"]["requests_hash"] == bytes(32 * 9)


def test_each_flag_alone_and_an_expected_hash_wrong_in_its_last_byte(P):
    blocks = [[[dlog(0)]], [[dlog(1, dep(1)[:575])]], [[dlog(2)]], [[dlog(3)]], [[other_log(4)]]]
    other = [[], [], [(2, b"\x05"), (1, b"\x06")], [(1, b"\x07")], []]
    rows = rows_of(P, blocks)
    good = _hashes(check(P, rows, other=other))
    wrong = list(good)
    wrong[3] = good[3][:31] + bytes([good[3][31] ^ 1])
    r = check(P, rows, other=other, exp_hash=wrong)
    assert r["block_flags"].tolist() == [0, Q.LAYOUT, Q.ORDER, Q.HASH, 0] and r["first_bad"] == 1
    assert check(P, rows, other=other, exp_hash=good)["block_flags"].tolist() == [0, Q.LAYOUT, Q.ORDER, 0, 0]
    # the least bad block, not the first in flag order
    rc, got, sc = RawReq(rows_of(P, blocks[2:])).call(_ctx(P), other=other[2:], exp_hash=[good[3]] * 3, want=("block_flags",))
    assert rc == OK and sc == (2, 0) and np.frombuffer(got["block_flags"], "<u4").tolist() == [Q.ORDER | Q.HASH, 0, Q.HASH]


# --------------------------------------------------------------------------------------------------- outputs and buffers
def test_subsets_of_the_outputs_unaligned_byte_arrays_and_short_caps(P):
    """each output alone, none, all; the byte arrays of inputs and outputs at odd addresses; deposit_cap 0 and one short: the per-deposit
    arrays stay untouched behind their guards, hashes and flags are unchanged"""
    blocks = [[[dlog(0), other_log(1)], [dlog(2, dep(2) + b"\x00")]], [], [[dlog(3), dlog(4)]]]
    other = [[(1, _data(30))], [(2, _data(9))], []]
    rows = rows_of(P, blocks)
    exp, nd, first_bad = Q.expected(rows, CONTRACT, other)
    assert nd == 3 and first_bad == 0
    ctx = _ctx(P)
    for dev in (False, True):
        raw = RawReq(rows, dev=dev)
        for want in [(), Q.OUTPUTS] + [(k,) for k in Q.OUTPUTS] + [("deposit", "block_flags"), ("deposit_log", "requests_hash")]:
            rc, got, sc = raw.call(ctx, other=other, want=want, deposit_cap=nd)
            assert rc == OK and sc == (nd, first_bad), (dev, want, sc)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
        rc, got, sc = raw.call(ctx, other=other, deposit_cap=nd, skew={"deposit": 1, "requests_hash": 3}, in_skew=1 if dev else 3)
        assert rc == OK and sc == (nd, first_bad) and all(got[k, "guards"] and got[k] == exp[k] for k in Q.OUTPUTS), dev
        for cap in (0, nd - 1):
            rc, got, sc = raw.call(ctx, other=other, deposit_cap=cap)
            assert rc == OK and sc == (nd, first_bad), (dev, cap)
            for k in Q.OUTPUTS:
                assert got[k, "guards"], (dev, cap, k)
                assert set(got[k]) <= {0xEE} if k in Q.PER_DEPOSIT else got[k] == exp[k], (dev, cap, k)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments(P):
    """each returns PHANT_E_INVALID_ARG and touches nothing; in the device form the firsts and offsets are caught by the checking kernel"""
    ctx = _ctx(P)
    blocks = [[[dlog(0), other_log(1)], []], [], [[other_log(2)], [dlog(3)], []]]
    other = [[(1, b"ab")], [], [(1, b"c"), (2, b"defg")]]
    rows = rows_of(P, blocks)
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantRequestsIn), C.sizeof(L.PhantRequestsOut))
    req, n_req = Q.pack_other(other, 3)

    def refused(raw, **kw):
        rc, got, sc = raw.call(ctx, other=other, **kw)
        assert rc == E_INVALID_ARG, (rc, kw)
        assert sc == SCALARS_UNTOUCHED, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawReq(rows, dev=dev)
        for k in range(2):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        refused(raw, reserved=(1, 0))
        refused(raw, reserved=(0, 1))
        for k in ("receipts", "block_first", "log_first", "address", "topic_first", "topics", "data_at", "data_len", "req_block_first", "req_type", "req_off"):
            refused(raw, over={k: None})
        if dev:  # (the host form's total is the last offset: it finds the missing bytes by it as well)
            refused(raw, over={"req_bytes": None})
        refused(raw, over={"req_bytes": None, "req_total": 7})
        refused(raw, over={"n_blocks": 0})
        refused(raw, over={"n": raw.n - 1})
        refused(raw, over={"n_logs": raw.nl - 1})
        refused(raw, over={"n_topics": raw.nt + 1})
        refused(raw, over={"n_req": n_req - 1})
        for k, a in (("block_first", rows["block_first"]), ("log_first", rows["log_first"]), ("topic_first", rows["topic_first"]),
                     ("req_block_first", req["req_block_first"]), ("req_off", req["req_off"])):
            for at, by in ((0, 1), (1, 100), (-1, 1), (-1, -1)):
                if k == "req_off" and at == -1 and not dev:
                    continue  # (the host form has no other total than the last offset: its last row is as long as that says)
                lie = np.array(a).copy()
                lie[at] = (int(lie[at + 1]) + 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
                refused(raw, over={k: lie})
        if dev:
            refused(raw, over={"req_total": 8})
            refused(raw, over={"req_total": 6})
    dev = RawReq(rows, dev=True)
    for k, by in (("deposit_log", 2), ("deposit_first", 1), ("block_flags", 3)):
        refused(dev, skew={k: by})
    for form_dev in (False, True):  # no block: nothing is written but the scalars
        rc, got, sc = RawReq(rows_by_hand([]), dev=form_dev).call(ctx)
        assert rc == OK and sc == (0, 0) and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str))


# ------------------------------------------------------------------------------------------------------- the layers above
def test_validate_requests_on_a_prague_segment(P):
    """three Prague blocks built by hand, chained through validate_chain, their receipts through validate_receipts, their requests through
    validate_requests: no flag; a deposit's amount changed in a log: that block's hash; a pre-Prague header: inactive"""
    from tests import headers_ref as H
    from tests.test_gpu_headers import anchor, child
    x = P.types.block
    rng = np.random.default_rng(21)
    logs = [[[other_log(0)], [dlog(1), dlog(2)]], [[other_log(3)]], [[dlog(4)], []]]
    other = [[(1, _data(76, 3))], [], [(1, _data(76, 4)), (2, _data(116, 5))]]
    receipts = [[_plain(i, logs=ls) for i, ls in enumerate(b)] for b in logs]
    enc = _enc(receipts, G.CONSENSUS)
    seg, *_ = G.expected(enc, G.CONSENSUS)
    want = []
    for i, b in enumerate(logs):  # (every log of the contract here is a well-formed deposit)
        mine = [Q.deposit_row(d) for receipt in b for a, _, d in receipt if a == CONTRACT]
        want.append(Q.requests_hash(([(0, b"".join(mine))] if mine else []) + other[i]))
    headers = [anchor(rng, 21)]
    for b in range(3):
        headers.append(child(rng, headers[-1], receipts_root=seg["receipts_root"][32 * b:32 * b + 32], logs_bloom=seg["logs_bloom"][256 * b:256 * b + 256],
                             gas_used=21000 * len(receipts[b]), request_hash=want[b]))
    objs = [x.BlockHeader(**h) for h in headers]
    _, flags, first_bad = x.validate_chain(objs)
    assert first_bad == 4 and not np.asarray(flags).any()
    items = [G.message_item(e) for e in enc]
    v = x.validate_receipts(objs[1:], items, tx_counts=[len(b) for b in receipts], logs=True)
    assert v.first_bad == 3 and v.reason == []
    q = x.validate_requests(objs[1:], v.receipts, CONTRACT, other)
    assert q.first_bad == 3 and q.reason == [] and not q.block_flags.any() and q.requests.n_deposits == 3
    assert q.requests.requests_hash.tobytes() == b"".join(want) and q.requests.requests(0) == Q.deposit_row(dep(1)) + Q.deposit_row(dep(2))
    assert x.validate_requests(x.pack_headers(objs[1:]), v.receipts, CONTRACT, other).first_bad == 3
    # without the system calls' requests block 0 commits to something else
    q = x.validate_requests(objs[1:], v.receipts, CONTRACT, [[], [], other[2]])
    assert q.first_bad == 0 and q.reason == ["RequestsHash"] and q.block_flags.tolist() == [Q.HASH, 0, 0]
    # another contract: no deposits anywhere
    q = x.validate_requests(objs[1:], v.receipts, b"\x01" * 20, other)
    assert q.block_flags.tolist() == [Q.HASH, 0, Q.HASH] and q.requests.n_deposits == 0
    # a header from before the fork: its block is not looked at
    old = x.BlockHeader(**{**headers[2], "request_hash": None})
    q = x.validate_requests([objs[1], old, objs[3]], v.receipts, CONTRACT, other)
    assert q.first_bad == 3 and q.requests.requests_hash[1].tobytes() == bytes(32)
