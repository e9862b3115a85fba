"""Block headers on the device (phant_header_chain, phant_header_chain_dev, phant_headers_decode_rlp, phant_amd.types.block)
against tests/headers_ref.py, which defines the answer for any chain, and against the 171 fixture headers and the mainnet genesis
header.  Every comparison is exact.  tests/test_emu_headers.py runs the same bodies over the kernel sources compiled for the host, at
the sizes tests/suite.py gives it."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import golden, suite
from tests import headers_ref as H

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def _objs(P, headers):
    return [P.types.block.BlockHeader(**h) for h in headers]


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------------------ synthetic chains
def _below(rng, bound):
    """an integer in [0, bound), bound up to 2^64"""
    return int(rng.integers(0, min(bound, 1 << 62)))


def anchor(rng, nf=17, **kw):
    h = dict(parent_hash=_bytes(rng, 32), uncle_hash=H.EMPTY_UNCLE_HASH, fee_recipient=_bytes(rng, 20), state_root=_bytes(rng, 32),
             transactions_root=_bytes(rng, 32), receipts_root=_bytes(rng, 32), logs_bloom=_bytes(rng, 256), difficulty=0,
             block_number=int(rng.integers(0, 1 << 40)), gas_limit=int(rng.integers(20_000_000, 40_000_000)), gas_used=0,
             timestamp=int(rng.integers(1, 1 << 33)), extra_data=_bytes(rng, int(rng.integers(0, 33))), prev_randao=_bytes(rng, 32),
             nonce=bytes(8), base_fee_per_gas=int(rng.integers(7, 1 << 40)), withdrawals_root=_bytes(rng, 32),
             blob_gas_used=int(rng.integers(0, 1 << 20)), excess_blob_gas=int(rng.integers(0, 1 << 30)), parent_beacon_root=_bytes(rng, 32),
             request_hash=_bytes(rng, 32))
    h.update(kw)
    if "gas_used" not in kw:
        h["gas_used"] = _below(rng, h["gas_limit"] + 1)
    return {f: (h[f] if i < nf else None) for i, f in enumerate(H.FIELDS)}


def child(rng, p, nf=None, **kw):
    """a header that passes every rule against p (where p's fields allow one)"""
    nf = H.n_fields(p) if nf is None else nf
    md = p["gas_limit"] // 1024
    lo, hi = max(p["gas_limit"] - md + 1, 5000), p["gas_limit"] + md - 1
    c = anchor(rng, nf)
    M64 = (1 << 64) - 1  # (a parent at the top of a field has no valid child: the child stays there and is flagged)
    c.update(parent_hash=H.hash(p), block_number=min(p["block_number"] + 1, M64), timestamp=min(p["timestamp"] + int(rng.integers(1, 13)), M64),
             gas_limit=lo + _below(rng, hi + 1 - lo) if lo <= hi else p["gas_limit"])
    c["gas_limit"] = min(c["gas_limit"], (1 << 64) - 1)
    c.update({k: v for k, v in kw.items() if k == "gas_limit"})
    c["gas_used"] = _below(rng, c["gas_limit"] + 1)
    if nf >= 16 and p.get("base_fee_per_gas") is not None:
        e = H.expected_base_fee(p)
        c["base_fee_per_gas"] = e if e is not None and e < 1 << 256 else 0
    c.update(kw)
    return c


def chain(rng, n, nf=17):
    out = [anchor(rng, nf)]
    while len(out) < n:
        out.append(child(rng, out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_headers_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""
    OUTS = ("hashes", "flags", "enc", "enc_off")

    def __init__(self, P, headers=None, dev=False, seg_first=None, expected=None, arrays=None):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch, self.B = L, dev, torch, P.types.block
        a = self.B.pack_headers(_objs(P, headers)) if arrays is None else arrays
        self.n = len(a["extra_off"]) - 1
        self.n_segs = 0 if seg_first is None else len(seg_first) - 1
        if seg_first is not None:
            a = dict(a, seg_first=np.asarray(seg_first, np.uint32))
        if expected is not None:
            a = dict(a, expected_hash=np.frombuffer(b"".join(expected), np.uint8).copy())
        self.arr = {k: self._up(v) for k, v in a.items()}
        self.null = set()
        self.enc_total = 0

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

    def call(self, ctx, want=OUTS, enc_cap=None, guard=64):
        """-> (rc, {output: bytes}, first_bad, enc_len); every buffer has `guard` bytes of 0xEE behind its capacity"""
        L = self.L
        ptr = [None if k in self.null or k not in self.arr else self._ptr(self.arr[k]) for k in L.HEADER_ARRAYS]
        arg = L.PhantHeadersIn(C.sizeof(L.PhantHeadersIn), self.n, self.n_segs, 0, *ptr)
        enc_cap = self.enc_total if enc_cap is None else enc_cap
        size = dict(hashes=32 * self.n, flags=4 * self.n, enc=enc_cap, enc_off=8 * (self.n + 1))
        bufs = {k: self._buf((size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantHeadersOut(C.sizeof(L.PhantHeadersOut), 0xEEEEEEEE, enc_cap, *[self._ptr(bufs[k]) if k in bufs else None for k in self.OUTS],
                                0xEEEEEEEEEEEEEEEE)
        fn = ctx._lib.phant_header_chain_dev if self.dev else ctx._lib.phant_header_chain
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            h = self._down(b)
            assert (h[(size[k] + 7) // 8 * 8:] == 0xEE).all(), k  # nothing behind the capacity
            got[k] = h[:size[k]].tobytes()
        return rc, got, int(out.first_bad), int(out.enc_len)


def expected_of(headers, seg_first=None, expected=None):
    hashes, flags, first_bad = H.validate_chain(headers, seg_first, expected)
    enc = [H.encode(h) for h in headers]
    off = np.cumsum([0] + [len(e) for e in enc]).astype(np.uint64)
    return dict(hashes=b"".join(hashes), flags=np.asarray(flags, np.uint32).tobytes(), enc=b"".join(enc), enc_off=off.tobytes()), first_bad


def check_call(P, headers, seg_first=None, expected=None, forms=(False, True), want=Raw.OUTS):
    """every answer of the call for this chain against the restatement, in both forms -> the expected flags"""
    exp, first_bad = expected_of(headers, seg_first, expected)
    for dev in forms:
        raw = Raw(P, headers, dev=dev, seg_first=seg_first, expected=expected)
        raw.enc_total = len(exp["enc"])
        rc, got, fb, enc_len = raw.call(_ctx(P), want=want)
        assert rc == OK, (dev, _ctx(P)._lib.phant_last_error(_ctx(P).handle))
        assert (fb, enc_len) == (first_bad, len(exp["enc"])), (dev, fb, first_bad)
        for k in want:
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], 4 if k == "flags" else 32 if k == "hashes" else 8 if k == "enc_off" else 1))
    return np.frombuffer(exp["flags"], np.uint32)


def _first_difference(a, b, width):
    for i in range(0, max(len(a), len(b)), width):
        if a[i:i + width] != b[i:i + width]:
            return i // width, a[i:i + width].hex(), b[i:i + width].hex()
    return None


# -------------------------------------------------------------------------------------------------------- known answers
def test_fixture_headers_as_one_call_of_84_segments(P):
    """171 headers, 84 chains, 87 parent/child pairs: the fixtures' hashes, no flag; then with the hashes expected; then one altered"""
    chains = H.load_vectors()
    headers = [h for c in chains for h, _, _, _ in c]
    want = [hh for c in chains for _, hh, _, _ in c]
    seg_first = np.cumsum([0] + [len(c) for c in chains]).tolist()
    assert len(headers) == 171 and len(seg_first) == 85
    B = P.types.block
    hashes, flags, first_bad = B.validate_chain(_objs(P, headers), seg_first=seg_first)
    assert hashes == want and not flags.any() and first_bad == 171
    hashes, flags, first_bad = B.validate_chain(_objs(P, headers), seg_first=seg_first, expected_hashes=want)
    assert hashes == want and not flags.any() and first_bad == 171
    for k in (0, 100, 170):  # an anchor, a header in the middle, the last one
        bad = list(want)
        bad[k] = bad[k][:31] + bytes([bad[k][31] ^ 1])
        hashes, flags, first_bad = B.validate_chain(_objs(P, headers), seg_first=seg_first, expected_hashes=bad)
        assert hashes == want and first_bad == k and flags[k] == B.Flags.ExpectedHashMismatch and np.count_nonzero(flags) == 1
        assert B.first_error(flags[k]) == "ExpectedHashMismatch"
    # as ONE segment every chain's genesis is checked against the previous chain's last header
    check_call(P, headers, expected=want)
    check_call(P, headers, seg_first=seg_first, expected=want)
    r = B.header_chain(_objs(P, headers), seg_first=seg_first, want_encodings=True)
    assert r.encoded == [raw for c in chains for _, _, raw, _ in c]


def test_mainnet_genesis(P):
    h, want, size = H.mainnet_genesis()
    o = _objs(P, [h])[0]
    assert o.n_fields == 15 and o.hash() == want and len(o.encode()) == size and o.encode() == H.encode(h)
    check_call(P, [h], expected=[want])
    # against itself as a parent: a pre-merge header (two headers without a base fee skip that rule)
    flags = check_call(P, [h, h])
    F = P.types.block.Flags
    assert flags[1] == F.InvalidTimestamp | F.InvalidBlockNumber | F.InvalidDifficulty | F.InvalidNonce | F.InvalidParentHash
    assert P.types.block.first_error(flags[1]) == H.first_error(int(flags[1]))


# ------------------------------------------------------------------------------------------------------ synthetic chains
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 257, 2047, 2048, 2049])
def test_valid_chains(P, n):
    """a parent/child pair across a wave boundary (63 | 64), across a workgroup boundary (255 | 256), the last call one workgroup
    plans (2 047 headers, 2 048 offsets) and the first two that the tiled scan takes"""
    rng = np.random.default_rng(100 + n)
    headers = chain(rng, n)
    flags = check_call(P, headers, expected=[H.hash(h) for h in headers] if n < 100 else None)
    assert not flags.any()


def test_every_subset_of_outputs(P):
    rng = np.random.default_rng(30)
    headers = chain(rng, 65)
    headers[40] = dict(headers[40], timestamp=0)
    subsets = [s for k in range(5) for s in itertools.combinations(Raw.OUTS, k)]
    if suite.EMULATED and not suite.FULL:  # (the emulated run alone thins them; a GPU runs all 16 in both forms)
        subsets = subsets[::3] + [Raw.OUTS]
    for s in subsets:
        check_call(P, headers, want=s)


def test_capacity_one_byte_short(P):
    """enc_len is right, neither enc nor enc_off is touched, the other outputs still arrive"""
    rng = np.random.default_rng(31)
    headers = chain(rng, 5)
    exp, first_bad = expected_of(headers)
    total = len(exp["enc"])
    for dev in (False, True):
        raw = Raw(P, headers, dev=dev)
        rc, got, fb, enc_len = raw.call(_ctx(P), enc_cap=total - 1)
        assert rc == OK and enc_len == total and fb == 5
        assert got["enc"] == b"\xEE" * (total - 1) and got["enc_off"] == b"\xEE" * 48
        assert got["hashes"] == exp["hashes"] and got["flags"] == exp["flags"]
        rc, got, fb, enc_len = raw.call(_ctx(P), want=("enc_off",), enc_cap=0)  # (a buffer nobody wants has no capacity to exceed)
        assert rc == OK and got["enc_off"] == exp["enc_off"] and enc_len == total
        rc, got, fb, enc_len = raw.call(_ctx(P), enc_cap=total)
        assert rc == OK and got == exp


MUTATIONS = [  # single-field changes of one header: (field, new value or a function of (old value, the header's parent))
    ("parent_hash", lambda v, p: v[:5] + bytes([v[5] ^ 0x10]) + v[6:]),
    ("uncle_hash", lambda v, p: bytes(32)),
    ("fee_recipient", lambda v, p: bytes(20)),
    ("state_root", lambda v, p: v[::-1]),
    ("transactions_root", lambda v, p: v[::-1]),
    ("receipts_root", lambda v, p: v[::-1]),
    ("logs_bloom", lambda v, p: bytes(256)),
    ("difficulty", 1),
    ("difficulty", (1 << 64) - 1),
    ("block_number", lambda v, p: v + 1),
    ("block_number", lambda v, p: v - 1),
    ("block_number", 0),
    ("gas_limit", lambda v, p: p["gas_limit"] + p["gas_limit"] // 1024),
    ("gas_limit", lambda v, p: p["gas_limit"] - p["gas_limit"] // 1024),
    ("gas_limit", 4999),
    ("gas_limit", 0),
    ("gas_limit", (1 << 64) - 1),
    ("gas_used", lambda v, p: (1 << 64) - 1),
    ("gas_used", 0),
    ("timestamp", lambda v, p: p["timestamp"]),
    ("timestamp", 0),
    ("extra_data", bytes(33)),
    ("extra_data", b""),
    ("extra_data", b"\x7f"),
    ("prev_randao", lambda v, p: bytes(32)),
    ("nonce", bytes(7) + b"\x01"),
    ("nonce", b"\x80" + bytes(7)),
    ("base_fee_per_gas", lambda v, p: v + 1),
    ("base_fee_per_gas", lambda v, p: v - 1),
    ("base_fee_per_gas", 0),
    ("base_fee_per_gas", (1 << 256) - 1),
    ("withdrawals_root", lambda v, p: bytes(32)),
]


def _mutate(headers, i, field, value):
    out = list(headers)
    out[i] = dict(out[i])
    out[i][field] = value(out[i][field], out[i - 1]) if callable(value) else value
    return out


def test_every_single_field_mutation_of_header_64(P):
    """header 64 is the first of the second wave, its parent is in another wave: its flags AND those of header 65, whose parent hash
    now fails, against the restatement"""
    rng = np.random.default_rng(40)
    headers = chain(rng, 130)
    table = MUTATIONS[::4] if suite.EMULATED and not suite.FULL else MUTATIONS
    seen = 0
    for field, value in table:
        m = _mutate(headers, 64, field, value)
        flags = check_call(P, m, forms=(False,))
        changed = m[64] != headers[64]
        assert bool(flags[65] & H.BIT["InvalidParentHash"]) == changed and np.count_nonzero(flags) <= 2, field
        seen |= int(flags[64])
    if table is MUTATIONS:
        assert seen == 0xfff  # every rule fired at least once
    # two mutations in two different headers: first_bad is the lower one, in both forms
    m = _mutate(_mutate(headers, 100, "difficulty", 5), 64, "timestamp", 0)
    flags = check_call(P, m)
    assert list(np.flatnonzero(flags)) == [64, 65, 100, 101]
    m = _mutate(headers, 129, "nonce", b"\x01" * 8)
    assert list(np.flatnonzero(check_call(P, m))) == [129]


# -------------------------------------------------------------------------------------------------------- boundaries
def _pairs_call(P, pairs):
    """every pair a segment of two: one call"""
    headers = [h for pair in pairs for h in pair]
    return check_call(P, headers, seg_first=list(range(0, len(headers) + 1, 2)))[1::2]


def test_integer_boundaries(P):
    rng = np.random.default_rng(50)
    M64 = (1 << 64) - 1
    pairs, want = [], []

    def pair(p_kw, c_kw, bits=None):
        p = anchor(rng, **p_kw)
        c = child(rng, p, **c_kw)
        pairs.append((p, c))
        want.append(bits)
    # every integer at its encoding boundaries (whatever they flag: the restatement says)
    for v in (0, 0x7f, 0x80, 0xff, 0x100, (1 << 32) - 1, 1 << 32, 1 << 63, M64):
        for f in ("difficulty", "block_number", "gas_limit", "gas_used", "timestamp"):
            pair({}, {f: v})
            pair({f: v} if f != "gas_used" else {f: v, "gas_limit": max(v, 5000)}, {})
        p = anchor(rng, 19, blob_gas_used=v, excess_blob_gas=M64 - v)
        pairs.append((p, child(rng, p, blob_gas_used=M64 - v, excess_blob_gas=v)))
        want.append(0)
    # the gas limit at p +- p / 1024 exactly and one inside
    g, md = 30_000_000, 30_000_000 // 1024
    pair(dict(gas_limit=g), dict(gas_limit=g + md, gas_used=0), H.BIT["GasLimitTooHigh"])
    pair(dict(gas_limit=g), dict(gas_limit=g + md - 1, gas_used=0), 0)
    pair(dict(gas_limit=g), dict(gas_limit=g - md, gas_used=0), H.BIT["GasLimitTooLow"])
    pair(dict(gas_limit=g), dict(gas_limit=g - md + 1, gas_used=0), 0)
    pair(dict(gas_limit=5002, gas_used=2501), dict(gas_limit=4999, gas_used=0), H.BIT["GasLimitLessThanMinimum"])
    pair(dict(gas_limit=5002, gas_used=2501), dict(gas_limit=5000, gas_used=0), 0)
    pair(dict(gas_limit=M64, gas_used=M64 // 2), dict(gas_limit=M64, gas_used=M64), 0)      # p + p / 1024 is beyond 64 bits
    pair(dict(block_number=M64), {}, H.BIT["InvalidBlockNumber"])                          # p.number + 1 = 2^64: no 64-bit number equals it
    pair(dict(block_number=M64), dict(block_number=0), H.BIT["InvalidBlockNumber"])
    # t = p.gas_limit / 2 = 0
    for gl in (0, 1):
        pair(dict(gas_limit=gl, gas_used=0, base_fee_per_gas=9), dict(base_fee_per_gas=9))
        pair(dict(gas_limit=gl, gas_used=1, base_fee_per_gas=9), dict(base_fee_per_gas=9))
        assert H.validate(*pairs[-1]) & H.BIT["InvalidBaseFee"] and not H.validate(*pairs[-2]) & H.BIT["InvalidBaseFee"]
    # a delta that rounds to the floor of one, and the same fee going down (delta 0)
    pair(dict(gas_limit=g, gas_used=g // 2 + 1, base_fee_per_gas=7), dict(base_fee_per_gas=8), 0)
    pair(dict(gas_limit=g, gas_used=g // 2 + 1, base_fee_per_gas=7), dict(base_fee_per_gas=7), H.BIT["InvalidBaseFee"])
    pair(dict(gas_limit=g, gas_used=g // 2 - 1, base_fee_per_gas=7), dict(base_fee_per_gas=7), 0)
    # base fees 0, 1, 7, 2^64, 2^255 with the parent full, empty and at its target; one off in both directions
    for fee in (0, 1, 7, 1 << 64, 1 << 255, (1 << 256) - 1):
        for used in (g, 0, g // 2, g // 2 + 12345):
            p = anchor(rng, gas_limit=g, gas_used=used, base_fee_per_gas=fee)
            e = H.expected_base_fee(p)
            for have in (e, e + 1, e - 1):
                if 0 <= have < 1 << 256:
                    pairs.append((p, child(rng, p, base_fee_per_gas=have)))
                    want.append(0 if have == e else H.BIT["InvalidBaseFee"])
            if e >= 1 << 256:  # beyond the field: whatever the header holds, the bit is set
                for have in (0, (1 << 256) - 1, e & ((1 << 256) - 1)):
                    pairs.append((p, child(rng, p, base_fee_per_gas=have)))
                    want.append(H.BIT["InvalidBaseFee"])
    # a gas delta of 64 bits times a fee of 256 bits: the 320-bit product and quotients beyond the field
    for fee in ((1 << 256) - 1, (1 << 200) + 12345, 1 << 192):
        for gl, used in ((2, M64), (M64, M64), (1 << 63, 3), (2, 2), (1 << 33, (1 << 33) - 1)):
            p = anchor(rng, gas_limit=gl, gas_used=used, base_fee_per_gas=fee)
            e = H.expected_base_fee(p)
            have = e if e is not None and e < 1 << 256 else fee
            pairs.append((p, child(rng, p, base_fee_per_gas=have)))
            want.append(None)
    flags = _pairs_call(P, pairs)
    for k, (f, w) in enumerate(zip(flags, want)):
        if w is not None:
            assert int(f) == w, (k, hex(int(f)), hex(w))


def test_extra_data_lengths(P):
    """0 bytes, one byte below and at 0x80, 32 / 33 (the rule), 55 / 56 (the long string form), 300, and 70 000 (a three-byte list length)"""
    rng = np.random.default_rng(51)
    pairs = []
    for x in (b"", b"\x00", b"\x7f", b"\x80", b"\xff", _bytes(rng, 32), _bytes(rng, 33), _bytes(rng, 55), _bytes(rng, 56), _bytes(rng, 300),
              _bytes(rng, suite.scale(70_000, 66_000))):
        p = anchor(rng, extra_data=x[::-1])
        pairs.append((p, child(rng, p, extra_data=x)))
    assert H.encode(pairs[-1][1])[0] == 0xfa
    flags = _pairs_call(P, pairs)
    assert [int(f) for f in flags] == [0] * 6 + [H.BIT["ExtraDataTooLong"]] * 5


def test_every_field_count(P):
    """each n_fields alone -- the arrays no header of the call encodes are NULL --, and a segment that steps through all six"""
    rng = np.random.default_rng(52)
    NEEDS = {"base_fee": 16, "withdrawals_root": 17, "blob_gas_used": 19, "excess_blob_gas": 19, "parent_beacon_root": 20, "requests_hash": 21}
    for nf in H.FIELD_COUNTS:
        headers = chain(rng, 3, nf)
        exp, first_bad = expected_of(headers)
        for dev in (False, True):
            raw = Raw(P, headers, dev=dev)
            raw.null = {k for k, v in NEEDS.items() if v > nf}
            raw.enc_total = len(exp["enc"])
            rc, got, fb, enc_len = raw.call(_ctx(P))
            assert rc == OK and got == exp and fb == 3, (nf, dev)
    steps = [anchor(rng, 15)]
    for nf in (16, 17, 19, 20, 21, 21, 15):
        steps.append(child(rng, steps[-1], nf))
    flags = check_call(P, steps)
    # exactly one of two headers without a base fee: where the reference would unwrap a null, the bit is set
    assert [bool(f & H.BIT["InvalidBaseFee"]) for f in flags] == [False, True, False, False, False, False, False, True]
    pre_london = [anchor(rng, 15)]
    pre_london.append(child(rng, pre_london[0]))
    assert not check_call(P, pre_london).any()  # two headers without one skip the rule


# ------------------------------------------------------------------------------------------------------------ sizes
def test_device_form_and_one_context_small_large_small(P):
    rng = np.random.default_rng(60)
    small = chain(rng, 3)
    large = chain(rng, suite.scale(2500, 2100))  # (beyond what one workgroup plans: the tiled scan and its neighbours)
    large[1500] = dict(large[1500], timestamp=1)
    exp = {id(c): expected_of(c) for c in (small, large)}
    ctx = _ctx(P)
    for headers in (small, large, small):
        want, first_bad = exp[id(headers)]
        for dev in (True, False):
            raw = Raw(P, headers, dev=dev)
            raw.enc_total = len(want["enc"])
            rc, got, fb, enc_len = raw.call(ctx)
            assert rc == OK and fb == first_bad and enc_len == raw.enc_total, ctx._lib.phant_last_error(ctx.handle)
            assert got == want


def test_a_call_beyond_the_pinned_stage(P):
    """16 384 headers are about 9 MB of fields: the caller's arrays and the answers cross the bus array by array"""
    rng = np.random.default_rng(61)
    n = suite.scale(16384, 3000)
    base = chain(rng, 64)
    headers = (base * ((n + 63) // 64))[:n]  # (64 distinct headers repeated: every 64th pair is a break in the chain)
    if suite.EMULATED and not suite.FULL:
        headers = [dict(h, extra_data=h["extra_data"] + bytes(2800)) for h in headers]  # (the same bytes from fewer headers)
    flags = check_call(P, headers, forms=(False,), want=("hashes", "flags"))
    assert sum(v.nbytes for v in P.types.block.pack_headers(_objs(P, headers)).values()) > 8 << 20
    if not (suite.EMULATED and not suite.FULL):
        assert list(np.flatnonzero(flags)) == list(range(64, n, 64))


# ---------------------------------------------------------------------------------------------------------- refused
def test_refused_arguments(P):
    rng = np.random.default_rng(70)
    headers = chain(rng, 6, 21)
    ctx = _ctx(P)
    L = ctx._lib

    def refused(dev, mutate, seg_first=None):
        raw = Raw(P, headers, dev=dev, seg_first=seg_first, expected=[bytes(32)] * 6)
        if not dev:
            raw.arr = {k: v.copy() for k, v in raw.arr.items()}
        mutate(raw)
        rc, got, fb, enc_len = raw.call(ctx, enc_cap=8192)
        assert rc == E_INVALID_ARG, (dev, rc)
        assert all(v == b"\xEE" * len(v) for v in got.values()) and fb == 0xEEEEEEEE and enc_len == 0xEEEEEEEEEEEEEEEE  # a refused call writes nothing

    def poke(name, index, value):
        return lambda raw: raw.arr[name].__setitem__(index, value)

    for dev in (False, True):
        rc, got, fb, _ = Raw(P, headers, dev=dev, seg_first=[0, 2, 6]).call(ctx, enc_cap=8192)  # the call itself is fine
        assert rc == OK and fb == 6
        for nf in (0, 14, 18, 22):
            refused(dev, poke("n_fields", 3, nf))
        refused(dev, poke("extra_off", 2, 1 << 20))       # goes backwards behind it
        refused(dev, poke("extra_off", 0, 1))             # does not start at 0
        refused(dev, poke("seg_first", 1, 0), [0, 2, 6])  # 0 0 6: does not increase
        refused(dev, poke("seg_first", 1, 7), [0, 2, 6])  # 0 7 6
        refused(dev, poke("seg_first", 2, 5), [0, 2, 6])  # does not end at n
        refused(dev, poke("seg_first", 2, 7), [0, 2, 6])
        refused(dev, poke("seg_first", 0, 1), [0, 2, 6])  # does not start at 0
        refused(dev, lambda raw: setattr(raw, "n_segs", 0), [0, 2, 6])
        refused(dev, lambda raw: setattr(raw, "n_segs", 7), [0, 2, 6])
        for name in L_ARRAYS_NEEDED:  # a NULL array that a header needs
            refused(dev, lambda raw, name=name: raw.null.add(name))
    # the structs themselves
    from phant_amd import _lib as Lb
    arg = Lb.PhantHeadersIn(C.sizeof(Lb.PhantHeadersIn) - 4, 1)
    out = Lb.PhantHeadersOut(C.sizeof(Lb.PhantHeadersOut), 77)
    for fn in (L.phant_header_chain, L.phant_header_chain_dev):
        assert fn(ctx.handle, C.byref(arg), C.byref(out)) == E_INVALID_ARG
        assert fn(ctx.handle, None, C.byref(out)) == E_INVALID_ARG
        assert fn(ctx.handle, C.byref(Lb.PhantHeadersIn(C.sizeof(Lb.PhantHeadersIn))), None) == E_INVALID_ARG
        assert out.first_bad == 77
        assert fn(ctx.handle, C.byref(Lb.PhantHeadersIn(C.sizeof(Lb.PhantHeadersIn))), C.byref(out)) == OK and out.first_bad == 0  # n == 0
        out.first_bad = 77


L_ARRAYS_NEEDED = ("parent_hash", "uncle_hash", "fee_recipient", "state_root", "transactions_root", "receipts_root", "logs_bloom", "difficulty",
                   "number", "gas_limit", "gas_used", "timestamp", "extra_data", "extra_off", "prev_randao", "nonce", "base_fee",
                   "withdrawals_root", "blob_gas_used", "excess_blob_gas", "parent_beacon_root", "requests_hash", "n_fields")


# ---------------------------------------------------------------------------------------------------------- decoder
def test_decoded_fixture_headers_hash_to_the_fixtures_values(P):
    """decode(raw) fed straight into phant_header_chain: the hash of a raw header is the hash of its bytes"""
    B = P.types.block
    everything = [x for c in H.load_vectors() for x in c]
    for from_blocks in (False, True):
        arrays, status = B.decode_arrays([x[3] if from_blocks else x[2] for x in everything], from_blocks=from_blocks)
        assert not status.any()
        assert B.unpack_headers(arrays) == _objs(P, [x[0] for x in everything])
        r = B.header_chain(None, arrays=arrays, want_encodings=True)
        assert r.hashes == [x[1] for x in everything] and r.encoded == [x[2] for x in everything]
    g, want, _ = H.mainnet_genesis()
    assert B.BlockHeader.decode(H.encode(g)) == _objs(P, [g])[0] and B.BlockHeader.decode(H.encode(g)).hash() == want


def test_the_decoder_refuses(P):
    from tests import receipts_ref as R
    B = P.types.block
    rng = np.random.default_rng(80)
    h = anchor(rng, 21, extra_data=b"\x05")
    raw = H.encode(h)
    items = [R.rlp_str(x) for x in R.rlp_decode(raw)]
    relist = lambda its: R.rlp_list(its)  # noqa: E731
    bad = {
        "a non-minimal integer": relist(items[:11] + [b"\x82\x00\x05"] + items[12:]),
        "a nine-byte integer": relist(items[:11] + [R.rlp_str(bytes([1]) + bytes(8))] + items[12:]),
        "a 33-byte base fee": relist(items[:15] + [R.rlp_str(bytes([1]) + bytes(32))] + items[16:]),
        "a 31-byte hash": relist([R.rlp_str(bytes(31))] + items[1:]),
        "a 19-byte address": relist(items[:2] + [R.rlp_str(bytes(19))] + items[3:]),
        "a 255-byte bloom": relist(items[:6] + [R.rlp_str(bytes(255))] + items[7:]),
        "a seven-byte nonce": relist(items[:14] + [R.rlp_str(bytes(7))] + items[15:]),
        "18 items": relist(items[:18]),
        "14 items": relist(items[:14]),
        "22 items": relist(items + [b"\x80"]),
        "trailing bytes": raw + b"\x00",
        "a truncation": raw[:-1],
        "a prefixed single byte": relist(items[:12] + [b"\x81\x05"] + items[13:]),
        "a nested list": relist(items[:12] + [b"\xc0"] + items[13:]),
        "a string": R.rlp_str(raw),
        "nothing": b"",
    }
    arrays, status = B.decode_arrays([raw] + list(bad.values()) + [raw])
    assert list(status) == [0] + [1] * len(bad) + [0], [k for k, s in zip(bad, status[1:]) if not s]
    assert list(arrays["n_fields"]) == [21] + [0] * len(bad) + [21]
    assert B.unpack_headers(arrays)[0] == B.unpack_headers(arrays)[-1] == _objs(P, [h])[0]
    # a refused item cannot be passed on by mistake: the chain call refuses its n_fields
    ctx = _ctx(P)
    raw_call = Raw(P, arrays=arrays)
    rc, got, fb, _ = raw_call.call(ctx, enc_cap=1 << 16)
    assert rc == E_INVALID_ARG
    with pytest.raises(ValueError):
        B.BlockHeader.decode(bad["trailing bytes"])
    # whole blocks: the header must be the first of three or four lists
    block = H.load_vectors()[0][1][3]
    hdr = H.decode_block(block)
    _, st = B.decode_arrays([block, hdr, block[:-1], block + b"\x00"], from_blocks=True)
    assert list(st) == [0, 1, 1, 1]
    _, st = B.decode_arrays([block], from_blocks=False)
    assert list(st) == [1]


# ------------------------------------------------------------------------------------------------------ engine API
def test_payload_block_hash(P):
    """the blockHash check newPayloadV2Handler leaves out, on fixture blocks: the header rebuilt from a payload's fields and the two
    roots computed from its transactions and withdrawals hashes to the fixture's `hash` (rlp(index) keys, as a header commits to)"""
    from oracle import oracle as O
    B = P.types.block
    cases = golden.fixtures()["cases"]
    chains = H.load_vectors()
    picked = 0
    for c, ch in list(zip(cases, chains))[::suite.scale(9, 30)]:
        assert len(c["blocks"]) == len(ch) - 1
        for b, (h, want, _, _) in zip(c["blocks"], ch[1:]):
            txs = [bytes.fromhex(t) for t in b["tx_values"]]
            wds = [bytes.fromhex(w) for w in b["withdrawal_values"]]
            payload = dict(parentHash=h["parent_hash"], feeRecipient=h["fee_recipient"], stateRoot=h["state_root"], receiptsRoot=h["receipts_root"],
                           logsBloom=h["logs_bloom"], prevRandao=h["prev_randao"], blockNumber=h["block_number"], gasLimit=h["gas_limit"],
                           gasUsed=h["gas_used"], timestamp=h["timestamp"], extraData=h["extra_data"], baseFeePerGas=h["base_fee_per_gas"],
                           blockHash=want)
            ok, got, built = B.payload_block_hash(payload, txs, wds, keys="rlp")
            assert ok and got == want and built == _objs(P, [h])[0]
            ok, got, _ = B.payload_block_hash(dict(payload, gasUsed=h["gas_used"] + 1), txs, wds, keys="rlp")
            assert not ok and got != want
            # toBlock's own keys (32-byte big-endian indices): another header, whose hash the restatement gives
            ok, got, built = B.payload_block_hash(payload, txs, wds)
            ref = dict(h, transactions_root=O.index_root_be32(txs), withdrawals_root=O.index_root_be32(wds))
            assert got == H.hash(ref) and ok == (ref == h)
            picked += 1
    assert picked >= 3
