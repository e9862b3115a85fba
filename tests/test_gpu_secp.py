"""Sender recovery on the device (phant_ecrecover_batch, phant_tx_senders, phant_diag_secp_op) against tests/secp_ref.py, which
defines the answer for ANY tuple (z, r, s, recid) and any byte string offered as a transaction.  Every comparison is exact.
tests/test_emu_secp.py runs the same bodies over the kernel sources compiled for the host, at the sizes tests/suite.py gives it."""
import ctypes as C

import numpy as np
import pytest

from tests import secp_ref as S
from tests import suite

pytestmark = pytest.mark.gpu
M256 = (1 << 256) - 1


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def be(v):
    return int(v).to_bytes(32, "big")


def rows(vals):
    return np.frombuffer(b"".join(be(v) for v in vals), np.uint8).reshape(-1, 32).copy()


def ints(a):
    return [int.from_bytes(bytes(r), "big") for r in a]


# 0, 1, 2, p - 1, p - 2, n - 1, 2^255, 2^256 - 1 (every limb all-ones), each single limb all-ones, values in [p, 2^256)
EDGES = ([0, 1, 2, S.P - 1, S.P - 2, S.N - 1, 1 << 255, M256] + [0xFFFFFFFF << (32 * i) for i in range(8)] +
         [S.P, S.P + 1, S.P + 977, M256 - 1, S.N, S.N + 1])


def _rand_ints(rng, n):
    return [int.from_bytes(rng.bytes(32), "big") for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------ primitives
def test_field_and_scalar_primitives(P):
    rng = np.random.default_rng(1)
    n_rand = suite.scale(2000, 60)
    a = [x for x in EDGES for _ in EDGES] + _rand_ints(rng, n_rand)
    b = [y for _ in EDGES for y in EDGES] + _rand_ints(rng, n_rand)
    A, B = rows(a), rows(b)
    sig = P.signer
    assert ints(sig.secp_op("fe_mul", A, B)) == [x * y % S.P for x, y in zip(a, b)]
    assert ints(sig.secp_op("sc_mul", A, B)) == [x * y % S.N for x, y in zip(a, b)]
    one = EDGES + _rand_ints(rng, suite.scale(2000, 20))
    O = rows(one)
    assert ints(sig.secp_op("fe_sqr", O)) == [x * x % S.P for x in one]
    assert ints(sig.secp_op("fe_inv", O)) == [pow(x, S.P - 2, S.P) for x in one]
    assert ints(sig.secp_op("sc_inv", O)) == [pow(x, S.N - 2, S.N) for x in one]
    inv = ints(sig.secp_op("fe_inv", O))
    assert all(x % S.P == 0 or x * i % S.P == 1 for x, i in zip(one, inv))


def test_square_roots(P):
    rng = np.random.default_rng(2)
    k = suite.scale(1000, 20)
    t = [v % S.P for v in _rand_ints(rng, k)]
    squares = [v * v % S.P for v in t]
    others = [(S.P - v) % S.P for v in squares if v]  # p = 3 (mod 4): -1 is no square, so neither is -(t^2)
    xs = squares + others + EDGES
    out = P.signer.secp_op("fe_sqrt", rows(xs))
    want_root = [pow(x, (S.P + 1) // 4, S.P) for x in xs]
    assert ints(out[:, :32]) == want_root
    assert list(out[:, 32]) == [1 if w * w % S.P == x % S.P else 0 for w, x in zip(want_root, xs)]
    assert list(out[:k, 32]) == [1] * k and list(out[k:k + len(others), 32]) == [0] * len(others)
    assert all(w in (v, S.P - v) for w, v in zip(want_root[:k], t))


def _pt_rows(pts):
    return np.frombuffer(b"".join(bytes(65)[:64] + b"\x01" if p is None else be(p[0]) + be(p[1]) + b"\x00" for p in pts),
                         np.uint8).reshape(-1, 65).copy()


def _pts(out):
    return [None if r[64] else (int.from_bytes(bytes(r[:32]), "big"), int.from_bytes(bytes(r[32:64]), "big")) for r in out]


def test_point_double_and_add_for_every_pair(P):
    rng = np.random.default_rng(3)
    G2 = S.add(S.G, S.G)
    pts = [S.G, G2]
    for _ in range(suite.scale(60, 6)):  # a walk of random steps: cheap for the reference, arbitrary for the kernel
        pts.append(S.add(pts[-1], pts[int(rng.integers(0, len(pts)))]))
    a = [S.G, S.G, S.G, None, None, S.G, G2, pts[5], pts[5]] + pts[2:] + pts[2:]
    b = [S.G, S.neg(S.G), None, S.G, None, G2, S.G, pts[5], S.neg(pts[5])] + pts[:-2] + pts[2:]
    want = [S.add(x, y) for x, y in zip(a, b)]
    assert want[1] is None and want[4] is None and want[8] is None
    assert _pts(P.signer.secp_op("pt_add", _pt_rows(a), _pt_rows(b))) == want
    assert _pts(P.signer.secp_op("pt_add_affine", _pt_rows(a), _pt_rows(b))) == want
    dbl = pts + [None, S.neg(S.G)]
    assert _pts(P.signer.secp_op("pt_double", _pt_rows(dbl))) == [S.add(x, x) for x in dbl]
    # out-of-range flag bytes count as "infinity", and what comes back is always canonical
    raw = P.signer.secp_op("pt_add", _pt_rows([S.G]), _pt_rows([S.neg(S.G)]))
    assert bytes(raw[0]) == bytes(64) + b"\x01"


# -------------------------------------------------------------------------------------------------------------- recovery
def _run(P, tuples, low_s=False, want="both", ctx=None):
    z, r, s, ids = zip(*tuples)
    # (operands beyond 2^256 cannot be written down: the cases below never make one)
    return P.signer.recover(rows(z), rows(r), rows(s), np.array(ids, np.uint8), low_s=low_s, want=want, ctx=ctx)


def _expect(oracle, tuples, low_s=False):
    st, pk, ad = S.recover_batch(oracle, tuples, S.LOW_S if low_s else 0)
    return (np.frombuffer(b"".join(pk), np.uint8).reshape(-1, 64), np.frombuffer(b"".join(ad), np.uint8).reshape(-1, 20),
            np.frombuffer(st, np.uint8))


def _same(got, want):
    assert np.array_equal(got[2], want[2]), (list(got[2][:16]), list(want[2][:16]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def genuine(oracle):
    """Genuine low-s signatures of random keys over random digests, with their keys and addresses -- computed ONCE.  Key u * w + v
    is a_u + b_v of two random sets (public key A_u + B_v: one addition instead of a scalar multiplication for the reference),
    the nonces likewise; every signature is checked against the verification equation below, a sample through S.recover."""
    rng = np.random.default_rng(11)
    w = suite.scale(64, 6)
    rnd = lambda: [v % (S.N - 1) + 1 for v in _rand_ints(rng, w)]  # noqa: E731
    a, b, c, e = rnd(), rnd(), rnd(), rnd()
    Ap, Bp, Cp, Ep = ([S.mul(v, S.G) for v in vs] for vs in (a, b, c, e))
    tuples, keys = [], []
    for u in range(w):
        for v in range(w):
            d, q = (a[u] + b[v]) % S.N, S.add(Ap[u], Bp[v])
            k, R = (c[v] + e[u]) % S.N, S.add(Cp[v], Ep[u])
            z = int.from_bytes(rng.bytes(32), "big")
            r = R[0] % S.N
            s = pow(k, -1, S.N) * (z + r * d) % S.N
            recid = (R[1] & 1) | (2 if R[0] >= S.N else 0)
            if s > S.N // 2:
                s, recid = S.N - s, recid ^ 1
            assert d and k and r and s and q is not None
            tuples.append((z, r, s, recid))
            keys.append(S.pubkey_bytes(q))
    for i in range(0, len(tuples), max(1, len(tuples) // 24)):
        code, q = S.recover(*tuples[i], S.LOW_S)
        assert code == S.OK and S.pubkey_bytes(q) == keys[i]
    blob = np.frombuffer(b"".join(keys), np.uint8)
    addrs = oracle.keccak256_batch(blob, np.arange(len(keys) + 1, dtype=np.uint64) * 64)[:, 12:]
    assert {t[3] for t in tuples} >= {0, 1}
    return tuples, blob.reshape(-1, 64), np.ascontiguousarray(addrs)


def test_known_answers(P, oracle):
    vec = S.load_vectors()
    e = vec["erecover"]
    tuples = [(int(e["hash"], 16), int(e["r"], 16), int(e["s"], 16), e["recid"])]
    for t in vec["mainnet"]:
        st, pre, r, s, recid = S.tx_signing_parts(t["tx"], 1)
        assert st == S.OK
        tuples.append((int.from_bytes(oracle.keccak256(pre), "big"), r, s, recid))
    pk, ad, st = _run(P, tuples, low_s=True)
    assert list(st) == [0, 0, 0] and bytes(pk[0]).hex() == e["pubkey"]
    assert [bytes(x).hex() for x in ad[1:]] == [t["sender"] for t in vec["mainnet"]]


def test_genuine_signatures_and_their_high_s_twins(P, genuine):
    tuples, keys, addrs = genuine
    n = len(tuples)
    pk, ad, st = _run(P, tuples, low_s=True)
    assert not st.any() and np.array_equal(pk, keys) and np.array_equal(ad, addrs)
    twins = [(z,) + S.high_s_twin(r, s, recid) for z, r, s, recid in tuples]
    pk, ad, st = _run(P, twins, low_s=False)
    assert not st.any() and np.array_equal(pk, keys) and np.array_equal(ad, addrs)
    pk, ad, st = _run(P, twins, low_s=True)
    assert list(st) == [S.HIGH_S] * n and not pk.any() and not ad.any()


def _corner_cases(oracle):
    rng = np.random.default_rng(12)
    cases = []
    d = 0x1234567
    cases.append((0,) + S.sign(d, 0))  # z = 0
    # R = G, -G, 2 G (r = its x, recid = the parity of its y) with u1 = u2 (the first non-zero window adds a point to
    # itself when R = G), u1 = -u2, and u1 + k u2 = 0 (Q at infinity); u = u2 small, window-aligned and random
    for k in (1, S.N - 1, 2):
        R = S.mul(k, S.G)
        r, recid = R[0], R[1] & 1
        assert r < S.N
        for u in (1, 5, 0x10, 0x100, 0xFF, int.from_bytes(rng.bytes(32), "big") % S.N):
            s = u * r % S.N
            for z in ((-s) % S.N, s, k * s % S.N, (-k * s) % S.N):  # u1 = -z / r
                cases.append((z, r, s, recid))
    # r + n < p: recid 2 / 3 reach x = r + n, on and off the curve; the same r with recid 0 / 1
    on = off = 0
    for r in range(1, 200):
        hit = S.lift_x(r + S.N, 0) is not None
        if (hit and on < 4) or (not hit and off < 4):
            on, off = on + hit, off + (not hit)
            for recid in (0, 1, 2, 3):
                cases.append((int.from_bytes(rng.bytes(32), "big"), r, int.from_bytes(rng.bytes(32), "big") % (S.N - 1) + 1, recid))
    assert on == 4 and off == 4
    cases.append((5, S.P - S.N, 7, 2))      # r + n = p exactly
    cases.append((5, S.P - S.N - 1, 7, 3))  # ... p - 1
    edge = (0, S.N, S.N - 1, S.N + 1, M256, 1, S.N // 2, S.N // 2 + 1)
    cases += [(9, r, s, recid) for r in edge for s in edge for recid in (0, 2)]
    cases += [(9, 1, 1, 4), (9, 0, 0, 255), (9, S.N, 1, 4), (M256, M256, M256, 255), (M256, 1, 1, 1), (S.N, S.G[0], 1, 0)]
    return cases


def test_ladder_corner_cases(P, oracle):
    cases = _corner_cases(oracle)
    for low_s in (False, True):
        want = _expect(oracle, cases, low_s)
        _same(_run(P, cases, low_s), want)
        if not low_s:
            seen = set(want[2])
            assert seen >= {S.OK, S.BAD_RANGE, S.BAD_RECID, S.NOT_ON_CURVE, S.INFINITY}, seen
        else:
            assert S.HIGH_S in set(want[2])


def test_batch_sizes_and_a_wave_with_every_second_lane_failing(P, oracle, genuine):
    tuples, keys, addrs = genuine
    bad = [c for c in _corner_cases(oracle) if S.recover(*c, S.LOW_S)[0] != S.OK]
    kinds = {S.recover(*c, S.LOW_S)[0] for c in bad}
    assert len(kinds) >= 5
    for n in suite.scale((1, 63, 64, 65, 257), (1, 65)):
        idx = [i % len(tuples) for i in range(n)]
        pk, ad, st = _run(P, [tuples[i] for i in idx], low_s=True)
        assert not st.any() and np.array_equal(pk, keys[idx]) and np.array_equal(ad, addrs[idx])
    n = suite.scale(130, 66)
    mixed = [tuples[i % len(tuples)] if i % 2 == 0 else bad[(i // 2) % len(bad)] for i in range(n)]
    pk, ad, st = _run(P, mixed, low_s=True)
    for i in range(n):
        if i % 2 == 0:
            j = i % len(tuples)
            assert st[i] == 0 and np.array_equal(pk[i], keys[j]) and np.array_equal(ad[i], addrs[j])
        else:
            assert st[i] == S.recover(*mixed[i], S.LOW_S)[0] and not pk[i].any() and not ad[i].any()


def test_every_output_choice_the_device_form_and_one_context_small_large_small(P, oracle, genuine):
    tuples, keys, addrs = genuine
    some = tuples[:suite.scale(70, 5)] + _corner_cases(oracle)[:suite.scale(40, 6)]
    pk, ad, st = _run(P, some, want="both")
    pk2, st2 = _run(P, some, want="pubkeys")
    ad3, st3 = _run(P, some, want="addresses")
    st4 = _run(P, some, want="status")
    assert np.array_equal(pk, pk2) and np.array_equal(ad, ad3)
    assert np.array_equal(st, st2) and np.array_equal(st, st3) and np.array_equal(st, st4)
    # the device form
    import torch
    ctx = P.context.default_context()
    z, r, s, ids = zip(*some)
    n = len(some)
    dev = [torch.from_numpy(x).cuda() for x in (rows(z), rows(r), rows(s), np.array(ids, np.uint8))]
    d_pk, d_ad, d_st = (torch.full((n * k,), 0xEE, dtype=torch.uint8).cuda() for k in (64, 20, 1))
    ctx.check(ctx._lib.phant_ecrecover_batch_dev(ctx.handle, *[t.data_ptr() for t in dev], n, 0, d_pk.data_ptr(), d_ad.data_ptr(),
                                                 d_st.data_ptr()))
    ctx.sync()
    assert np.array_equal(d_pk.cpu().numpy().reshape(-1, 64), pk) and np.array_equal(d_ad.cpu().numpy().reshape(-1, 20), ad)
    assert np.array_equal(d_st.cpu().numpy(), st)
    # one context: small, large, small again (the staging arena grows and is reused)
    own = ctx if suite.EMULATED else P.context.Context()
    try:
        big = suite.scale(3000, 70)
        for n in (3, big, 2):
            idx = [i % len(tuples) for i in range(n)]
            pk, ad, st = _run(P, [tuples[i] for i in idx], low_s=True, ctx=own)
            assert not st.any() and np.array_equal(pk, keys[idx]) and np.array_equal(ad, addrs[idx])
    finally:
        if own is not ctx:
            own.close()


def test_refused_arguments(P):
    from phant_amd import _lib as L
    ctx = P.context.default_context()
    lib, h = ctx._lib, ctx.handle
    a = np.zeros((2, 32), np.uint8)
    ids, st = np.zeros(2, np.uint8), np.full(2, 0xEE, np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for f in (lib.phant_ecrecover_batch, lib.phant_ecrecover_batch_dev):
        assert f(h, None, None, None, None, 0, 0, None, None, p(st)) == L.OK  # n == 0
        assert f(h, None, p(a), p(a), p(ids), 2, 0, None, None, p(st)) == L.E_INVALID_ARG
        assert f(h, p(a), None, p(a), p(ids), 2, 0, None, None, p(st)) == L.E_INVALID_ARG
        assert f(h, p(a), p(a), None, p(ids), 2, 0, None, None, p(st)) == L.E_INVALID_ARG
        assert f(h, p(a), p(a), p(a), None, 2, 0, None, None, p(st)) == L.E_INVALID_ARG
        assert f(h, p(a), p(a), p(a), p(ids), 2, 2, None, None, p(st)) == L.E_INVALID_ARG  # an unknown flag bit
        assert f(h, p(a), p(a), p(a), p(ids), 2, 0, None, None, None) == L.E_INVALID_ARG   # nothing to write
        assert f(None, p(a), p(a), p(a), p(ids), 2, 0, None, None, p(st)) == L.E_INVALID_ARG
    assert list(st) == [0xEE, 0xEE]
    off = np.zeros(2, np.uint64)
    assert lib.phant_tx_senders(h, None, None, 0, 1, None, p(st)) == L.OK
    assert lib.phant_tx_senders(h, None, p(off), 1, 1, None, None) == L.E_INVALID_ARG
    assert lib.phant_tx_senders(h, None, None, 1, 1, None, p(st)) == L.E_INVALID_ARG
    off[:] = (5, 1)
    assert lib.phant_tx_senders(h, p(a), p(off), 1, 1, None, p(st)) == L.E_INVALID_ARG
    assert lib.phant_diag_secp_op(h, 9, p(a), p(a), 2, p(a)) == L.E_INVALID_ARG
    assert lib.phant_diag_secp_op(h, 0, p(a), None, 2, p(a)) == L.E_INVALID_ARG
    with pytest.raises(ValueError):
        P.signer.recover(a, a, a, ids, want="everything")


# ---------------------------------------------------------------------------------------------------------- transactions
D = 0xC0FFEE0DDF00D


def _addr(oracle, d=D):
    return oracle.keccak256(S.pubkey_bytes(S.mul(d, S.G)))[12:]


def _senders(P, txs, chain_id=1):
    ad, st = P.signer.senders(txs, chain_id)
    return [bytes(x) for x in ad], list(st)


def test_fixture_and_mainnet_senders(P):
    vec = S.load_vectors()
    items = vec["mainnet"] + vec["fixtures"]
    if suite.EMULATED and not suite.FULL:
        items = vec["mainnet"] + vec["fixtures"][::9]
    ad, st = _senders(P, [t["tx"] for t in items])
    assert st == [0] * len(items)
    assert [a.hex() for a in ad] == [t["sender"] for t in items]
    assert _senders(P, []) == ([], [])  # n = 0


def _edge_data_lengths(oracle, typ, kw):
    """data lengths at which the spliced preimage's list header changes form (55 | 56, 255 | 256, 65 535 | 65 536 payload bytes),
    next to the data item's own (0, 1, 55 | 56, 255 | 256)"""
    st, pre, *_ = S.tx_signing_parts(S.make_tx(oracle, 1, typ, 1, data=b"", **kw), 1)
    top = S.rlp_item(pre, 1 if typ else 0, len(pre))
    body0 = top[2] - top[1]  # the payload with empty data (one byte, 0x80)
    enc = lambda L: L + (1 if L <= 55 else 2 if L <= 255 else 3)  # noqa: E731  (its bytes are >= 0x80)
    want = {55, 56, 255, 256, 65535, 65536}
    return sorted({L for L in range(0, 65600) if body0 - 1 + enc(L) in want} | {0, 1, 55, 56, 255, 256})


def test_signed_transactions_of_every_type(P, oracle):
    me = _addr(oracle)
    al = [(b"\x22" * 20, [b"\x01" * 32, b"\x02" * 32]), (b"\x33" * 20, [])]
    shapes = [(0, {}), (0, {"eip155": False}), (0, {"to": b""}), (1, {}), (1, {"access_list": al}), (2, {}),
              (2, {"access_list": al, "to": b""})]
    txs, labels = [], []
    for typ, kw in shapes:
        lengths = _edge_data_lengths(oracle, typ, kw) + [3000]
        if suite.EMULATED and not suite.FULL:
            lengths = lengths[::3]
        for L in lengths:
            txs.append(S.make_tx(oracle, D, typ, 1, data=b"\xd5" * L, nonce=len(txs), **kw))
            labels.append((typ, kw, L))
    forms = {S.tx_signing_parts(t, 1)[1][1 if t[0] < 0x80 else 0] for t in txs}
    if not suite.EMULATED or suite.FULL:
        assert {0xF7, 0xF8, 0xF9, 0xFA} <= forms and min(forms) < 0xF7, forms  # every length form of the spliced header
    ad, st = _senders(P, txs)
    assert st == [0] * len(txs), [lab for lab, code in zip(labels, st) if code]
    assert ad == [me] * len(txs)
    for t in txs[::max(1, len(txs) // 6)]:
        assert S.tx_sender(oracle, t, 1) == (S.OK, me)
    # a chain id of several bytes and of zero in the EIP-155 tail
    for cid in (0, 127, 128, 11155111, (1 << 64) - 1):
        t = [S.make_tx(oracle, D, 0, cid), S.make_tx(oracle, D, 0, cid, eip155=False)]
        assert _senders(P, t, cid) == ([me, me], [0, 0]), cid


def test_transactions_that_fail(P, oracle):
    me = _addr(oracle)
    good = [S.make_tx(oracle, D, 0, 1, data=b"xyz"), S.make_tx(oracle, D, 1, 1, access_list=[(b"\x44" * 20, [b"\x05" * 32])]),
            S.make_tx(oracle, D, 2, 1, data=b"q" * 60)]
    txs = [S.make_tx(oracle, D, 0, 5),                       # signed for another chain
           S.make_tx(oracle, D, 0, 1, v_override=29),
           S.make_tx(oracle, D, 2, 1, v_override=2),         # y_parity 2
           S.make_tx(oracle, D, 1, 1, v_override=1 << 70),
           S.make_tx(oracle, D, 0, 1, high_s=True), S.make_tx(oracle, D, 2, 1, high_s=True),
           b"\x03" + good[2][1:], b"\x00" + good[2][1:], b"\x7f", b"", b"\x80", b"\xc0",
           good[0] + b"\x00", good[1] + b"\x00",
           good[0]]
    want = [S.BAD_V, S.BAD_V, S.BAD_V, S.BAD_V, S.HIGH_S, S.HIGH_S] + [S.BAD_TX] * 8 + [S.OK]
    assert [S.tx_sender(oracle, t, 1)[0] for t in txs] == want
    ad, st = _senders(P, txs)
    assert st == want and ad == [bytes(20)] * (len(txs) - 1) + [me]
    # every truncation of one transaction of each type, good ones in between
    cut = []
    for g in good:
        step = 1 if not suite.EMULATED or suite.FULL else 7
        cut += [g[:k] for k in range(0, len(g), step)] + [g]
    ad, st = _senders(P, cut)
    for t, a, code in zip(cut, ad, st):
        if t in good:
            assert (code, a) == (S.OK, me)
        else:
            assert (code, a) == (S.BAD_TX, bytes(20)), len(t)
            assert S.tx_signing_parts(t, 1)[0] == S.BAD_TX
