"""Blob (type 3) and set-code (type 4) transactions on the device (phant_block_transactions_ex, phant_block_transactions_ex_dev,
phant_amd.types.transaction.block_transactions(fork=)) against tests/tx_ref_forks.py, which defines every output for every byte string,
and against phant_block_transactions for the same bytes where the fork is London.  Every comparison is exact, in both forms.
tests/test_emu_transactions_forks.py runs the same bodies over the kernel sources compiled for the host."""
import ctypes as C

import numpy as np
import pytest

from tests import secp_ref as S
from tests import suite
from tests import tx_ref as T
from tests import tx_ref_forks as F
from tests.test_gpu_transactions import ALL, D, NO_SENDER, OK, E_INVALID_ARG, Raw, _ctx, _data, _first_difference, _huge_lengths, hostile_corpus
from tests.test_gpu_transactions import raw_tx as raw_tx_012

pytestmark = pytest.mark.gpu
TX_EX = tuple(name for name, _, _ in F.TX_OUTPUTS)
AUTH = tuple(name for name, _, _ in F.AUTH_OUTPUTS)
AUTH_NO_RECOVERY = tuple(k for k in AUTH if k not in ("authority", "auth_status"))
WIDTH = {name: np.dtype(dt).itemsize * k for name, dt, k in T.OUTPUTS + F.TX_OUTPUTS + F.AUTH_OUTPUTS}
M64, M256 = F.M64, F.M256
D2 = 0xA11CE  # the private key of the genuine authorizations


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawEx(Raw):
    """phant_txs_ex_in / _out on top of tests/test_gpu_transactions.Raw's buffers"""

    def call_ex(self, ctx, fork, chain_id=1, base_fee=None, gas_limit=None, blob_base_fee=None, recover=True, want=None, auth_cap=None, guard=64,
                flags=None, sizes=None, reserved=0, skew=None, n=None):
        """-> (rc, {output: bytes}, first_bad, n_auth, blob_gas_used); every buffer has `guard` bytes of 0xEE in front of and behind its
        rows; the per-authorization ones have auth_cap rows (None: as many as the definition has tuples: the caller says)"""
        L = self.L
        want = ((ALL if recover else NO_SENDER) + TX_EX + (AUTH if recover else AUTH_NO_RECOVERY)) if want is None else want
        n = self.n if n is None else n
        if flags is None:
            flags = (L.TXS_HAVE_GAS_LIMIT if gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
        fee = None if base_fee is None else np.frombuffer(int(base_fee).to_bytes(32, "big"), np.uint8).copy()
        bfee = None if blob_base_fee is None else np.frombuffer(int(blob_base_fee).to_bytes(32, "big"), np.uint8).copy()
        base = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, self._ptr(self.blob), self._ptr(self.off), self.tx_bytes, chain_id,
                            None if fee is None else fee.ctypes.data, int(gas_limit or 0))
        rows = {k: (n + 1 if k == "auth_first" else (auth_cap or 0) if k in AUTH else n) for k in want}
        size = {k: WIDTH[k] * rows[k] for k in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        ptr = lambda k: self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0xEEEEEEEE, *[ptr(k) for k in ALL])
        arg = L.PhantTxsExIn(C.sizeof(L.PhantTxsExIn), fork, base, None if bfee is None else bfee.ctypes.data, auth_cap or 0, reserved)
        xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE, out, *[ptr(k) for k in TX_EX + AUTH])
        if sizes:
            arg.struct_size, xout.struct_size, arg.base.struct_size, xout.base.struct_size = sizes
        fn = ctx._lib.phant_block_transactions_ex_dev if self.dev else ctx._lib.phant_block_transactions_ex
        rc = fn(ctx.handle, C.byref(arg), C.byref(xout))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        return rc, got, int(xout.base.first_bad), int(xout.n_auth), int(xout.blob_gas_used)


def check_ex(P, oracle, txs, fork, chain_id=1, base_fee=None, gas_limit=None, blob_base_fee=None, recover=True, forms=(False, True), ctx=None):
    """every answer of the _ex call for these transactions against the definition, in both forms -> (the expected flags, the
    expected auth_status)"""
    exp, first_bad, n_auth, blob_gas = F.expected(oracle, txs, chain_id, fork, base_fee, gas_limit, blob_base_fee, recover)
    ctx = ctx or _ctx(P)
    for dev in forms:
        rc, got, fb, na, bg = RawEx(P, txs, dev=dev).call_ex(ctx, fork, chain_id, base_fee, gas_limit, blob_base_fee, recover, auth_cap=n_auth)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert (fb, na, bg) == (first_bad, n_auth, blob_gas), (dev, fb, first_bad, na, n_auth, bg, blob_gas)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    return np.frombuffer(exp["flags"], np.uint32), np.frombuffer(exp["auth_status"], np.uint8)


def _auth(oracle, k=0, chain_id=1, **kw):
    """genuine authorization tuple number k"""
    return F.make_authorization(oracle, D2 + k % 5, chain_id, address=bytes([0x70 + k % 16]) * 20, nonce=k, **kw)


@pytest.fixture(scope="module")
def pool(oracle):
    """transactions of all five types: genuine ones, refused ones, ones that break a rule"""
    al = [(b"\x44" * 20, [b"\x05" * 32, b"\x06" * 32]), (b"\x45" * 20, [])]
    mk = lambda typ, **kw: F.make_tx(oracle, D, typ, 1, **kw)  # noqa: E731
    return [mk(0, data=b"xyz", gas=50000), mk(3, hashes=[F.versioned(k) for k in range(3)], data=_data(90), access_list=al),
            mk(1, access_list=al, data=_data(200), gas=10**6), mk(4, auths=[_auth(oracle, 0), _auth(oracle, 1)], data=_data(40)),
            mk(2, access_list=al, data=_data(700), gas=10**6), mk(4, auths=[], nonce=3), mk(3, hashes=[], nonce=4), b"", b"\x05\xc0",
            mk(3, to=b"", nonce=5), mk(4, auths=[_auth(oracle, 2, chain_id=0)], high_s=True), mk(3, hashes=[F.versioned(1, 2)], blob_fee=1),
            F.raw_tx(4, v=2), mk(2, to=b"", data=_data(300), gas=10**6), mk(4, auths=[_auth(oracle, k) for k in range(3, 7)], gas=99999)[:-1],
            mk(3, gas=21000, data=_data(30)), mk(0, gas=21000 + 16 * 20, data=b"\x01" * 20), mk(4, auths=[_auth(oracle, 7)], gas=40000)]


# ------------------------------------------------------------------------------------------------------ batch sizes, forks
def test_batch_sizes_at_every_fork(P, oracle, pool):
    """0, 1, 63, 64 and 65 transactions of all five types at PRAGUE; the same bytes at CANCUN (type 4 undecodable) and at LONDON (types
    3 and 4 undecodable), where every output equals what phant_block_transactions answers"""
    for n in suite.scale((0, 1, 63, 64, 65), (0, 1, 65)):
        txs = [pool[(i * 5 + n) % len(pool)] for i in range(n)]
        flags, _ = check_ex(P, oracle, txs, F.PRAGUE, base_fee=7, gas_limit=30_000_000, blob_base_fee=3)
        assert n < 18 or len(set(flags.tolist())) >= 10
        typ = np.asarray([t[0] if t and t[0] < 0x80 else 0 for t in txs])
        cancun, _ = check_ex(P, oracle, txs, F.CANCUN, base_fee=7, gas_limit=30_000_000, blob_base_fee=3)
        assert (cancun[typ == 4] == T.UNDECODABLE).all() and ((cancun[typ == 3] & T.UNDECODABLE) == (flags[typ == 3] & T.UNDECODABLE)).all()
        london, _ = check_ex(P, oracle, txs, F.LONDON, base_fee=7, gas_limit=30_000_000, blob_base_fee=3)
        assert (london[typ >= 3] == T.UNDECODABLE).all()
        old, old_first_bad = T.expected(oracle, txs, 1, 7, 30_000_000)
        for dev in (False, True):
            raw = RawEx(P, txs, dev=dev)
            rc0, got0, fb0 = raw.call(_ctx(P), base_fee=7, gas_limit=30_000_000)
            rc1, got1, fb1, na, bg = raw.call_ex(_ctx(P), F.LONDON, base_fee=7, gas_limit=30_000_000, want=ALL)
            assert rc0 == rc1 == OK and fb0 == fb1 == old_first_bad and (na, bg) == (0, 0)
            for k in ALL:
                assert got0[k] == got1[k] == old[k], (dev, k)


def test_subsets_of_the_new_outputs(P, oracle, pool):
    """each new output wanted alone and seeded random subsets of all of them: the span the host form fetches ends at every position"""
    txs = pool[:suite.scale(18, 6)]
    exp, first_bad, n_auth, blob_gas = F.expected(oracle, txs, 1, F.PRAGUE, 7)
    rng = np.random.default_rng(5)
    everything = ALL + TX_EX + AUTH
    subsets = [()] + [(k,) for k in TX_EX + AUTH] + [tuple(k for k in everything if rng.integers(0, 2)) for _ in range(suite.scale(24, 3))]
    if suite.EMULATED and not suite.FULL:
        subsets = subsets[::4]
    for dev in (False, True):
        raw = RawEx(P, txs, dev=dev)
        for want in subsets:
            rc, got, fb, na, bg = raw.call_ex(_ctx(P), F.PRAGUE, base_fee=7, want=want, auth_cap=n_auth)
            assert rc == OK and (fb, na, bg) == (first_bad, n_auth, blob_gas), (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)


# ---------------------------------------------------------------------------------------------------- authorization totals
def _spread(total):
    """tuples per type-4 transaction, uneven, with a transaction that has none between two that have some"""
    return {0: [0, 0], 1: [0, 1, 0], 63: [20, 0, 1, 42], 64: [1, 0, 63], 65: [65, 0], 257: [65, 0, 100, 1, 0, 91]}[total]


@pytest.fixture(scope="module")
def tuples(oracle):
    """257 authorization tuples, every fourth genuine (a signature is the expensive part of the definition), the others well-formed"""
    return [_auth(oracle, k) if k % 4 == 0 else F.raw_tuple(1, bytes([k % 251]) * 20, k, k % 2, 1 + k, 2 + k) for k in range(257)]


def test_authorization_totals(P, oracle, tuples):
    """0, 1, 63, 64, 65 and 257 tuples over the transactions of a call, other types in between; auth_first against the definition"""
    for total in suite.scale((0, 1, 63, 64, 65, 257), (0, 1, 65)):
        txs, at = [], 0
        for i, k in enumerate(_spread(total)):
            txs.append(F.raw_tx(4, auths=tuples[at:at + k], nonce=i))
            txs.append(raw_tx_012(i % 3, nonce=i) if i % 2 else F.raw_tx(3, nonce=i))
            at += k
        exp, _, n_auth, _ = F.expected(oracle, txs, 1, F.PRAGUE)
        assert n_auth == total and np.frombuffer(exp["auth_first"], np.uint32)[::2].tolist() == np.cumsum([0] + _spread(total)).tolist()
        check_ex(P, oracle, txs, F.PRAGUE)
        check_ex(P, oracle, txs, F.PRAGUE, recover=False, forms=(True,))


def test_auth_cap(P, oracle, tuples):
    """auth_cap of 0, n_auth - 1 and n_auth: the rows beyond it are not written (the guards behind the written rows stay), n_auth and
    auth_first are complete, and the call is PHANT_OK"""
    txs = [F.raw_tx(4, auths=tuples[:3]), F.raw_tx(3), F.raw_tx(4, auths=tuples[3:suite.scale(70, 9)], nonce=1)]
    exp, first_bad, n_auth, _ = F.expected(oracle, txs, 1, F.PRAGUE)
    for dev in (False, True):
        for cap in (0, n_auth - 1, n_auth):
            rc, got, fb, na, _ = RawEx(P, txs, dev=dev).call_ex(_ctx(P), F.PRAGUE, auth_cap=cap, want=("flags", "auth_first") + AUTH)
            assert rc == OK and fb == first_bad and na == n_auth and got["auth_first"] == exp["auth_first"], (dev, cap)
            for k in AUTH:
                assert got[k, "guards"] and got[k] == exp[k][:cap * WIDTH[k]], (dev, cap, k)


# ------------------------------------------------------------------------------------------------------------- seams
def _lengths(tx):
    """(raw bytes, signing preimage bytes)"""
    st, f, sig = F.decode(tx, 1, F.PRAGUE)
    assert st == S.OK
    return len(tx), len(sig[0])


def test_block_seams_of_both_sponges(P, oracle):
    """raw length and signing-preimage length each at 135 .. 137 and 271 .. 273 bytes for types 3 and 4 (the approach of
    tests/test_gpu_transactions.py: the calldata's length is bisected, a longer value shifts the lengths where the calldata's header grows)"""
    seams = (135, 136, 137, 271, 272, 273)
    txs = []
    for kw in (dict(typ=3, r=1, s=2), dict(typ=4, r=1, s=2, auths=[F.raw_tuple(1, b"\x77" * 20, 0, 0, 1, 1)])):
        for which in (0, 1):
            for t in seams:
                for value in (1, 0x100, 0x10000):
                    n = next((n for n in range(300) if _lengths(F.raw_tx(data=b"\xd5" * n, value=value, **kw))[which] >= t), None)
                    if n is not None and _lengths(F.raw_tx(data=b"\xd5" * n, value=value, **kw))[which] == t:
                        txs.append(F.raw_tx(data=_data(n), value=value, **kw))
                        break
                else:
                    raise AssertionError((kw["typ"], which, t))
    assert len(txs) == 24 and {_lengths(t)[0] for t in txs} >= set(seams) and {_lengths(t)[1] for t in txs} >= set(seams)
    flags, _ = check_ex(P, oracle, txs, F.PRAGUE, recover=False)
    assert not (flags & F.ERROR_BITS).any()


def test_authorization_message_seams(P, oracle):
    """the message's list payload at 55 and 56 bytes, where its header grows to two bytes (a payload is rlp(chain_id) + 21 + rlp(nonce): 55
    with a chain id of 24 bytes and a nonce of 8, or of 32 bytes and nonce 0; chain ids of 13 and 14 bytes stay far below); chain id 0,
    the call's own and 2^256 - 1; nonces of 0, one byte below and from 0x80, eight bytes"""
    ids = (0, 1, 0x7F, 0x80, (1 << 100) + 5, 1 << 104, 1 << 184, 1 << 192, M256)
    nonces = (0, 0x7F, 0x80, M64 - 1)
    payloads = {S.rlp_item(m, 1, len(m))[2] - S.rlp_item(m, 1, len(m))[1] for c in ids for n in nonces for m in [F.authorization_message(c, b"\x77" * 20, n)]}
    assert {23, 37, 55, 56, 63} <= payloads and max(len(F.authorization_message(M256, b"\x77" * 20, n)) for n in nonces) == 66
    auths = [F.make_authorization(oracle, D2, c, nonce=n) for c in ids for n in nonces]
    txs = [F.raw_tx(4, auths=auths[:11]), F.raw_tx(3), F.raw_tx(4, auths=auths[11:], nonce=1)]
    flags, status = check_ex(P, oracle, txs, F.PRAGUE)
    assert not (flags & (F.ERROR_BITS ^ T.SIGNATURE)).any() and status.tolist() == [S.OK] * 8 + [F.AUTH_CHAIN_ID] * 28  # (nobody signed the transactions)
    # the call's own chain id of eight bytes
    big = [F.make_authorization(oracle, D2, c, nonce=3) for c in (M64, M64 - 1, 1 << 64, 0)]
    _, status = check_ex(P, oracle, [F.raw_tx(4, chain_id=M64, auths=big)], F.PRAGUE, chain_id=M64)
    assert status.tolist() == [S.OK, F.AUTH_CHAIN_ID, F.AUTH_CHAIN_ID, S.OK]


# ------------------------------------------------------------------------------------------------------- hostile bytes
@pytest.mark.parametrize("typ", (3, 4))
def test_hostile_bytes(P, oracle, typ):
    """one call over every truncation, single-byte replacement and 2^64 - 1 length of a subject: flags, sig_status, auth_first and
    auth_status (the whole of every output) equal the definition's"""
    al = [(b"\x44" * 20, [])]
    kw = dict(hashes=[F.versioned(0), F.versioned(1)]) if typ == 3 else dict(auths=[_auth(oracle, 0), F.raw_tuple(0, b"\x78" * 20, 1, 1, 5, 6)])
    tx = F.make_tx(oracle, D, typ, 1, data=b"\x00\x9a\x01", access_list=al, gas=200000, **kw)  # (short: the definition recovers every entry)
    corpus = hostile_corpus(tx) + _huge_lengths(tx)
    if suite.EMULATED and not suite.FULL:
        corpus = corpus[::9] + _huge_lengths(tx)
    flags, status = check_ex(P, oracle, corpus, F.PRAGUE, base_fee=3, gas_limit=10**7, blob_base_fee=2)
    assert (flags & T.UNDECODABLE).any() and (flags == 0).any()
    if not suite.EMULATED or suite.FULL:
        assert (flags & T.BAD_V).any() and (flags & T.SIGNATURE).any()
    if typ == 4 and (not suite.EMULATED or suite.FULL):
        assert {S.OK, S.BAD_V, F.AUTH_CHAIN_ID} <= set(status.tolist()) and set(status.tolist()) & {S.BAD_RANGE, S.HIGH_S, S.NOT_ON_CURVE}


# ------------------------------------------------------------------------------------------------------ rule boundaries
def test_rule_boundaries(P, oracle):
    base, blob_base = 1000, 77
    d = _data(100)
    zeros = d.count(0)
    floor = 21000 + 10 * (zeros + 4 * (100 - zeros))
    intrinsic = T.intrinsic_gas(d, False, 0, 0)
    assert intrinsic < floor == F.floor_gas(d)
    txs, want = [], []

    def case(tx, bits):
        txs.append(tx)
        want.append(bits)

    for fee, bits in ((blob_base - 1, F.BLOB_FEE_BELOW_BASE), (blob_base, 0), (blob_base + 1, 0)):
        case(F.raw_tx(3, blob_fee=fee), bits)
    case(F.raw_tx(4, blob_fee=0), 0)  # (no blob fee rule for type 4)
    case(F.raw_tx(3, hashes=[], blob_fee=blob_base), F.BLOB_NONE)
    hs = [F.versioned(k) for k in range(4)]
    case(F.raw_tx(3, hashes=[F.versioned(0, 2)] + hs[1:], blob_fee=blob_base), F.BLOB_VERSION)
    case(F.raw_tx(3, hashes=hs[:3] + [F.versioned(3, 2)], blob_fee=blob_base), F.BLOB_VERSION)
    case(F.raw_tx(3, hashes=hs[:3] + [F.versioned(3, 0)], blob_fee=blob_base), F.BLOB_VERSION)
    case(F.raw_tx(3, to=b"", blob_fee=blob_base), F.NO_TO | T.IS_CREATE)
    case(F.raw_tx(4, to=b""), F.NO_TO | T.IS_CREATE)
    case(F.raw_tx(4, auths=[]), F.AUTH_NONE)
    # the floor, where the intrinsic gas is below it ...
    for typ in (0, 2):
        case(raw_tx_012(typ, data=d, gas=floor - 1), F.FLOOR_GAS)
        case(raw_tx_012(typ, data=d, gas=floor), 0)
    case(F.raw_tx(3, data=d, gas=floor - 1, blob_fee=blob_base), F.FLOOR_GAS)
    case(F.raw_tx(3, data=d, gas=floor, blob_fee=blob_base), 0)
    case(F.raw_tx(3, data=d, gas=intrinsic - 1, blob_fee=blob_base), F.FLOOR_GAS | T.INTRINSIC_GAS)
    # ... and where it is above (a creation; two authorizations)
    create = T.intrinsic_gas(d, True, 0, 0)
    assert create > floor
    case(raw_tx_012(2, to=b"", data=d, gas=floor - 1), F.FLOOR_GAS | T.INTRINSIC_GAS | T.IS_CREATE)
    case(raw_tx_012(2, to=b"", data=d, gas=floor), T.INTRINSIC_GAS | T.IS_CREATE)
    case(raw_tx_012(2, to=b"", data=d, gas=create), T.IS_CREATE)
    two = [F.raw_tuple(1, b"\x77" * 20, k, 0, 1, 1) for k in range(2)]
    case(F.raw_tx(4, auths=two, data=d, gas=intrinsic + 50000 - 1), T.INTRINSIC_GAS)
    case(F.raw_tx(4, auths=two, data=d, gas=intrinsic + 50000), 0)
    # an upfront cost of exactly 2^256 - 1 reached through the blob term, and one more
    blob_term = 3 * 131072 * (1 << 200)
    case(F.raw_tx(3, hashes=hs[:3], blob_fee=1 << 200, max_fee=base, gas=21000, value=M256 - 21000 * base - blob_term), 0)
    case(F.raw_tx(3, hashes=hs[:3], blob_fee=1 << 200, max_fee=base, gas=21000, value=M256 - 21000 * base - blob_term + 1), T.COST_OVERFLOW)
    case(F.raw_tx(3, hashes=hs[:3], blob_fee=M256, max_fee=base, gas=21000, value=0), T.COST_OVERFLOW)
    case(F.raw_tx(3, hashes=[hs[0]], blob_fee=(M256 - 21000 * base) // 131072, max_fee=base, gas=21000, value=(M256 - 21000 * base) % 131072), 0)
    # the rules of type 2 on both types, several bits together
    case(F.raw_tx(3, max_fee=5000, max_priority=5001, blob_fee=blob_base), T.PRIORITY_ABOVE_MAX)
    case(F.raw_tx(4, max_fee=999, max_priority=1), T.FEE_BELOW_BASE)
    case(F.raw_tx(3, chain_id=2, blob_fee=blob_base), T.CHAIN_ID)
    case(F.raw_tx(4, chain_id=2), T.CHAIN_ID)
    case(F.raw_tx(3, chain_id=3, max_fee=5, max_priority=9, gas=100, nonce=M64, to=b"", hashes=[F.versioned(0, 3)], blob_fee=1, v=2),
         T.BAD_V | T.CHAIN_ID | T.PRIORITY_ABOVE_MAX | T.FEE_BELOW_BASE | T.INTRINSIC_GAS | T.NONCE_MAX | T.IS_CREATE | F.NO_TO | F.BLOB_VERSION
         | F.BLOB_FEE_BELOW_BASE | F.FLOOR_GAS)
    case(F.raw_tx(4, auths=[], to=b"", gas=30_000_001), T.GAS_ABOVE_BLOCK | T.IS_CREATE | F.NO_TO | F.AUTH_NONE)
    flags, _ = check_ex(P, oracle, txs, F.PRAGUE, base_fee=base, gas_limit=30_000_000, blob_base_fee=blob_base, recover=False)
    assert [hex(f) for f in flags] == [hex(b) for b in want]
    X = P.types.transaction
    r = X.block_transactions(txs, 1, base_fee=base, block_gas_limit=30_000_000, recover=False, fork=X.FORK_PRAGUE, blob_base_fee=blob_base)
    assert r.first_bad == 0 and r.errors(1) == [] and r.errors(len(txs) - 1) == ["GasAboveBlock", "NoTo", "AuthNone"]
    assert int(r.floor_gas[11]) == floor and int(r.intrinsic_gas[22]) == intrinsic + 50000
    assert bytes(r.upfront_cost[23]) == b"\xff" * 32 and bytes(r.upfront_cost[24]) == bytes(32) and bytes(r.upfront_cost[26]) == b"\xff" * 32
    assert check_ex(P, oracle, txs[1:4], F.PRAGUE, base_fee=base, blob_base_fee=blob_base, recover=False)[0].tolist() == [0, 0, 0]  # first_bad = n
    # blob_base_fee NULL: that rule is skipped; below PRAGUE: no floor, and type 4 does not decode
    flags, _ = check_ex(P, oracle, txs, F.PRAGUE, base_fee=base, gas_limit=30_000_000, recover=False)
    assert not (flags & F.BLOB_FEE_BELOW_BASE).any() and (flags & F.FLOOR_GAS).any()
    flags, _ = check_ex(P, oracle, txs, F.CANCUN, base_fee=base, gas_limit=30_000_000, blob_base_fee=blob_base, recover=False)
    assert not (flags & F.FLOOR_GAS).any() and (flags & F.BLOB_FEE_BELOW_BASE).any()


# ------------------------------------------------------------------------------------------------------ tuple verdicts
def test_tuple_verdicts(P, oracle):
    """a foreign chain id, nonce 2^64 - 1, y_parity 2, a high-s twin, r = 0: each a status of its tuple, and the transaction stays
    unflagged; a genuine tuple recovers its signer's address"""
    me = oracle.keccak256(S.pubkey_bytes(S.mul(D2, S.G)))[12:]
    auths = [F.make_authorization(oracle, D2, 1), F.make_authorization(oracle, D2, 0, nonce=5), F.make_authorization(oracle, D2, 2),
             F.make_authorization(oracle, D2, 1, nonce=M64), F.make_authorization(oracle, D2, 1, y_parity=2), F.make_authorization(oracle, D2, 1, high_s=True),
             F.make_authorization(oracle, D2, 1, r=0), F.make_authorization(oracle, D2, 2, nonce=M64, y_parity=3), F.make_authorization(oracle, D2, 1, nonce=9)]
    want = [S.OK, S.OK, F.AUTH_CHAIN_ID, F.AUTH_NONCE_MAX, S.BAD_V, S.HIGH_S, S.BAD_RANGE, F.AUTH_CHAIN_ID, S.OK]
    txs = [F.make_tx(oracle, D, 4, 1, auths=auths[:4]), F.make_tx(oracle, D, 4, 1, auths=auths[4:], nonce=1)]
    flags, status = check_ex(P, oracle, txs, F.PRAGUE, base_fee=7, gas_limit=30_000_000)
    assert status.tolist() == want and flags.tolist() == [0, 0]
    r = P.types.transaction.block_transactions(txs, 1, fork=F.PRAGUE)
    assert [bytes(a) for a in r.authority] == [me if s == S.OK else bytes(20) for s in want] and r.first_bad == 2 and r.n_auth == 9


def test_blob_gas_used(P, oracle):
    hs = [F.versioned(k) for k in range(6)]
    for txs, blobs in (([F.raw_tx(3, hashes=[]), raw_tx_012(2)], 0), ([F.raw_tx(3)], 1),
                       ([F.raw_tx(3, hashes=hs), raw_tx_012(0), F.raw_tx(3, hashes=hs[:2], v=2), F.raw_tx(3, hashes=hs[:3])[:-1], F.raw_tx(4)], 8)):
        for dev in (False, True):
            rc, _, _, _, used = RawEx(P, txs, dev=dev).call_ex(_ctx(P), F.PRAGUE, want=("flags",), recover=False)
            assert rc == OK and used == 131072 * blobs == F.expected(oracle, txs, 1, F.PRAGUE, recover=False)[3]


# ---------------------------------------------------------------------------------------------------- refused arguments
def test_refused_arguments(P, oracle, pool):
    """each returns PHANT_E_INVALID_ARG and touches nothing"""
    ctx = _ctx(P)
    txs = pool[:6]
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantTxsExIn), C.sizeof(L.PhantTxsExOut), C.sizeof(L.PhantTxsIn), C.sizeof(L.PhantTxsOut))

    def refused(raw, **kw):
        kw.setdefault("auth_cap", 8)
        rc, got, fb, na, bg = raw.call_ex(ctx, kw.pop("fork", F.PRAGUE), **kw)
        assert rc == E_INVALID_ARG, (rc, kw)
        assert fb == 0xEEEEEEEE and na == 0xEEEEEEEE and bg == 0xEEEEEEEEEEEEEEEE, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawEx(P, txs, dev=dev)
        for k in range(4):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        refused(raw, fork=3)
        refused(raw, fork=0xFFFFFFFF)
        refused(raw, reserved=1)
        refused(raw, flags=4)
        refused(raw, recover=False, want=("flags", "authority"))
        refused(raw, recover=False, want=("auth_status",))
        refused(raw, recover=False, want=("sender", "auth_hash"))
    dev = RawEx(P, txs, dev=True)
    for k, by in (("blob_off", 4), ("floor_gas", 2), ("auth_nonce", 1), ("blobs", 2), ("auth_first", 3)):
        refused(dev, skew={k: by})
    rc, got, fb, na, _ = dev.call_ex(ctx, F.PRAGUE, auth_cap=8, skew={"max_fee_per_blob_gas": 1, "auth_sig": 3, "authority": 1})  # byte arrays need no alignment
    assert rc == OK and na == 2
    for d in (False, True):
        rc, got, fb, na, bg = RawEx(P, txs, dev=d).call_ex(ctx, F.PRAGUE, n=0, want=("auth_first", "flags"))
        assert rc == OK and (fb, na, bg) == (0, 0, 0) and got["auth_first"] == bytes(4)


# ------------------------------------------------------------------------------------------------------------ python
def test_the_python_result(P, oracle, pool):
    X = P.types.transaction
    r = X.block_transactions(pool, 1, base_fee=7, block_gas_limit=30_000_000, fork=X.FORK_PRAGUE, blob_base_fee=3)
    exp, first_bad, n_auth, blob_gas = F.expected(oracle, pool, 1, F.PRAGUE, 7, 30_000_000, 3)
    assert (r.first_bad, r.n_auth, r.blob_gas_used, r.n) == (first_bad, n_auth, blob_gas, len(pool)) and n_auth == 5 and blob_gas == 131072 * 6
    for name, _, _ in T.OUTPUTS + F.TX_OUTPUTS + F.AUTH_OUTPUTS:
        assert getattr(r, name).tobytes() == exp[name], name
    assert [bytes(h) for h in r.versioned_hashes(1)] == [F.versioned(k) for k in range(3)] and len(r.versioned_hashes(0)) == 0
    a = r.authorizations(3)
    assert len(a["auth_status"]) == 2 and a["auth_nonce"].tolist() == [0, 1] and not a["auth_status"].any()
    assert len(r.authorizations(4)["authority"]) == 0 and r.authorizations(10)["auth_status"].tolist() == [S.OK]
    assert r.errors(0) == [] and r.errors(5) == ["AuthNone"] and r.errors(6) == ["BlobNone"] and r.errors(9) == ["NoTo"] and r.errors(10) == ["Signature"]
    assert r.errors(11) == ["BlobVersion", "BlobFeeBelowBase"] and r.errors(15) == ["IntrinsicGas", "FloorGas"] and X.FLAG_NAMES_EX[17] == "FloorGas"
    quiet = X.block_transactions(pool, 1, recover=False, fork=X.FORK_PRAGUE)
    assert not hasattr(quiet, "authority") and not hasattr(quiet, "sender") and (quiet.auth_hash == r.auth_hash).all() and quiet.n_auth == 5
    cancun = X.block_transactions(pool, 1, fork=X.FORK_CANCUN)
    assert cancun.n_auth == 0 and cancun.blob_gas_used == blob_gas and cancun.errors(3) == ["Undecodable"] and len(cancun.auth_status) == 0
    old = X.block_transactions(pool, 1, base_fee=7)
    assert old.fork is None and not hasattr(old, "floor_gas") and old.errors(1) == ["Undecodable"]
    empty = X.block_transactions([], 1, fork=X.FORK_PRAGUE)
    assert empty.n == 0 and empty.first_bad == 0 and empty.n_auth == 0 and empty.auth_first.tolist() == [0]
    assert X.blob_base_fee(0) == 1 and X.blob_base_fee(10**7, X.FORK_CANCUN) == F.blob_base_fee(10**7, F.CANCUN) > X.blob_base_fee(10**7)
