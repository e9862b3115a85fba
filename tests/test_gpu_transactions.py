"""A block's transactions on the device (phant_block_transactions, phant_block_transactions_dev, phant_amd.types.transaction) against
tests/tx_ref.py, which defines every output for every byte string, against phant_tx_senders for the same bytes, and against the
fixtures' and the mainnet transactions.  Every comparison is exact.  tests/test_emu_transactions.py runs the same bodies over the kernel
sources compiled for the host, at the sizes tests/suite.py gives it."""
import ctypes as C

import numpy as np
import pytest

from tests import secp_ref as S
from tests import suite
from tests import tx_ref as T

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG, E_UNSUPPORTED = 0, -1, -6
ALL = tuple(name for name, _, _ in T.OUTPUTS)
NO_SENDER = tuple(k for k in ALL if k not in ("sender", "sig_status"))
WIDTH = {name: np.dtype(dt).itemsize * k for name, dt, k in T.OUTPUTS}
D = 0xC0FFEE  # the private key of the genuine transactions
R0, S0 = int.from_bytes(bytes(range(0x81, 0xA1)), "big"), int.from_bytes(bytes(range(0x21, 0x41)), "big")  # a signature nobody made
M64, M256 = (1 << 64) - 1, (1 << 256) - 1


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


# -------------------------------------------------------------------------------------------------- transactions by hand
def access_list(entries):
    return S.rlp_list([S.rlp_list([S.rlp_bytes(a), S.rlp_list([S.rlp_bytes(k) for k in keys])]) for a, keys in entries])


def raw_tx(typ, chain_id=1, nonce=0, gas_price=10**9, gas=10**6, to=b"\x11" * 20, value=1, data=b"", al=b"\xc0", v=None, r=R0, s=S0, max_priority=2,
           eip155=True):
    """an UNSIGNED raw transaction (r, s as given): al = the access list's whole encoding"""
    if v is None:
        v = 0 if typ else (35 + 2 * chain_id if eip155 else 27)
    if typ == 0:
        items = [S.rlp_int(nonce), S.rlp_int(gas_price), S.rlp_int(gas), S.rlp_bytes(to), S.rlp_int(value), S.rlp_bytes(data)]
    elif typ == 1:
        items = [S.rlp_int(chain_id), S.rlp_int(nonce), S.rlp_int(gas_price), S.rlp_int(gas), S.rlp_bytes(to), S.rlp_int(value), S.rlp_bytes(data), al]
    else:
        items = [S.rlp_int(chain_id), S.rlp_int(nonce), S.rlp_int(max_priority), S.rlp_int(gas_price), S.rlp_int(gas), S.rlp_bytes(to), S.rlp_int(value),
                 S.rlp_bytes(data), al]
    return (bytes([typ]) if typ else b"") + S.rlp_list(items + [S.rlp_int(v), S.rlp_int(r), S.rlp_int(s)])


def _data(n, seed=0):
    """n bytes, a third of them zero"""
    b = np.random.default_rng(1000 + n + seed).integers(0, 256, n, dtype=np.uint8)
    b[::3] = 0
    return b.tobytes()


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_txs_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, txs, dev=False, off=None, blob=None):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        b, o = P.types.transaction.pack(txs)
        self.blob = self._up(b if blob is None else blob)
        self.off = self._up(o if off is None else np.asarray(off, np.uint64))
        self.n = len(o if off is None else off) - 1
        self.tx_bytes = int((o if off is None else off)[-1])

    def _up(self, a):
        if not self.dev:
            return a
        return self.torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    def _ptr(self, x):
        return None if x is None else x.data_ptr() if self.dev else x.ctypes.data

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, chain_id=1, base_fee=None, gas_limit=None, recover=True, want=None, flags=None, guard=64, n=None, null_in=(), skew=None,
             sizes=None):
        """-> (rc, {output: bytes}, first_bad); every buffer has `guard` bytes of 0xEE in front of and behind its rows.  skew: {output: bytes
        its pointer is moved up by}"""
        L = self.L
        want = (ALL if recover else NO_SENDER) if want is None else want
        n = self.n if n is None else n
        if flags is None:
            flags = (L.TXS_HAVE_GAS_LIMIT if gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
        fee = None if base_fee is None else np.frombuffer(int(base_fee).to_bytes(32, "big"), np.uint8).copy()
        arg = L.PhantTxsIn(C.sizeof(L.PhantTxsIn), n, flags, 0, None if "txs" in null_in else self._ptr(self.blob),
                           None if "tx_off" in null_in else self._ptr(self.off), self.tx_bytes, chain_id, None if fee is None else fee.ctypes.data,
                           int(gas_limit or 0))
        size = {k: WIDTH[k] * n for k in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0xEEEEEEEE, *[self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None for k in ALL])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_transactions_dev if self.dev else ctx._lib.phant_block_transactions
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            assert (b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all(), k  # nothing in front of or behind the rows
            got[k] = b[at:at + size[k]].tobytes()
        return rc, got, int(out.first_bad)


def _first_difference(a, b, width):
    for i in range(0, max(len(a), len(b)), width):
        if a[i:i + width] != b[i:i + width]:
            return i // width, a[i:i + width].hex(), b[i:i + width].hex()
    return None


def check_call(P, oracle, txs, chain_id=1, base_fee=None, gas_limit=None, recover=True, forms=(False, True), want=None, ctx=None):
    """every answer of the call for these transactions against the definition, in both forms -> the expected flags"""
    exp, first_bad = T.expected(oracle, txs, chain_id, base_fee, gas_limit, recover)
    ctx = ctx or _ctx(P)
    for dev in forms:
        rc, got, fb = Raw(P, txs, dev=dev).call(ctx, chain_id, base_fee, gas_limit, recover, want)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert fb == first_bad, (dev, fb, first_bad)
        for k in got:
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    return np.frombuffer(exp["flags"], np.uint32)


@pytest.fixture(scope="module")
def pool(oracle):
    """a dozen transactions of every kind: genuine ones of each type, refused ones, ones that break a rule"""
    al = [(b"\x44" * 20, [b"\x05" * 32, b"\x06" * 32]), (b"\x45" * 20, [])]
    return [S.make_tx(oracle, D, 0, 1, data=b"xyz", gas=50000), S.make_tx(oracle, D, 0, 1, eip155=False, nonce=1, gas=21000),
            S.make_tx(oracle, D, 1, 1, access_list=al, data=_data(200), gas=10**6), S.make_tx(oracle, D, 2, 1, access_list=al, data=_data(700), gas=10**6),
            S.make_tx(oracle, D, 2, 1, to=b"", data=_data(300), gas=10**6), b"", b"\x03\xc0", S.make_tx(oracle, D, 0, 1, v_override=29),
            S.make_tx(oracle, D, 2, 1, high_s=True), S.make_tx(oracle, D, 2, 5), S.make_tx(oracle, D, 0, 1, gas=20999),
            raw_tx(2, gas_price=5, max_priority=6), S.make_tx(oracle, D, 1, 1, data=_data(136))[:-1], raw_tx(0, data=_data(5000))]


# ------------------------------------------------------------------------------------------------------ batch sizes, outputs
def test_batch_sizes_in_both_forms(P, oracle, pool):
    for n in suite.scale((0, 1, 63, 64, 65, 257), (0, 1, 65)):
        txs = [pool[(i * 5 + n) % len(pool)] for i in range(n)]
        flags = check_call(P, oracle, txs, base_fee=7, gas_limit=30_000_000)
        assert n < 14 or len(set(flags.tolist())) >= 8


def test_subsets_of_outputs(P, oracle, pool):
    """each output wanted alone, each left out alone, none, and seeded random subsets: the outputs are copied one by one, independent of
    each other but for the end of the span the host form fetches, which the single ones and the random ones move over every position"""
    txs = pool[:suite.scale(14, 6)]
    exp, first_bad = T.expected(oracle, txs, 1, 7, None, True)
    rng = np.random.default_rng(3)
    subsets = [()] + [(k,) for k in ALL] + [tuple(x for x in ALL if x != k) for k in ALL]
    subsets += [tuple(k for k in ALL if rng.integers(0, 2)) for _ in range(suite.scale(32, 4))]
    if suite.EMULATED and not suite.FULL:
        subsets = subsets[::5]
    for dev in (False, True):
        raw = Raw(P, txs, dev=dev)
        for want in subsets:
            rc, got, fb = raw.call(_ctx(P), base_fee=7, want=want)
            assert rc == OK and fb == first_bad, (dev, want)
            for k in want:
                assert got[k] == exp[k], (dev, want, k)


def test_one_context_small_large_small(P, oracle, pool):
    ctx = _ctx(P) if suite.EMULATED else P.context.Context()
    try:
        big = [pool[i % len(pool)] for i in range(suite.scale(3000, 70))]
        for txs in (pool[:3], big, pool[3:5]):
            check_call(P, oracle, txs, base_fee=7, ctx=ctx)
    finally:
        if not suite.EMULATED:
            ctx.close()


def test_a_call_beyond_the_pinned_stage(P, oracle):
    """more bytes than the 8 MiB stage holds: the same answers by plain copies; and the long-transaction path (49 KB of calldata in one lane)"""
    txs = [raw_tx(i % 3, nonce=i, data=_data(49152 + (i % 2), i), to=b"" if i % 2 else b"\x22" * 20, gas=10**7) for i in range(suite.scale(180, 3))]
    txs += [raw_tx(0)]
    flags = check_call(P, oracle, txs, recover=False)
    assert (flags[1] & T.INITCODE_SIZE) and not (flags[0] & T.ERROR_BITS)


# ------------------------------------------------------------------------------------------------------------- seams
def _kinds():
    return [dict(typ=0, eip155=False), dict(typ=0), dict(typ=1, al=access_list([(b"\x09" * 20, [])]), gas_price=7), dict(typ=2)]


def _lengths(tx, chain_id):
    """(raw bytes, signing preimage bytes, raw list payload, signing list payload)"""
    st, pre, *_ = S.tx_signing_parts(tx, chain_id)
    assert st == S.OK
    start = 1 if tx[0] < 0x80 else 0
    return len(tx), len(pre), len(tx) - S.rlp_item(tx, start, len(tx))[1], len(pre) - S.rlp_item(pre, start, len(pre))[1]


def _hitting(kw, chain_id, which, targets, top):
    """(calldata length, value) pairs at which quantity `which` of _lengths is each of `targets`: it grows with the calldata (bisect), by two
    where the calldata's own header grows -- a value one byte longer then shifts the lengths onto the target"""
    hits = []
    for t in targets:
        for value in (1, 0x100, 0x10000):
            size = lambda n: _lengths(raw_tx(chain_id=chain_id, data=b"\xd5" * n, value=value, **kw), chain_id)[which]  # noqa: E731
            lo, hi = 0, top
            while lo < hi:
                mid = (lo + hi) // 2
                if size(mid) < t:
                    lo = mid + 1
                else:
                    hi = mid
            if size(lo) == t:
                hits.append((lo, value))
                break
    assert len(hits) == len(targets), (kw, chain_id, which, hits)
    return hits


def test_block_seams_of_both_sponges(P, oracle):
    """raw length and signing-preimage length each at 135 .. 137 and 271 .. 273 bytes for every kind of transaction and chain ids whose
    EIP-155 suffix is 3, 3, 4 and 11 bytes (a 9-byte v)"""
    seams = (135, 136, 137, 271, 272, 273)
    for chain_id in (1, 127, 128, M64):
        txs = []
        for kw in _kinds():
            for which in (0, 1):
                txs += [raw_tx(chain_id=chain_id, data=_data(n), value=value, **kw) for n, value in _hitting(kw, chain_id, which, seams, 300)]
        assert len(txs) == 48 and {_lengths(t, chain_id)[0] for t in txs} >= set(seams) and {_lengths(t, chain_id)[1] for t in txs} >= set(seams)
        flags = check_call(P, oracle, txs, chain_id=chain_id, recover=False)
        assert not (flags & T.ERROR_BITS).any()


def test_list_header_seams(P, oracle):
    """list payloads of 55 / 56, 255 / 256, 65 535 / 65 536 bytes for the raw list and, separately, for the signing list (between the
    two, the raw list already has the longer header while the signing list still has the shorter one); calldata of 0 bytes, one byte below and one
    from 0x80, 55 / 56 bytes"""
    txs = []
    for kw in _kinds():
        # (the raw list holds v, r and s: it stays below 56 bytes only with a short r and s, and a typed list only with an empty access list)
        small = dict(kw, r=1, s=2, gas_price=7, **({"al": b"\xc0"} if kw["typ"] else {}))
        for which in (2, 3):
            txs += [raw_tx(data=_data(n), value=value, **small) for n, value in _hitting(small, 1, which, (55, 56), 100)]
            txs += [raw_tx(data=_data(n), value=value, **kw) for n, value in _hitting(kw, 1, which, (255, 256, 65535, 65536), 66000)]
        txs += [raw_tx(data=d, **kw) for d in (b"", b"\x00", b"\x7f", b"\x80", b"\xff", _data(55), _data(56))]
    seams = {55, 56, 255, 256, 65535, 65536}
    assert {_lengths(t, 1)[2] for t in txs} >= seams and {_lengths(t, 1)[3] for t in txs} >= seams
    headers = {(_lengths(t, 1)[0] - _lengths(t, 1)[2], _lengths(t, 1)[1] - _lengths(t, 1)[3]) for t in txs}
    assert any(a != b for a, b in headers)  # the two lists under headers of different sizes
    flags = check_call(P, oracle, txs, recover=False)
    assert not (flags & T.ERROR_BITS).any()


# ------------------------------------------------------------------------------------------------------- hostile bytes
def hostile_corpus(tx):
    """every truncation, every single-byte replacement by each of ten values, an appended byte"""
    out = [tx[:k] for k in range(len(tx))]
    for k in range(len(tx)):
        out += [tx[:k] + bytes([b]) + tx[k + 1:] for b in (0x00, 0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8, 0xFF) if b != tx[k]]
    return out + [tx + b"\x00"]


def hostile_subject(oracle, typ):
    al = [(b"\x44" * 20, [b"\x05" * 32]), (b"\x45" * 20, [])]
    return S.make_tx(oracle, D, typ, 1, data=b"\x00\x9a\x01", access_list=al if typ else (), gas=60000)


def _huge_lengths(tx):
    """a length field of 2^64 - 1 in place of the list's header, of the first item and of the last item's"""
    start = 1 if tx[0] < 0x80 else 0
    top = S.rlp_item(tx, start, len(tx))
    ff = b"\xff" * 8
    return [tx[:start] + b"\xff" + ff + tx[top[1]:], tx[:top[1]] + b"\xbf" + ff + tx[top[1] + 1:], tx[:len(tx) - 33] + b"\xbf" + ff + tx[len(tx) - 32:],
            tx[:start] + b"\xfb" + ff[:4] + tx[top[1]:]]


@pytest.mark.parametrize("typ", (0, 1, 2))
def test_hostile_bytes(P, oracle, typ):
    """one call over the whole corpus: flags and sig_status equal the definition's and what phant_tx_senders answers for the same blob"""
    tx = hostile_subject(oracle, typ)
    corpus = hostile_corpus(tx) + _huge_lengths(tx)
    if suite.EMULATED and not suite.FULL:
        corpus = corpus[::9] + _huge_lengths(tx)
    flags = check_call(P, oracle, corpus, base_fee=3, gas_limit=10**7)
    ad, st = P.signer.senders(corpus, 1)
    rc, got, _ = Raw(P, corpus).call(_ctx(P), want=("sender", "sig_status", "flags"))
    assert rc == OK and got["sender"] == ad.tobytes() and got["sig_status"] == st.tobytes()
    assert ((flags & T.UNDECODABLE) != 0).tolist() == (st == S.BAD_TX).tolist() and ((flags & T.BAD_V) != 0).tolist() == (st == S.BAD_V).tolist()
    if not suite.EMULATED or suite.FULL:
        assert {S.OK, S.BAD_TX, S.BAD_V} <= set(st.tolist()) and set(st.tolist()) & {S.BAD_RANGE, S.HIGH_S, S.NOT_ON_CURVE}


# -------------------------------------------------------------------------------------------------------- access lists
def test_access_lists(P, oracle):
    A, K = b"\x0a" * 20, b"\x0b" * 32
    tup = lambda addr, keys, extra=b"": S.rlp_list([S.rlp_bytes(addr), S.rlp_list([S.rlp_bytes(k) for k in keys])] + ([extra] if extra else []))  # noqa: E731
    lists = [b"\xc0", S.rlp_list([tup(A, [])]), S.rlp_list([tup(A, []), tup(A, [K]), tup(A, [K, K])]), S.rlp_list([tup(A, [K] * 40)] * 3),
             S.rlp_list([tup(A[:19], [K])]), S.rlp_list([tup(A, [K[:31]])]), S.rlp_list([tup(A, [K], b"\x80")]), S.rlp_list([S.rlp_list([S.rlp_bytes(A)])]),
             S.rlp_list([S.rlp_bytes(A)]), S.rlp_bytes(b"\x01" * 3), S.rlp_list([tup(A, [K]), b"\x01"])]
    txs = [raw_tx(typ, al=al, data=b"\x00\x01", nonce=i) for typ in (1, 2) for i, al in enumerate(lists)]
    flags = check_call(P, oracle, txs, recover=False)
    assert ((flags & T.UNDECODABLE) != 0).tolist() == ([False] * 4 + [True] * 7) * 2
    r = P.types.transaction.block_transactions(txs, 1, recover=False)
    assert r.al_addresses.tolist()[:4] == [0, 1, 3, 3] and r.al_keys.tolist()[:4] == [0, 0, 3, 120]
    assert r.intrinsic_gas.tolist()[:4] == [21020 + 2400 * a + 1900 * k for a, k in ((0, 0), (1, 0), (3, 3), (3, 120))]
    assert bytes(r.access_list(2)) == lists[2][S.rlp_item(lists[2], 0, len(lists[2]))[1]:] and bytes(r.data(2)) == b"\x00\x01" and r.errors(4) == ["Undecodable"]


# ------------------------------------------------------------------------------------------------------ rule boundaries
def test_rule_boundaries(P, oracle):
    base, I = 1000, T.intrinsic_gas
    d = _data(100)
    txs, want = [], []

    def case(tx, bits):
        txs.append(tx)
        want.append(bits)

    for typ in (0, 1, 2):
        for fee, bits in ((base - 1, T.FEE_BELOW_BASE), (base, 0), (base + 1, 0)):
            case(raw_tx(typ, gas_price=fee, max_priority=1), bits)
    case(raw_tx(2, gas_price=5000, max_priority=5000), 0)
    case(raw_tx(2, gas_price=5000, max_priority=5001), T.PRIORITY_ABOVE_MAX)
    case(raw_tx(2, gas_price=999, max_priority=1000), T.PRIORITY_ABOVE_MAX | T.FEE_BELOW_BASE)
    case(raw_tx(1, gas_price=999, max_priority=1000), T.FEE_BELOW_BASE)  # (no priority rule for type 1)
    for typ in (0, 2):
        for to in (b"\x11" * 20, b""):
            need = I(d, not to, 0, 0)
            case(raw_tx(typ, to=to, data=d, gas=need - 1), T.INTRINSIC_GAS | (0 if to else T.IS_CREATE))
            case(raw_tx(typ, to=to, data=d, gas=need), 0 if to else T.IS_CREATE)
    assert I(d, True, 0, 0) == I(d, False, 0, 0) + 32000 + 2 * 4
    case(raw_tx(0, to=b"", data=_data(49152), gas=10**7), T.IS_CREATE)
    case(raw_tx(0, to=b"", data=_data(49153), gas=10**7), T.IS_CREATE | T.INITCODE_SIZE)
    case(raw_tx(2, to=b"\x11" * 20, data=_data(49153), gas=10**7), 0)
    case(raw_tx(1, nonce=M64 - 1), 0)
    case(raw_tx(1, nonce=M64), T.NONCE_MAX)
    case(raw_tx(0, value=M256, gas_price=base, gas=21000), T.COST_OVERFLOW)
    case(raw_tx(2, value=0, gas_price=M256, max_priority=M256, gas=21000), T.COST_OVERFLOW)
    case(raw_tx(2, value=M256 - 21000 * base, gas_price=base, gas=21000), 0)       # the upfront cost is exactly 2^256 - 1
    case(raw_tx(2, value=M256 - 21000 * base + 1, gas_price=base, gas=21000), T.COST_OVERFLOW)
    case(raw_tx(0, value=M256 % M64, gas_price=M256 // M64, gas=M64), T.GAS_ABOVE_BLOCK)  # exactly 2^256 - 1 again
    case(raw_tx(0, value=M256 % M64 + 1, gas_price=M256 // M64, gas=M64), T.GAS_ABOVE_BLOCK | T.COST_OVERFLOW)
    case(raw_tx(0, gas=30_000_000), 0)
    case(raw_tx(0, gas=30_000_001), T.GAS_ABOVE_BLOCK)
    case(raw_tx(1, chain_id=2), T.CHAIN_ID)
    case(raw_tx(2, chain_id=0), T.CHAIN_ID)
    case(raw_tx(0, chain_id=2), T.BAD_V)  # (a legacy transaction of another chain: its v matches nothing)
    case(raw_tx(2, chain_id=3, gas_price=5, max_priority=9, gas=100, nonce=M64), T.CHAIN_ID | T.PRIORITY_ABOVE_MAX | T.FEE_BELOW_BASE | T.INTRINSIC_GAS | T.NONCE_MAX)
    first = next(i for i, b in enumerate(want) if b & T.ERROR_BITS)
    flags = check_call(P, oracle, txs, base_fee=base, gas_limit=30_000_000, recover=False)
    assert [hex(f) for f in flags] == [hex(b) for b in want]
    r = P.types.transaction.block_transactions(txs, 1, base_fee=base, block_gas_limit=30_000_000, recover=False)
    assert r.first_bad == first == 0 and r.errors(len(txs) - 1) == ["ChainId", "PriorityAboveMax", "FeeBelowBase", "IntrinsicGas", "NonceMax"]
    assert check_call(P, oracle, txs[1:3], base_fee=base, recover=False).tolist() == [0, 0]  # first_bad = n
    # base_fee NULL: the two fee rules are skipped, no effective gas price; no gas limit: that rule is skipped
    flags = check_call(P, oracle, txs, recover=False)
    assert not (flags & (T.FEE_BELOW_BASE | T.PRIORITY_ABOVE_MAX | T.GAS_ABOVE_BLOCK)).any()
    assert bytes(r.effective_gas_price[9]) == (base + 4000).to_bytes(32, "big")  # min(5000, 5000 - 1000) + 1000


# -------------------------------------------------------------------------------------------------------------- senders
def test_fixture_and_mainnet_senders(P, oracle):
    doc = S.load_vectors()
    vec = doc["mainnet"] + doc["fixtures"]
    if suite.EMULATED and not suite.FULL:
        vec = doc["mainnet"] + doc["fixtures"][::13]
    txs = [t["tx"] for t in vec]
    r = P.types.transaction.block_transactions(txs, 1)
    assert [bytes(a).hex() for a in r.sender] == [t["sender"] for t in vec] and not r.sig_status.any()
    assert not (r.flags & (T.UNDECODABLE | T.BAD_V | T.SIGNATURE)).any()
    assert (r.tx_hash == P.types.transaction.hashes(txs)).all()
    check_call(P, oracle, txs, forms=(True,))


def test_genuine_signatures_and_their_high_s_twins(P, oracle):
    """256 signatures of tests/secp_ref.sign as transactions of every type, each with its high-s twin (the same key, refused: HIGH_S)"""
    n = suite.scale(256, 6)
    me = oracle.keccak256(S.pubkey_bytes(S.mul(D, S.G)))[12:]
    txs = []
    for i in range(n):
        kw = dict(nonce=i, data=_data(i), eip155=i % 2 == 0, gas=10**5)
        txs += [S.make_tx(oracle, D, i % 3, 1, **kw), S.make_tx(oracle, D, i % 3, 1, high_s=True, **kw)]
    rc, got, fb = Raw(P, txs).call(_ctx(P), want=("sender", "sig_status", "flags"))
    assert rc == OK and fb == 1
    assert got["sender"] == (me + bytes(20)) * n and got["sig_status"] == bytes([S.OK, S.HIGH_S]) * n
    assert (np.frombuffer(got["flags"], np.uint32) & T.ERROR_BITS).tolist() == [0, T.SIGNATURE] * n
    check_call(P, oracle, txs[:suite.scale(40, 4)], forms=(True,))


# ---------------------------------------------------------------------------------------------------- refused arguments
def test_refused_arguments(P, oracle, pool):
    """each returns PHANT_E_INVALID_ARG (a 4 GiB transaction: PHANT_E_UNSUPPORTED) and touches nothing"""
    ctx = _ctx(P)
    txs = pool[:4]
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantTxsIn), C.sizeof(L.PhantTxsOut))
    good = P.types.transaction.pack(txs)[1]

    def refused(raw, code=E_INVALID_ARG, **kw):
        rc, got, fb = raw.call(ctx, **kw)
        assert rc == code, (rc, kw)
        assert fb == 0xEEEEEEEE and all(set(v) <= {0xEE} for v in got.values()), kw

    for dev in (False, True):
        raw = Raw(P, txs, dev=dev)
        refused(raw, sizes=(sizes[0] - 8, sizes[1]))
        refused(raw, sizes=(sizes[0], sizes[1] + 8))
        refused(raw, n=0, sizes=(sizes[0] + 8, sizes[1]))
        refused(raw, null_in=("txs",))
        refused(raw, null_in=("tx_off",))
        refused(raw, flags=4)
        refused(raw, flags=0x80000000)
        refused(raw, recover=False, want=("sender", "flags"))
        refused(raw, recover=False, want=("sig_status",))
        back = good.copy()
        back[2] = back[1] - 1
        refused(Raw(P, txs, dev=dev, off=back))
        shifted = good.copy()
        shifted[0] = 1
        refused(Raw(P, txs, dev=dev, off=shifted))
        huge = good.copy()
        huge[-1] = good[-2] + (1 << 32)
        if not dev:  # (the device form compares tx_off[n] with tx_bytes, which would have to be 4 GiB of device memory)
            refused(Raw(P, txs, off=huge), code=E_UNSUPPORTED)
    dev = Raw(P, txs, dev=True)
    dev.tx_bytes += 1
    refused(dev)  # tx_off[n] is not tx_bytes
    dev.tx_bytes -= 1
    for k, by in (("nonce", 4), ("data_off", 2), ("intrinsic_gas", 1), ("flags", 2), ("al_keys", 1), ("data_len", 3)):
        refused(dev, skew={k: by})
    rc, got, fb = dev.call(ctx, skew={"tx_hash": 1, "sig": 3, "to": 1})  # byte arrays need no alignment
    assert rc == OK and fb == 4
    rc, got, fb = Raw(P, txs).call(ctx, n=0)
    assert rc == OK and fb == 0


# ------------------------------------------------------------------------------------------------------------ python
def test_the_python_result(P, oracle, pool):
    X = P.types.transaction
    r = X.block_transactions(pool, 1, base_fee=7, block_gas_limit=30_000_000)
    exp, first_bad = T.expected(oracle, pool, 1, 7, 30_000_000)
    assert r.first_bad == first_bad == 5 and r.n == len(pool)
    for name, _, _ in T.OUTPUTS:
        assert getattr(r, name).tobytes() == exp[name], name
    assert bytes(r.data(0)) == b"xyz" and bytes(r.data(3)) == _data(700) and len(r.access_list(3)) == int(r.al_len[3]) > 0
    assert r.errors(0) == [] and r.errors(5) == ["Undecodable"] and r.errors(8) == ["Signature"] and X.FLAG_NAMES[11] == "IsCreate"
    assert (int(r.flags[4]) & T.IS_CREATE) and not int(r.flags[4]) & X.ERROR_BITS
    quiet = X.block_transactions(pool, 1, recover=False)
    assert not hasattr(quiet, "sender") and (quiet.tx_hash == r.tx_hash).all() and (quiet.sig_hash == r.sig_hash).all()
    empty = X.block_transactions([], 1)
    assert empty.n == 0 and empty.first_bad == 0
