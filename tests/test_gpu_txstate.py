"""A block's transactions against the pre-state on the device (phant_block_txs_prestate, phant_block_txs_prestate_dev,
phant_amd.types.transaction.against_prestate) against tests/txstate_ref.py, which defines every output.  Every comparison is exact, in
the host form and in the device form.  tests/test_emu_txstate.py runs the same bodies over the kernel sources compiled for the host, at
the sizes tests/suite.py gives it."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import suite
from tests import txstate_ref as R

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1
ALL = tuple(name for name, _, _, _ in R.OUTPUTS)
M64, M256 = R.M64, R.M256
CODE_HASH = bytes(range(1, 33))
DESIGNATOR = b"\xef\x01\x00" + b"\x55" * 20


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def addr(k):
    """address number k: bytes nobody chose"""
    return hashlib.sha256(b"txstate" + int(k).to_bytes(8, "big")).digest()[:20]


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_txstate_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, dev, txs, accounts, codes=(), auth_first=None, auths=(), probes=()):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        self.counts = {"n": len(txs), "n_auth": len(auths), "n_accounts": len(accounts), "n_codes": len(codes), "n_probe": len(probes)}
        self.code_bytes = sum(len(c) for c in codes)
        self.arrays = {k: None if a is None else self._up(a) for k, a in R.inputs(txs, accounts, codes, auth_first, auths, probes).items()}

    def _up(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size == 0:
            a = np.zeros(8, np.uint8)  # (a pointer that is not NULL, to nothing the call may read)
        return self.torch.from_numpy(a.copy()).cuda() if self.dev else a.copy()

    def _ptr(self, x):
        return None if x is None else x.data_ptr() if self.dev else x.ctypes.data

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, fork, want=None, guard=64, null=(), counts=None, sizes=None, reserved=0, skew=None, code_bytes=None):
        """-> (rc, {output: bytes, (output, "guards"): bool}, first_bad, n_undetermined); every buffer has `guard` bytes of 0xEE in front of
        and behind its rows.  null: inputs passed as NULL; counts: counts other than the arrays'; skew: {array: bytes its pointer moves up}"""
        L = self.L
        want = ALL if want is None else want
        cnt = dict(self.counts, **(counts or {}))
        ptr = lambda k: None if k in null or self.arrays[k] is None else self._ptr(self.arrays[k]) + (skew or {}).get(k, 0)  # noqa: E731
        arg = L.PhantTxstateIn(C.sizeof(L.PhantTxstateIn), fork, cnt["n"], cnt["n_auth"], cnt["n_accounts"], cnt["n_codes"], cnt["n_probe"], reserved,
                               *[ptr(k) for k in L.TXSTATE_INPUTS], self.code_bytes if code_bytes is None else code_bytes, ptr("probe"))
        size = {name: np.dtype(dt).itemsize * k * cnt[rows] for name, dt, k, rows in R.OUTPUTS if name in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantTxstateOut(C.sizeof(L.PhantTxstateOut), 0xEEEEEEEE, 0xEEEEEEEE, 0,
                                *[self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None for k in ALL])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_txs_prestate_dev if self.dev else ctx._lib.phant_block_txs_prestate
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        return rc, got, int(out.first_bad), int(out.n_undetermined)


def _first_difference(name, a, b):
    width = {n: np.dtype(dt).itemsize * k for n, dt, k, _ in R.OUTPUTS}[name]
    for i in range(0, max(len(a), len(b)), width):
        if a[i:i + width] != b[i:i + width]:
            return i // width, a[i:i + width].hex(), b[i:i + width].hex()
    return None


def check(P, fork, txs, accounts, codes=(), auth_first=None, auths=(), probes=(), forms=(False, True), want=None):
    """every answer of the call against the definition, in both forms -> the expected state_flags"""
    exp, first_bad, n_und = R.expected(fork, txs, accounts, codes, auth_first, auths, probes)
    ctx = _ctx(P)
    for dev in forms:
        rc, got, fb, nu = Raw(P, dev, txs, accounts, codes, auth_first, auths, probes).call(ctx, fork, want)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert (fb, nu) == (first_bad, n_und), (dev, fb, first_bad, nu, n_und)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(k, got[k], exp[k]))
    return np.frombuffer(exp["state_flags"], np.uint32)


# ------------------------------------------------------------------------------------------------------ blocks by arrangement
def make_accounts(na, rng):
    """na rows: mostly funded accounts, every ninth proven absent"""
    return [R.account(addr(j), nonce=int(rng.integers(0, 1000)), balance=int(rng.integers(1, 1 << 62)) << int(rng.integers(0, 190)),
                      status=R.ABSENT if j % 9 == 8 else R.PRESENT) for j in range(na)]


def make_block(n, accounts, arrangement, rng):
    """n transactions whose senders are arranged as asked; nonces right except every seventh, costs of up to 250 bits, a row in 29
    skipped (none in the "straddle" and "unbroken" arrangements, which count positions)"""
    na = len(accounts)
    skipped = [i % 29 == 17 and arrangement not in ("straddle", "unbroken") for i in range(n)]
    if arrangement == "distinct":
        who = [i % na for i in range(n)]
    elif arrangement in ("one", "unbroken"):  # "unbroken": the one sender's sequence is all n rows, the first n places of the sorted order
        who = [na // 2] * n
    elif arrangement == "interleaved":  # one sender with 257 rows, one with 65, the others between them: only a stable order ranks them
        quota = {0: 257, na - 1: 65}
        who = []
        for i in range(n):
            pick = 0 if i % 3 == 1 else na - 1 if i % 7 == 2 else None
            if pick is not None and quota[pick] > 0:
                quota[pick] -= not skipped[i]
            elif na > 2:
                pick = 1 + i % (na - 2)
            who.append(pick or 0)
    else:  # "straddle": in the sorted order a sequence of two begins in lane 63 / 255 and ends in the next wave's / tile's first lane
        who = [min(i if i < 64 else i - 1 if i < 256 else i - 2, na - 1) for i in range(n)]
        who = [who[k] for k in rng.permutation(n)]
    sent, txs = {}, []
    for i, j in enumerate(who):
        nonce = accounts[j]["nonce"] + sent.get(j, 0) + (0 if i % 7 != 3 else int(rng.integers(-1, 2)))
        sent[j] = sent.get(j, 0) + (not skipped[i])
        txs.append(R.tx(accounts[j]["address"], max(nonce, 0), int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 188)),
                        accounts[int(rng.integers(0, na))]["address"] if i % 11 != 5 else addr(10**6 + i),
                        flags=R.TX_IS_CREATE if i % 13 == 6 else 0, sig_status=1 if skipped[i] else 0))
    return txs


def test_sizes_and_sender_arrangements(P):
    """every block size around a wave, a tile of the scan (256: also the last block the small path takes, 257 the first of the general
    one) and a tile of the sort (2 048), against every table size, the senders arranged four ways"""
    rng = np.random.default_rng(11)
    sizes = suite.scale((0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025, 2047, 2048, 2049), (0, 1, 65, 256, 257))
    tables = (1, 2, 63, 64, 65, 1000)
    for q, n in enumerate(sizes):
        for w, arrangement in enumerate(("distinct", "one", "interleaved", "straddle")):
            accounts = make_accounts(tables[(q + w) % len(tables)] if n < 257 else 1000, rng)
            txs = make_block(n, accounts, arrangement, rng)
            flags = check(P, R.LONDON, txs, accounts, probes=[addr(3), addr(10**7)])
            assert n < 64 or len(set(flags.tolist())) >= 3
            out, _, _ = R.define(R.LONDON, txs, accounts)  # the sequences the arrangements promise are there
            if arrangement == "interleaved" and n >= 1025:
                assert sorted(out["sends"])[-2:] == [65, 257]
            if arrangement == "straddle" and n >= 257:
                order = sorted(range(n), key=lambda i: (out["sender_row"][i], i))
                assert out["sender_row"][order[63]] == out["sender_row"][order[64]] and out["sender_row"][order[255]] == out["sender_row"][order[256]]
                assert out["sends"][63] == out["sends"][254] == 2
    for na in suite.scale(tables + (2048, 2049), (2, 65, 2048, 2049)):  # every table size against one block; both sides of the small path's
        accounts = make_accounts(na, rng)
        check(P, R.PRAGUE, make_block(129, accounts, "interleaved", rng), accounts)


def test_join(P):
    """addresses that agree in their first and last eight bytes, the zero address, the table's first and last row, duplicate rows (the
    lowest wins), an unproven sender, probes the witness has and lacks"""
    twins = [bytes(range(8)) + bytes([0, 0, m, 0]) + bytes(range(8, 16)) for m in range(4)]
    zero = bytes(20)
    accounts = [R.account(twins[0], nonce=1, balance=10**18), R.account(zero, nonce=2, balance=10**18), R.account(twins[1], nonce=3, balance=10**18),
                R.account(addr(1), nonce=4, status=R.ABSENT), R.account(twins[1], nonce=99), R.account(addr(2), nonce=5, status=20),
                R.account(zero, nonce=98, status=17), R.account(twins[2], nonce=6, balance=10**18)]
    txs = [R.tx(twins[0], 1, 5, twins[2]), R.tx(twins[1], 3, 5, zero), R.tx(twins[2], 6, 5, twins[3]), R.tx(zero, 2, 5, twins[1]), R.tx(twins[3], 0, 5, zero),
           R.tx(addr(2), 5, 5, addr(2)), R.tx(addr(1), 4, 0, twins[0]), R.tx(twins[1], 4, 5, addr(2))]
    flags = check(P, R.LONDON, txs, accounts, probes=[twins[2], twins[3], zero, addr(1), addr(77), twins[1]])
    assert flags.tolist() == [0, 0, R.TO_UNKNOWN, 0, R.SENDER_UNKNOWN, R.SENDER_UNKNOWN | R.TO_UNKNOWN, 0, R.TO_UNKNOWN]
    out, _, _ = R.define(R.LONDON, txs, accounts, probes=[twins[1], zero])
    assert out["probe_row"] == [2, 1] and out["sender_row"][5] == 5 and out["sends"] == [1, 1, 2, 1, 0, 0, 0, 1]
    # a table in which every row is the same address, and no table at all
    check(P, R.LONDON, txs[:3], [R.account(twins[1], nonce=k) for k in range(suite.scale(300, 70))], probes=[twins[1]])
    assert (check(P, R.LONDON, txs, [], probes=[zero]) == R.SENDER_UNKNOWN | R.TO_UNKNOWN).all()


def test_sums(P):
    """costs of ff..ff in every dword position (a carry crosses each boundary), 2^256 - 1 until the sum saturates, a cost-overflow row in
    the middle of a sequence, a balance equal to and one below the need, expected_nonce saturating"""
    a, b = addr(1), addr(2)
    sat = R.NEEDS_INFLOW | R.SPENT_SATURATED
    for k in range(8):
        ones = 0xFFFFFFFF << (32 * k)
        need = 2 * ones + 7  # (k = 7: beyond 2^256 - 1, which no balance reaches)
        accounts = [R.account(a, balance=min(need, M256)), R.account(b, balance=min(need - 1, M256))]
        txs = [R.tx(x, i // 2, c, b) for i, (x, c) in enumerate((x, c) for c in (ones, ones, 7) for x in (a, b))]
        flags = check(P, R.LONDON, txs, accounts)
        assert flags.tolist() == ([0] * 5 + [R.NEEDS_INFLOW] if k < 7 else [0, 0, R.NEEDS_INFLOW, R.NEEDS_INFLOW, sat, sat]), k
    accounts = [R.account(a, nonce=M64 - 2, balance=M256), R.account(b, balance=5)]
    txs = [R.tx(a, min(M64 - 2 + i, M64), M256, b) for i in range(4)] + [R.tx(b, 0, 1, a), R.tx(b, 1, 1 << 256, a), R.tx(b, 2, 3, a), R.tx(b, 3, 3, a)]
    flags = check(P, R.LONDON, txs, accounts)
    assert flags.tolist() == [0, R.NEEDS_INFLOW, sat, sat, 0, R.NEEDS_INFLOW, sat, sat]
    out, _, _ = R.define(R.LONDON, txs, accounts)
    assert out["expected_nonce"][:4] == [M64 - 2, M64 - 1, M64, M64] and out["spent_before"][1:4] == [M256] * 3 and out["spent_before"][6] == M256
    # a long sequence of the widest costs: the sum runs far into the ninth limb, through every level of the scan
    n = suite.scale(700, 130)
    check(P, R.LONDON, [R.tx(a, i, M256 - i, b) for i in range(n)], [R.account(a, balance=M256), R.account(b)])
    check(P, R.LONDON, [R.tx(a, 0, M256, b)], [R.account(a, balance=M256), R.account(b)])
    assert check(P, R.LONDON, [R.tx(a, 0, M256, b)], [R.account(a, balance=M256 - 1), R.account(b)]).tolist() == [R.NEEDS_INFLOW | R.BALANCE_SHORT]


def test_rules(P):
    """every flag alone at each fork; NOT_EOA against CODE_MISSING against a designator (also of 22 and 24 bytes and with a wrong third
    byte); an authority in an earlier transaction, in the same one, in a skipped one; first_bad with errors at several rows"""
    a, b, c = addr(1), addr(2), addr(3)
    acc = lambda **kw: [R.account(a, **kw), R.account(b, balance=10**18), R.account(c, status=R.ABSENT)]  # noqa: E731
    codes = [b"\x60\x00", DESIGNATOR, DESIGNATOR[:22], DESIGNATOR + b"\x00", b"\xef\x01\x01" + DESIGNATOR[3:], b""]
    for fork in suite.scale((R.LONDON, R.CANCUN, R.PRAGUE), (R.LONDON, R.PRAGUE)):
        prague = fork == R.PRAGUE
        lead = R.tx(b, 0, 0, c)
        one = lambda t, accounts, **kw: int(check(P, fork, [lead, t], accounts, codes, **kw)[1])  # noqa: E731
        assert one(R.tx(a, 0, 0, b), acc()) == 0
        assert one(R.tx(a, 0, 0, b, sig_status=3), acc()) == R.SKIPPED
        assert one(R.tx(a, 0, 0, b, flags=R.TX_BAD_V), acc()) == R.SKIPPED
        assert one(R.tx(addr(9), 0, 0, b), acc()) == R.SENDER_UNKNOWN
        assert one(R.tx(a, 0, 0, addr(9)), acc()) == R.TO_UNKNOWN
        assert one(R.tx(a, 0, 0, addr(9), flags=R.TX_IS_CREATE), acc()) == 0
        assert one(R.tx(a, 4, 0, b), acc(nonce=5)) == R.NONCE_LOW
        assert one(R.tx(a, 6, 0, b), acc(nonce=5)) == R.NONCE_HIGH
        assert one(R.tx(a, 0, 9, b), acc(balance=8)) == R.NEEDS_INFLOW
        assert int(check(P, fork, [R.tx(a, 0, 9, b)], acc(balance=8))[0]) == R.NEEDS_INFLOW | R.BALANCE_SHORT
        assert one(R.tx(a, 0, 0, b), acc(code_hash=CODE_HASH, code_index=0)) == R.NOT_EOA
        assert one(R.tx(a, 0, 0, b), acc(code_hash=CODE_HASH)) == (R.CODE_MISSING if prague else R.NOT_EOA)
        assert one(R.tx(a, 7, 9, b), acc(code_hash=CODE_HASH, code_index=1)) == (R.UNDETERMINED if prague else R.NOT_EOA | R.NONCE_HIGH | R.NEEDS_INFLOW)
        for k in (2, 3, 4, 5):
            assert one(R.tx(a, 0, 0, b), acc(code_hash=CODE_HASH, code_index=k)) == R.NOT_EOA
        assert one(R.tx(a, 0, 0, b), acc(code_index=1)) == 0  # (the empty code hash: no code, whatever the index says)
        # authorities: tuple 0 failed, tuples 1 and 2 are genuine
        txs = [R.tx(b, 0, 0, a), R.tx(a, 3, 0, b), R.tx(b, 1, 0, a), R.tx(a, 1, 0, b), R.tx(c, 0, 0, a), R.tx(c, 9, 0, a)]
        auths = [(b, 4), (a, 0), (c, 0), (addr(9), 0)]
        und = R.UNDETERMINED if prague else R.NONCE_HIGH
        flags = check(P, fork, txs, acc(), codes, auth_first=[0, 1, 2, 2, 2, 4, 4], auths=auths)  # a's tuple rides in a's own first row
        assert flags.tolist() == [0, R.NONCE_HIGH, 0, R.UNDETERMINED if prague else 0, 0, und]
        skipped = [dict(t, sig_status=5) if i == 1 else t for i, t in enumerate(txs)]
        flags = check(P, fork, skipped, acc(), codes, auth_first=[0, 1, 2, 2, 2, 4, 4], auths=auths)
        assert flags.tolist() == [0, R.SKIPPED, 0, R.NONCE_HIGH, 0, und]
        flags = check(P, fork, txs, acc(), codes, auth_first=None, auths=auths)
        assert flags.tolist() == [0, R.NONCE_HIGH, 0, 0, 0, R.NONCE_HIGH]
        flags = check(P, fork, txs, acc(), codes, auth_first=[0, 0, 0, 0, 0, 0, 0], auths=auths)  # tuples that belong to no transaction
        assert flags.tolist() == [0, R.NONCE_HIGH, 0, 0, 0, R.NONCE_HIGH]
    exp, first_bad, _ = R.expected(R.LONDON, [R.tx(b, 0, 0, c)] * 3 + [R.tx(a, 1, 0, b), R.tx(b, 3, 0, c), R.tx(a, 9, 0, b)], acc())
    assert first_bad == 1
    n = suite.scale(400, 100)
    flags = check(P, R.LONDON, [R.tx(b, i if i not in (n - 130 + 64, n - 3) else 0, 0, c) for i in range(n)], acc())
    assert np.flatnonzero(flags & R.ERROR_BITS).tolist() == [n - 130 + 64, n - 3]


def random_block(rng, fork, n, na, tuple_density):
    accounts = make_accounts(na, rng)
    codes = [b"\x60\x00\x60\x00", DESIGNATOR, bytes(23), b"\xef\x01\x00" + bytes(20), b"\xef\x01"]
    for j in range(0, na, 6):
        accounts[j].update(code_hash=CODE_HASH, code_index=R.CODE_NONE if j % 12 else int(rng.integers(0, len(codes))) if j else 1)
    txs = make_block(n, accounts, "distinct" if na > 3 else "one", rng)
    who = rng.permutation(n)
    txs = [dict(t, sender=txs[int(who[i]) if i % 3 else i]["sender"]) for i, t in enumerate(txs)]
    per_tx = [int(rng.integers(1, 4)) if rng.random() < tuple_density else 0 for _ in range(n)]
    auth_first = np.concatenate([[0], np.cumsum(per_tx)]).astype(int).tolist()
    auths = [(accounts[int(rng.integers(0, na))]["address"] if rng.random() < 0.8 else addr(10**5 + k), 0 if rng.random() < 0.7 else 4)
             for k in range(auth_first[-1])]
    probes = [accounts[int(rng.integers(0, na))]["address"] if k % 2 else addr(10**8 + k) for k in range(int(rng.integers(0, 40)))]
    return dict(txs=txs, accounts=accounts, codes=codes, auth_first=auth_first, auths=auths, probes=probes)


def test_random_blocks_at_each_fork(P):
    """seeded blocks with codes, designators, tuples and probes; the tuples are few enough that the definition itself leaves under a
    quarter of the participating rows undetermined (asserted on its answer: skipped rules cannot hide a wrong kernel)"""
    rng = np.random.default_rng(23)
    for fork in (R.LONDON, R.CANCUN, R.PRAGUE):
        for n, na in suite.scale(((40, 30), (300, 120), (1500, 900), (2600, 3000)), ((40, 30), (150, 300))):
            blk = random_block(rng, fork, n, na, tuple_density=0.1 * na / n)
            flags = check(P, fork, **blk)
            part = int((~flags & R.SKIPPED != 0).sum())
            und = int((flags & R.UNDETERMINED != 0).sum())
            assert part > n // 2 and und * 4 < part and (fork < R.PRAGUE) == (und == 0), (fork, n, part, und)
            assert n < 100 or len(set(flags.tolist())) >= 8


def test_subsets_of_the_outputs(P):
    """each output alone, each left out, none: the span the host form fetches ends at every position"""
    rng = np.random.default_rng(5)
    blk = random_block(rng, R.PRAGUE, 70, 40, 0.05)
    exp, first_bad, n_und = R.expected(R.PRAGUE, **blk)
    ctx = _ctx(P)
    for dev in (False, True):
        raw = Raw(P, dev, **blk)
        for want in [()] + [(k,) for k in ALL] + [tuple(x for x in ALL if x != k) for k in ALL]:
            rc, got, fb, nu = raw.call(ctx, R.PRAGUE, want)
            assert rc == OK and (fb, nu) == (first_bad, n_und), (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
    # nothing to do at all
    rc, got, fb, nu = Raw(P, False, [], []).call(ctx, R.LONDON)
    assert (rc, fb, nu) == (OK, 0, 0)


@pytest.mark.parametrize("n, na", [(64, 90000), (170000, 2048)])
def test_a_call_beyond_the_pinned_stage(P, n, na):
    """The smallest shapes that cross the 8 MiB pinned stage, whose arena holds the outputs in front of the inputs.  90 000 pre-state rows
    (97 input bytes and 5 output bytes each): the inputs end beyond the stage and cross the bus array by array, the outputs still come
    back as one span.  170 000 transactions (85 input bytes and 52 output bytes each) against 2 048 rows: both directions go array by
    array.  Row for row against the definition, in both forms."""
    rng = np.random.default_rng(41)
    accounts = make_accounts(na, rng)
    txs = make_block(n, accounts, "distinct", rng)
    probes = [addr(3), addr(10**7), accounts[na // 3]["address"]]
    in_bytes = sum(a.nbytes for a in R.inputs(txs, accounts, probes=probes).values() if a is not None)
    rows = {"n": n, "n_accounts": na, "n_probe": len(probes)}
    out_bytes = sum(np.dtype(dt).itemsize * k * rows[r] for _, dt, k, r in R.OUTPUTS)
    assert in_bytes > 8 << 20  # (the inputs lie behind the outputs: whatever those take, they end beyond the stage)
    if n < na:  # the outputs with the control words, the sort's 512 digit totals and every array's padding in front of and between them
        assert out_bytes + 4 * (8 + 512) + 256 * (len(R.OUTPUTS) + 2) < 8 << 20
    else:
        assert out_bytes > 8 << 20
    flags = check(P, R.LONDON, txs, accounts, probes=probes)
    assert len(set(flags.tolist())) >= 3


@pytest.mark.parametrize("n, tiles", [(65600, 257), (65800, 258)])
def test_one_sequence_across_a_chunk_of_aggregates(P, n, tiles):
    """n rows of ONE sender against 2 048 pre-state rows, its sequence unbroken over every tile.  65 600 rows are 257 tiles: the aggregate
    pass runs a second chunk of 256 tiles, and the rank and the 288-bit sum of the rows in tile 256 are what the first chunk's last lane
    hands on.  65 800 rows are 258: what runs into tile 257 is tile 256's aggregate combined with the CARRY of the first chunk (a pass that
    dropped the carry passes at 257 tiles: its second chunk has nothing to store).  Row for row against the definition, in both forms."""
    rng = np.random.default_rng(n)
    na = 2048
    accounts = make_accounts(na, rng)
    txs = make_block(n, accounts, "unbroken", rng)
    assert (n + 255) // 256 == tiles and accounts[na // 2]["status"] == R.PRESENT
    flags = check(P, R.LONDON, txs, accounts)
    out, _, _ = R.define(R.LONDON, txs, accounts)
    assert out["sends"][na // 2] == n and out["expected_nonce"][n - 1] == accounts[na // 2]["nonce"] + n - 1
    assert len(set(flags.tolist())) >= 3 and int(flags[n - 1]) & R.SPENT_SATURATED


def test_refused_arguments(P):
    """one refusal per rule of the header, in both forms; nothing is written"""
    rng = np.random.default_rng(6)
    blk = random_block(rng, R.PRAGUE, 20, 12, 0.3)
    assert blk["auth_first"][-1] >= 2
    ctx = _ctx(P)

    def refused(dev, b=blk, **kw):
        rc, got, fb, nu = Raw(P, dev, **b).call(ctx, kw.pop("fork", R.PRAGUE), **kw)
        assert rc == E_INVALID_ARG, (dev, kw, rc)
        assert all((np.frombuffer(got[k], np.uint8) == 0xEE).all() for k in ALL), (dev, kw)
        assert ctx._lib.phant_last_error(ctx.handle)

    for dev in (False, True):
        back = list(blk["auth_first"])
        k = next(i for i in range(1, len(back)) if back[i] > back[i - 1])
        back[k - 1], back[k] = back[k], back[k - 1]
        refused(dev, dict(blk, auth_first=back))                                         # auth_first goes backwards
        refused(dev, counts={"n_auth": blk["auth_first"][-1] - 1})                          # ... beyond n_auth
        refused(dev, code_bytes=sum(map(len, blk["codes"])) - 1)                            # code_off beyond code_bytes
        raw = Raw(P, dev, **blk)
        off = np.asarray([0, 4, 3, 50, 73, 75], np.uint64)
        raw.arrays["code_off"] = raw._up(off)
        rc, _, _, _ = raw.call(ctx, R.PRAGUE)
        assert rc == E_INVALID_ARG                                                       # code_off goes backwards
        bad_index = [dict(a) for a in blk["accounts"]]
        bad_index[7]["code_index"] = len(blk["codes"])
        refused(dev, dict(blk, accounts=bad_index))                                       # a code_index that names no code
        refused(dev, fork=3)                                                              # an unknown fork
        refused(dev, reserved=1)
        refused(dev, sizes=(8, 8))                                                        # a wrong struct_size
        for name in ("sender", "sig_status", "tx_flags", "nonce", "upfront_cost", "to", "authority", "auth_status", "addresses", "account_status",
                     "nonces", "balances", "code_hashes", "code_index", "code_off", "codes", "probe"):
            if name == "probe" and not blk["probes"]:
                continue
            refused(dev, null=(name,))                                                    # a NULL input whose count is not zero
        # ... and no refusal when the count is zero, or for auth_first
        rc, _, _, _ = Raw(P, dev, **blk).call(ctx, R.PRAGUE, null=("auth_first",))
        assert rc == OK
        rc, _, _, _ = Raw(P, dev, **dict(blk, probes=[])).call(ctx, R.PRAGUE, null=("probe",))
        assert rc == OK
    refused(True, skew={"nonce": 4})                                                      # device form: a misaligned array
    refused(True, skew={"state_flags": 2})


def test_end_to_end_over_the_fixtures(P, oracle):
    """raw transactions -> block_transactions(fork=FORK_LONDON) -> against_prestate over every fixture case: the counts the fixtures fix"""
    from phant_amd.types import transaction as TX

    state = {}

    def rows_of(raws):
        state["bt"] = bt = TX.block_transactions(raws, 1, fork=TX.FORK_LONDON)
        return [{"sender": bt.sender[i].tobytes(), "nonce": int(bt.nonce[i]), "cost": int.from_bytes(bt.upfront_cost[i].tobytes(), "big"),
                 "to": bt.to[i].tobytes(), "sig_status": int(bt.sig_status[i]), "flags": int(bt.flags[i])} for i in range(bt.n)]

    def against(txs, accounts, codes):
        arrays = R.inputs([], accounts, codes)
        pre = type("Pre", (), {k: arrays[k] for k in ("account_status", "nonces", "balances", "code_hashes", "code_index")})()
        info = {"addresses": arrays["addresses"], "codes": arrays["codes"], "code_off": arrays["code_off"], "n_accounts": len(accounts),
                "n_codes": len(codes), "code_bytes": int(arrays["code_off"][-1])}
        r = TX.against_prestate(state["bt"], pre, info, TX.FORK_LONDON)
        assert all(not r.errors(i) for i in range(r.n)) and r.FLAG_NAMES == R.FLAG_NAMES
        return {k: getattr(r, k).tolist() for k in ("sender_row", "expected_nonce", "state_flags", "sends")}, r.first_bad

    assert R.walk_fixtures(oracle, rows_of, against) == R.FIXTURE_ANSWER
