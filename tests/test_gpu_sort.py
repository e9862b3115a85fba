"""radix_sort.hip's three shared primitives alone on the device, at inputs of the test's choosing: the exclusive scan
(phant_diag_scan_u32), the stable pair sort (phant_diag_sort_pairs) and the digest order (phant_diag_order_digests), each
against numpy / Python.  Every comparison is exact.  The entry points carve every device buffer at the size launch.h
documents, with a guard behind it that they read back: a kernel that writes past its buffer fails the call.
tests/test_emu_sort.py runs the same bodies over the kernel sources compiled for the host, at the sizes tests/suite.py
gives it."""
import ctypes as C

import numpy as np
import pytest

from tests import suite

pytestmark = pytest.mark.gpu

TILE = 2048            # counters / pairs per workgroup, of the scan and of the sort
LEVEL = TILE * TILE    # counters from which the scan has three levels
BIG = (256 * TILE, 256 * TILE + 1)  # 256 | 257 tiles: radix_rows_kernel's chunk loop
REPAIR = 0x80000000
TIE_CAP = 16


@pytest.fixture(scope="module")
def ctx():
    from phant_amd.context import default_context
    return default_context()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------------ scan
def scan(ctx, x):
    buf = np.ascontiguousarray(x, np.uint32).copy()
    ctx.check(ctx._lib.phant_diag_scan_u32(ctx.handle, _p(buf), buf.size))
    return buf


def scan_ref(x):
    return (np.cumsum(x, dtype=np.uint64) - x).astype(np.uint32)  # (truncated: the device's adds wrap at 2^32)


def scan_inputs(n, rng):
    """(name, counters) -- random below 2^20, all zero, all ones (wraps), one non-zero counter first / last"""
    first, last = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    first[0], last[-1] = 0x9E3779B9, 0x85EBCA6B
    return [("random", rng.integers(0, 1 << 20, n, dtype=np.uint32)), ("zero", np.zeros(n, np.uint32)),
            ("ones", np.full(n, 0xFFFFFFFF, np.uint32)), ("first", first), ("last", last)]


def _scan_case(ctx, n):
    rng = np.random.default_rng(n)
    for name, x in scan_inputs(n, rng):
        got = scan(ctx, x)
        assert np.array_equal(got, scan_ref(x)), (n, name, np.flatnonzero(got != scan_ref(x))[:4])
    # the callers' idiom: n + 1 counters, the last one zero -> it ends up holding the total
    x = rng.integers(0, 1 << 20, n + 1, dtype=np.uint32)
    x[n] = 0
    got = scan(ctx, x)
    assert int(got[n]) == int(x.sum(dtype=np.uint64)) & 0xFFFFFFFF and np.array_equal(got, scan_ref(x)), n


SCAN_ONE_LEVEL = (1, 7, 8, 9, 255, TILE - 1, TILE)
SCAN_TWO_LEVELS = (TILE + 1,) + tuple(3 * TILE + r for r in range(9))  # every tail residue n % 8 beside the uint4 path
SCAN_THREE_LEVELS = (LEVEL - 1, LEVEL) + tuple(LEVEL + r for r in range(1, 9))


def test_scan_one_level(ctx):
    for n in SCAN_ONE_LEVEL:
        _scan_case(ctx, n)


def test_scan_two_levels_every_tail_residue(ctx):
    for n in SCAN_TWO_LEVELS:
        _scan_case(ctx, n)


@pytest.mark.parametrize("n", SCAN_THREE_LEVELS)
def test_scan_three_levels_every_tail_residue(ctx, n):
    """2 048^2 counters and beyond: a third level (LEVEL - 1 and LEVEL are the last sizes with two).  On the device and in the
    full CPU suite only (tests/test_emu_sort.py)."""
    _scan_case(ctx, n)


# ------------------------------------------------------------------------------------------------------------- pair sort
def sort_pairs(ctx, keys, vals, bits):
    n = len(keys)
    k_out, v_out = np.full(n, 0xEEEEEEEEEEEEEEEE, np.uint64), np.full(n, 0xEEEEEEEE, np.uint32)
    ctx.check(ctx._lib.phant_diag_sort_pairs(ctx.handle, _p(keys), _p(vals), n, bits, _p(k_out), _p(v_out)))
    return k_out, v_out


def sort_ref(keys, vals, bits):
    """the stable order by the low `bits` bits rounded up to whole bytes; keys come back whole"""
    rb = (bits + 7) // 8 * 8
    mask = np.uint64((1 << rb) - 1)
    perm = np.argsort(keys & mask, kind="stable")
    return keys[perm], vals[perm]


KEY_SETS = ("uniform", "equal", "two", "descending", "ascending", "zipf") + tuple("byte%d" % k for k in range(8))


def key_set(kind, n, bits, rng):
    """n keys of a kind in their low `bits` bits, random garbage above them"""
    i = np.arange(n, dtype=np.uint64)
    if kind == "uniform":
        base = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    elif kind == "equal":
        base = np.full(n, 0x0123456789ABCDEF, np.uint64)
    elif kind == "two":  # only digits 0 and 255
        base = np.where(i & np.uint64(1), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
    elif kind == "descending":
        base = np.uint64(n - 1) - i
    elif kind == "ascending":
        base = i
    elif kind == "zipf":  # one key holds 90 % of the pairs
        base = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        base[rng.random(n) < 0.9] = np.uint64(0x5A5A5A5A5A5A5A5A)
    else:  # exactly one byte varies, the other seven are fixed and non-zero
        k = int(kind[4:])
        fixed = np.uint64(0x1122334455667788 & ~(0xFF << (8 * k)))
        base = fixed | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * k))
    if bits < 64:
        low = np.uint64((1 << bits) - 1)
        base = (base & low) | (rng.integers(0, 1 << 64, n, dtype=np.uint64) & ~low)
    return np.ascontiguousarray(base, np.uint64)


def _sort_case(ctx, kind, n, bits, rng, vals=None):
    keys = key_set(kind, n, bits, rng)
    vals = np.arange(n, dtype=np.uint32) if vals is None else vals  # (i: stability shows)
    keys0 = keys.copy()
    got_k, got_v = sort_pairs(ctx, keys, vals, bits)
    want_k, want_v = sort_ref(keys, vals, bits)
    assert np.array_equal(keys, keys0)
    assert np.array_equal(got_k, want_k), (kind, n, bits, np.flatnonzero(got_k != want_k)[:4])
    assert np.array_equal(got_v, want_v), (kind, n, bits, np.flatnonzero(got_v != want_v)[:4])


SORT_SIZES = (1, 63, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, 3 * TILE + 1)
SORT_BITS = (1, 8, 9, 16, 24, 32, 33, 64)


def _sizes_and_bits(kind):
    """(n, bits): the complete cross on the device.  The default CPU suite, where a pass costs the same whatever n is: three tiles + 1
    (the histogram's second workgroup holds one tile) with two passes, a tile + 1 and a wave + 1; a varying byte with just the passes
    that reach it."""
    if kind.startswith("byte"):
        fast = [(3 * TILE + 1, 8 * (int(kind[4:]) + 1))]
    else:
        fast = [(65, 16), (TILE + 1, 8), (3 * TILE + 1, 9)]
    return suite.scale([(n, bits) for n in SORT_SIZES for bits in SORT_BITS], fast)


@pytest.mark.parametrize("kind", KEY_SETS)
def test_sort_pairs_sizes_bits_and_key_sets(ctx, kind):
    rng = np.random.default_rng(KEY_SETS.index(kind))
    for n, bits in _sizes_and_bits(kind):
        _sort_case(ctx, kind, n, bits, rng)


def test_sort_pairs_random_values_with_repeats(ctx):
    rng = np.random.default_rng(77)
    n = 3 * TILE + 1
    _sort_case(ctx, "zipf", n, 16, rng, vals=rng.integers(0, 50, n, dtype=np.uint32) * np.uint32(0x01010101))


def test_sort_pairs_bits_zero_returns_the_input(ctx):
    rng = np.random.default_rng(5)
    keys, vals = key_set("uniform", 3000, 64, rng), rng.integers(0, 1 << 32, 3000, dtype=np.uint32)
    got_k, got_v = sort_pairs(ctx, keys, vals, 0)
    assert np.array_equal(got_k, keys) and np.array_equal(got_v, vals)
    e = np.zeros(0, np.uint64)
    ctx.check(ctx._lib.phant_diag_sort_pairs(ctx.handle, None, None, 0, 64, None, None))
    assert sort_pairs(ctx, e, np.zeros(0, np.uint32), 64)[0].size == 0


@pytest.mark.parametrize("n", BIG)
def test_sort_pairs_256_and_257_tiles(ctx, n):
    """radix_rows_kernel walks a digit's row of per-tile counts 256 tiles at a time: 257 tiles is its second chunk.  On the
    device and in the full CPU suite only (tests/test_emu_sort.py)."""
    rng = np.random.default_rng(n)
    for bits in (8, 32, 64):
        for kind in dict.fromkeys(("equal", "uniform", "byte0", "byte%d" % (bits // 8 - 1))):
            _sort_case(ctx, kind, n, bits, rng)


# ---------------------------------------------------------------------------------------------------------- digest order
PREFIX_BITS = (0, 8, 40, 64, 8 | REPAIR, 16 | REPAIR)


def order_digests(ctx, dig, seg, n_seg, prefix_bits):
    n = len(dig)
    order, flag = np.full(n, 0xEEEEEEEE, np.uint32), np.full(1, 0xEEEEEEEE, np.uint32)
    ctx.check(ctx._lib.phant_diag_order_digests(ctx.handle, _p(dig) if n else None, _p(seg), n, n_seg, prefix_bits, _p(order) if n else None,
                                                _p(flag)))
    return order, int(flag[0])


def order_ref_py(dig, seg):
    """THE reference: sorted(range(n), key=lambda i: (seg[i], digest[i]))"""
    rows = [bytes(r) for r in dig]
    return sorted(range(len(rows)), key=lambda i: (int(seg[i]) if seg is not None else 0, rows[i]))


def _words(dig):
    return dig.reshape(-1, 32).view(">u8").astype(np.uint64)  # (n, 4): a digest as four big-endian numbers


def _seg(dig, seg):
    return np.zeros(len(dig), np.uint32) if seg is None else seg


def order_ref(dig, seg):
    """the same order with numpy (test_the_references_and_the_flag_model_alone holds the two against each other)"""
    w = _words(dig)
    return np.lexsort((w[:, 3], w[:, 2], w[:, 1], w[:, 0], _seg(dig, seg))).astype(np.uint32)


def _sorted_bits(prefix_bits):
    k = (prefix_bits & 0x7FFFFFFF) or 32
    return (prefix_bits == 0 or bool(prefix_bits & REPAIR)), 64 if k >= 64 else (k + 7) // 8 * 8


def flag_model_py(dig, seg, prefix_bits):
    """The model in plain Python.  With repair: set iff a run of equal (segment, 32-bit prefix under the sorted bits' mask) is longer
    than TIE_CAP, or a (segment, digest) occurs twice.  Without: iff the stable order by (segment, sorted prefix) is not strictly
    ascending in (segment, digest)."""
    repair, bits = _sorted_bits(prefix_bits)
    rows = [(int(seg[i]) if seg is not None else 0, bytes(dig[i])) for i in range(len(dig))]
    if repair:
        m = min(bits, 32)
        runs = {}
        for s, d in rows:
            key = (s, int.from_bytes(d[:4], "big") >> (32 - m))
            runs[key] = runs.get(key, 0) + 1
        return max(runs.values(), default=0) > TIE_CAP or len(set(rows)) != len(rows)
    order = sorted(range(len(rows)), key=lambda i: (rows[i][0], int.from_bytes(rows[i][1][:8], "big") >> (64 - bits)))
    return any(rows[a] >= rows[b] for a, b in zip(order, order[1:]))


def flag_model(dig, seg, prefix_bits, ref=None):
    """flag_model_py with numpy (`ref`: order_ref(dig, seg), if the caller has it)"""
    n = len(dig)
    if n < 2:
        return False
    repair, bits = _sorted_bits(prefix_bits)
    w, s = _words(dig), _seg(dig, seg)
    cols = (s, w[:, 0], w[:, 1], w[:, 2], w[:, 3])
    if repair:
        o = order_ref(dig, seg) if ref is None else ref
        p = w[:, 0] >> np.uint64(64 - min(bits, 32))
        same = (s[o][1:] == s[o][:-1]) & (p[o][1:] == p[o][:-1])  # position i + 1 continues position i's run
        edges = np.flatnonzero(np.concatenate(([True], ~same, [True])))
        twice = np.ones(n - 1, bool)
        for c in cols:
            twice &= c[o][1:] == c[o][:-1]
        return bool(np.diff(edges).max() > TIE_CAP or twice.any())
    o = np.lexsort((w[:, 0] >> np.uint64(64 - bits), s))
    lt, eq = np.zeros(n - 1, bool), np.ones(n - 1, bool)
    for c in cols:
        a, b = c[o][:-1], c[o][1:]
        lt |= eq & (a < b)
        eq &= a == b
    return not bool(lt.all())


def _digests(rng, n, prefix32=None, lead=None):
    """n random digests; prefix32: their first four bytes as numbers; lead: bytes every one of them starts with"""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if prefix32 is not None:
        d[:, :4] = np.asarray(prefix32, ">u4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)
    if lead is not None:
        d[:, :len(lead)] = np.frombuffer(lead, np.uint8)
    return d


def tie_case(rng, run, where, n=600, in_order=False):
    """n digests with distinct 32-bit prefixes but for `run` of them that share one, which the order puts at the start, across
    positions 255 | 256 (a run leader in one workgroup of tie_fix_kernel, members in the next) or at the end; shuffled.  in_order: the
    run's members come in ascending order, so that the stable passes leave nothing to repair"""
    step = 0x00600000
    others = (np.arange(n - run, dtype=np.uint64) + 1) * step
    shared = {"start": 0, "across": (256 - run // 2) * step + 1, "end": 0xFFFFFFFF}[where]
    d = _digests(rng, n, prefix32=np.concatenate([others, np.full(run, shared, np.uint64)]))
    d = d[rng.permutation(n)]
    if in_order:
        at = np.flatnonzero((d[:, :4] == d[order_ref(d, None)[{"start": 0, "across": 256, "end": n - 1}[where]], :4]).all(1))
        d[at] = d[at][order_ref(d[at], None)]
    return d


def last_byte_flipped(d):
    d = d.copy()
    d[:, 31] ^= 1
    return d


def _segments(rng, n, n_seg, how):
    """segment indices below n_seg with some segments empty, the first and the last never; descending or shuffled"""
    if n_seg == 1:
        return np.zeros(n, np.uint32)
    used = np.unique(np.concatenate([[0, n_seg - 1], rng.integers(0, n_seg, max(2, min(n_seg, n) // 2))]))
    seg = used[rng.integers(0, len(used), n)].astype(np.uint32)
    seg[:2] = (0, n_seg - 1)
    return np.sort(seg)[::-1].copy() if how == "descending" else seg


def tie_cases():
    """(name, digests, seg_of or None, n_seg, the flag the case is built for at prefix_bits 0): shared bytes, runs around TIE_CAP, duplicates"""
    rng = np.random.default_rng(2024)
    out = []
    for k in (16, 17, 200):  # 31 shared bytes: one run, ordered by the last byte alone
        d = _digests(rng, 1, None).repeat(k, 0)
        d[:, 31] = rng.permutation(256)[:k]
        out.append(("31 shared bytes x %d" % k, d, None, 1, int(k > TIE_CAP)))
    for lead in (4, 8, 9):
        for k in (TIE_CAP, 300):
            out.append(("%d shared bytes x %d" % (lead, k), _digests(rng, k, lead=bytes(range(1, lead + 1))), None, 1, int(k > TIE_CAP)))
    for run in (2, 15, 16, 17):
        for where in ("start", "across", "end"):
            out.append(("run of %d at the %s" % (run, where), tie_case(rng, run, where), None, 1, int(run > TIE_CAP)))
    for where in ("start", "across", "end"):  # nothing out of order, and yet a run beyond TIE_CAP: the flag comes from its length alone
        out.append(("run of 17 in order at the %s" % where, tie_case(rng, 17, where, in_order=True), None, 1, 1))
    # 32 digests of one prefix, 16 in each of two segments: two runs of TIE_CAP
    d = _digests(rng, 300, prefix32=np.concatenate([np.full(32, 0x80000000), rng.integers(0, 1 << 31, 268)]))
    seg = np.concatenate([np.repeat([0, 1], 16), rng.integers(0, 2, 268)]).astype(np.uint32)
    p = rng.permutation(300)
    out.append(("a run a segment boundary cuts into 16 + 16", d[p], seg[p], 2, 0))
    out.append(("a run of 16 + 17 in two segments", np.concatenate([d, last_byte_flipped(d[:1])]), np.concatenate([seg, [1]]).astype(np.uint32), 2, 1))
    d = _digests(rng, 100)
    d[60] = d[7]
    seg = (np.arange(100) >= 50).astype(np.uint32)
    out.append(("one digest in two segments", d, seg, 2, 0))
    out.append(("one digest twice in one segment", d, (np.arange(100) >= 70).astype(np.uint32), 2, 1))
    out.append(("one digest twice, no segments", d, None, 1, 1))
    return out


def size_cases():
    """... sizes, segment counts and skewed digits, everything but the largest size"""
    rng = np.random.default_rng(2025)
    out = []
    for n in (0, 1, 2, TILE + 1):
        out.append(("random %d" % n, _digests(rng, n), None, 1, 0))
    for n_seg in (1, 2, 255, 256, 257, 65537):  # segment passes of 8, 8, 8, 8, 16 and 24 bits
        for how in ("descending", "shuffled"):
            n = TILE + 1
            out.append(("%d segments %s" % (n_seg, how), _digests(rng, n), _segments(rng, n, n_seg, how), n_seg, 0))
    d = _digests(rng, 3 * TILE + 1)  # three tiles: the histogram's second workgroup holds one; descending input
    out.append(("three tiles + 1, descending", d[order_ref(d, None)[::-1]], None, 1, 0))
    d = _digests(rng, TILE, lead=b"\x77")  # one digit holds a whole tile in the last pass, 255 digits are empty
    out.append(("a whole tile in one digit", d, None, 1, 0))
    return out


@pytest.fixture(scope="module")
def ties():
    return tie_cases()


@pytest.fixture(scope="module")
def sizes():
    return size_cases()


def _check_order(ctx, name, dig, seg, n_seg, prefix_bits, ref):
    n = len(dig)
    order, flag = order_digests(ctx, dig, seg, n_seg, prefix_bits)
    if flag_model(dig, seg, prefix_bits, ref):
        assert flag != 0, (name, hex(prefix_bits))
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), (name, hex(prefix_bits))  # (the caller throws it away)
    else:
        assert flag == 0, (name, hex(prefix_bits))
        assert np.array_equal(order, ref), (name, hex(prefix_bits), np.flatnonzero(order != ref)[:4])


def test_the_references_and_the_flag_model_alone(ties, sizes):
    """No device: the numpy forms against the plain Python ones on every case and prefix_bits, and the model against what the cases were
    built for -- before either is held against a kernel."""
    seen, cases = set(), ties + sizes
    for name, dig, seg, n_seg, built_for in cases:
        assert seg is None or (len(seg) == len(dig) and int(seg.max(initial=0)) < n_seg), name
        ref = order_ref(dig, seg)
        assert list(ref) == order_ref_py(dig, seg), name
        for pb in PREFIX_BITS:
            m = flag_model(dig, seg, pb, ref)
            assert m == flag_model_py(dig, seg, pb), (name, hex(pb))
            seen.add((pb, m))
        assert flag_model(dig, seg, 0, ref) == bool(built_for), name
    assert seen == {(pb, m) for pb in PREFIX_BITS for m in (False, True)}  # every mode both decides and gives up somewhere
    by_name = {c[0]: c for c in cases}
    _, d, s, _, _ = by_name["a run a segment boundary cuts into 16 + 16"]
    assert not flag_model(d, s, 0) and flag_model(d, None, 0)  # (the segments are what keeps the runs at TIE_CAP)
    _, d, s, _, _ = by_name["run of 17 at the across"]
    o = order_ref(d, None)
    p = d[o][:, :4].copy().view(">u4").ravel()
    assert (p[248:265] == p[248]).all() and p[247] != p[248] and p[265] != p[248]  # positions 248 .. 264: both sides of 255 | 256
    for where in ("start", "across", "end"):
        _, d, _, _, _ = by_name["run of 17 in order at the %s" % where]
        at = np.flatnonzero((d[:, :4] == d[order_ref(d, None)[{"start": 0, "across": 256, "end": -1}[where]], :4]).all(1))
        assert len(at) == 17 and list(order_ref(d[at], None)) == list(range(17))
    # without repair 64 sorted bits decide random digests, 8 do not
    d = _digests(np.random.default_rng(1), 500)
    assert not flag_model(d, None, 64) and flag_model(d, None, 8) and not flag_model(d[:1], None, 8)


def test_order_digests_ties_runs_and_duplicates(ctx, ties):
    """Every case at every prefix_bits.  The default CPU suite: the runs around TIE_CAP at the product's prefix_bits, the rest on eight
    bits with and without the repair."""
    for name, dig, seg, n_seg, _ in ties:
        ref = order_ref(dig, seg)
        for pb in suite.scale(PREFIX_BITS, (0,) if "run" in name else (8 | REPAIR, 8)):
            _check_order(ctx, name, dig, seg, n_seg, pb, ref)


def test_order_digests_sizes_and_segments(ctx, sizes):
    """n = 0, 1, 2, 2 049 and three tiles + 1; 1 .. 65 537 segments, descending and shuffled, some empty; seg_of null.  The default CPU
    suite runs every case at one prefix_bits: the product's for the skewed tiles, one that moves with the case for the rest."""
    for k, (name, dig, seg, n_seg, _) in enumerate(sizes):
        ref = order_ref(dig, seg)
        for pb in suite.scale(PREFIX_BITS, (0 if "tile" in name else PREFIX_BITS[k % len(PREFIX_BITS)],)):
            _check_order(ctx, name, dig, seg, n_seg, pb, ref)


@pytest.mark.parametrize("what", ["random", "one digit holds a pass, descending", "65537 segments"])
def test_order_digests_524289(ctx, what):
    """257 tiles.  On the device and in the full CPU suite only (tests/test_emu_sort.py)."""
    n = BIG[1]
    rng = np.random.default_rng(len(what))
    seg, n_seg, pbs = None, 1, (0,)
    if what == "random":
        dig, pbs = _digests(rng, n), PREFIX_BITS
    elif what == "65537 segments":
        dig, n_seg = _digests(rng, n), 65537
        seg = _segments(rng, n, n_seg, "shuffled")
    else:  # the first byte is the same everywhere: the fourth pass has one digit; 24 random bits tie often, never 17 times
        dig = _digests(rng, n, lead=b"\xA5")
        dig = dig[order_ref(dig, None)[::-1]]
    ref = order_ref(dig, seg)
    for pb in pbs:
        _check_order(ctx, what, dig, seg, n_seg, pb, ref)


# ------------------------------------------------------------------------------------------------------------ the rest
def test_refused_arguments_write_nothing(ctx):
    from phant_amd import _lib as L
    lib, h = ctx._lib, ctx.handle
    c4, k8 = np.full(4, 0xEEEEEEEE, np.uint32), np.full(4, 0xEEEEEEEEEEEEEEEE, np.uint64)
    v4, ko, vo = c4.copy(), k8.copy(), c4.copy()
    assert lib.phant_diag_scan_u32(None, _p(c4), 4) == L.E_INVALID_ARG
    assert lib.phant_diag_scan_u32(h, None, 4) == L.E_INVALID_ARG
    assert lib.phant_diag_scan_u32(h, None, 0) == L.OK
    for args in ((None, _p(k8), _p(v4), 4, 8, _p(ko), _p(vo)), (h, None, _p(v4), 4, 8, _p(ko), _p(vo)), (h, _p(k8), None, 4, 8, _p(ko), _p(vo)),
                 (h, _p(k8), _p(v4), 4, 8, None, _p(vo)), (h, _p(k8), _p(v4), 4, 8, _p(ko), None), (h, _p(k8), _p(v4), 4, 65, _p(ko), _p(vo)),
                 (h, _p(k8), _p(v4), 0, 65, _p(ko), _p(vo))):
        assert lib.phant_diag_sort_pairs(*args) == L.E_INVALID_ARG, args
    assert lib.phant_diag_sort_pairs(h, None, None, 0, 64, None, None) == L.OK
    dig, seg = np.zeros((4, 32), np.uint8), np.array([0, 1, 2, 1], np.uint32)
    order, flag = c4.copy(), c4[:1].copy()
    for args in ((None, _p(dig), _p(seg), 4, 3, 0, _p(order), _p(flag)), (h, None, _p(seg), 4, 3, 0, _p(order), _p(flag)),
                 (h, _p(dig), _p(seg), 4, 3, 0, None, _p(flag)), (h, _p(dig), _p(seg), 4, 3, 0, _p(order), None),
                 (h, _p(dig), _p(seg), 4, 2, 0, _p(order), _p(flag))):  # (the last: a segment index that is not below n_seg)
        assert lib.phant_diag_order_digests(*args) == L.E_INVALID_ARG, args
    assert b"n_seg" in lib.phant_last_error(h)
    for a in (c4, v4, vo, order, flag):
        assert (a == 0xEEEEEEEE).all()
    assert (k8 == ko).all() and (ko == 0xEEEEEEEEEEEEEEEE).all()
    assert lib.phant_diag_order_digests(h, _p(dig), None, 4, 3, 0, _p(order), _p(flag)) == L.OK  # seg_of may be null
    assert flag[0] != 0 and sorted(order) == [0, 1, 2, 3]  # (four equal digests)


def test_one_context_small_large_small(ctx):
    """the staging arena grows and is reused: the guards sit where THIS call's buffers end"""
    import phant_amd
    own = ctx if suite.EMULATED else phant_amd.context.Context()
    try:
        rng = np.random.default_rng(9)
        for n in (5, suite.scale(300_000, 3 * TILE + 5), 3):
            x = rng.integers(0, 1 << 20, n, dtype=np.uint32)
            assert np.array_equal(scan(own, x), scan_ref(x))
            _sort_case(own, "uniform", n, 16, rng)
            dig = _digests(rng, n)
            _check_order(own, "small large small", dig, None, 1, 0, order_ref(dig, None))
    finally:
        if own is not ctx:
            own.close()
