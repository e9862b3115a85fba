"""Range proofs on the device (phant_mpt_verify_ranges, phant_mpt_verify_ranges_dev, phant_amd.mpt.verify_ranges / prove_range) against
tests/range_ref.py, which defines every output.  Every comparison is exact, in the host form and in the device form, with 0xEE guards
around every buffer.  Tries and proofs come from the oracle (oracle.Trie / oracle.mptize) and, in the end-to-end test, from the
library's own prover.  tests/test_emu_ranges.py runs the same bodies over the kernel sources compiled for the host, at the sizes
tests/suite.py gives it."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import range_ref as R
from tests import suite

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1
UNSET = 0xEEEEEEEE
OUTPUTS = (("status", 1), ("has_more", 1), ("computed_root", 32), ("bad_leaf", 4))  # (name, bytes per range)
ALL = tuple(name for name, _ in OUTPUTS)
INPUTS = ("roots", "origins", "leaf_first", "has_proof", "keys", "vals", "val_off", "nodes", "node_off")


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def _oracle():
    from oracle import oracle as o
    o.build()
    o.lib()
    return o


def h(tag, k, n=32):
    """bytes nobody chose"""
    out = b""
    while len(out) < n:
        out += hashlib.sha256(tag.encode() + int(k).to_bytes(8, "big") + len(out).to_bytes(4, "big")).digest()
    return out[:n]


# ---------------------------------------------------------------------------------------------------- tries
_tries = {}


class T:
    """a trie of the oracle's with its sorted keys and values"""

    def __init__(self, keys, vals):
        order = sorted(range(len(keys)), key=lambda i: keys[i])
        self.keys, self.vals = [keys[i] for i in order], [vals[i] for i in order]
        o = _oracle()
        self.trie = o.Trie(self.keys, self.vals) if keys else None
        self.root = self.trie.root() if keys else R.EMPTY_ROOT
        self._proofs = {}

    def prove(self, key):
        if self.trie is None:
            return []
        if key not in self._proofs:
            self._proofs[key] = self.trie.prove(key)
        return self._proofs[key]

    def lower(self, origin):
        return next((i for i, k in enumerate(self.keys) if k >= origin), len(self.keys))

    def served(self, origin, count=None, has_proof=True):
        """-> ((root, origin, leaves, has_proof), nodes): `count` leaves from the first key >= origin on (None: all of them)"""
        lo = self.lower(origin)
        hi = len(self.keys) if count is None else min(len(self.keys), lo + count)
        leaves = list(zip(self.keys[lo:hi], self.vals[lo:hi]))
        nodes = (self.prove(origin) + (self.prove(leaves[-1][0]) if leaves else [])) if has_proof else []
        return (self.root, origin, leaves, has_proof), nodes


def trie(shape, n, seed=0, vlen=None):
    """the four key shapes: "random" 32-byte keys; "deep": 56 shared leading nibbles; "ends": one byte, 30 zero bytes, one byte;
    "clusters": groups that differ in the last byte only, with 1-byte values (leaves embed in their parents)"""
    tag = (shape, n, seed, vlen)
    if tag not in _tries:
        keys = set()
        for i in range(4 * n + 8):
            x = h(f"{shape} {seed}", i)
            keys.add({"random": x, "deep": h(f"pre {seed}", 0)[:28] + x[:4], "ends": x[:1] + bytes(30) + x[1:2],
                      "clusters": h(f"cl {seed}", x[0] % max(1, n // 5))[:31] + x[1:2]}[shape])
            if len(keys) == n:
                break
        keys = sorted(keys)
        vals = [bytes([1 + h("v", i)[0] % 255]) if shape == "clusters" else h(f"val {seed}", i, vlen or 1 + h("l", i)[0] % 100) for i in range(len(keys))]
        _tries[tag] = T(keys, vals)
    return _tries[tag]


def between(a, b):
    """a key strictly between a and b (or a itself when they are neighbours)"""
    return ((int.from_bytes(a, "big") + int.from_bytes(b, "big")) // 2).to_bytes(32, "big")


def below(k):
    return max(0, int.from_bytes(k, "big") - 1).to_bytes(32, "big")


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
def arrays_of(ranges, nodes):
    n = len(ranges)
    leaves = [kv for _, _, ls, _ in ranges for kv in ls]
    a = {"roots": np.frombuffer(b"".join(r[0] for r in ranges), np.uint8), "origins": np.frombuffer(b"".join(r[1] for r in ranges), np.uint8),
         "leaf_first": np.concatenate([[0], np.cumsum([len(r[2]) for r in ranges])]).astype(np.uint32) if n else np.zeros(1, np.uint32),
         "has_proof": np.array([int(bool(r[3])) for r in ranges], np.uint8), "keys": np.frombuffer(b"".join(k for k, _ in leaves), np.uint8),
         "vals": np.frombuffer(b"".join(v for _, v in leaves), np.uint8),
         "val_off": np.concatenate([[0], np.cumsum([len(v) for _, v in leaves])]).astype(np.uint64) if leaves else np.zeros(1, np.uint64),
         "nodes": np.frombuffer(b"".join(nodes), np.uint8),
         "node_off": np.concatenate([[0], np.cumsum([len(x) for x in nodes])]).astype(np.uint64) if nodes else np.zeros(1, np.uint64)}
    return a, dict(n_ranges=n, n_leaves=len(leaves), n_nodes=len(nodes))


class Raw:
    """phant_ranges_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, dev, ranges, nodes, replace=None):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        arrays, self.counts = arrays_of(ranges, nodes)
        arrays.update(replace or {})
        self.sizes = {"vals_len": int(arrays["vals"].size), "nodes_len": int(arrays["nodes"].size)}
        self.arrays = {k: self._up(a) for k, a in arrays.items()}

    def _up(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size == 0:
            a = np.zeros(8, np.uint8)  # (a pointer that is not NULL, to nothing the call may read)
        return self.torch.from_numpy(a.copy()).cuda() if self.dev else a.copy()

    def _ptr(self, x):
        return x.data_ptr() if self.dev else x.ctypes.data

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, want=None, guard=64, null=(), counts=None, sizes=None, reserved=(0, 0), out_reserved=(0, 0), skew=None, lens=None):
        """-> (rc, {output: bytes, (output, "guards"): bool}, (n_failed, first_failed)); every buffer has `guard` bytes of 0xEE in front of
        and behind its rows.  null: inputs passed as NULL; counts / lens: counts and byte lengths other than the arrays'; skew: {array:
        bytes its pointer moves up}"""
        L = self.L
        want = ALL if want is None else want
        cnt, ln = dict(self.counts, **(counts or {})), dict(self.sizes, **(lens or {}))
        ptr = lambda k: None if k in null else self._ptr(self.arrays[k]) + (skew or {}).get(k, 0)  # noqa: E731
        arg = L.PhantRangesIn(C.sizeof(L.PhantRangesIn), cnt["n_ranges"], cnt["n_leaves"], cnt["n_nodes"], (C.c_uint32 * 2)(*reserved),
                              ln["vals_len"], ln["nodes_len"], *[ptr(k) for k in INPUTS])
        size = {name: w * self.counts["n_ranges"] for name, w in OUTPUTS if name in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantRangesOut(C.sizeof(L.PhantRangesOut), UNSET, UNSET, (C.c_uint32 * 2)(*out_reserved),
                               *[self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None for k in ALL])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_mpt_verify_ranges_dev if self.dev else ctx._lib.phant_mpt_verify_ranges
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        return rc, got, (int(out.n_failed), int(out.first_failed))


def expected(ranges, nodes):
    """the definition's answer in the outputs' own bytes, and the two counts"""
    rows = R.verify_call(ranges, nodes)
    want = {"status": bytes(r[0] for r in rows), "has_more": bytes(r[1] for r in rows), "computed_root": b"".join(r[2] for r in rows),
            "bad_leaf": np.array([r[3] for r in rows], np.uint32).tobytes()}
    bad = [i for i, r in enumerate(rows) if r[0] != R.VALID]
    return want, (len(bad), bad[0] if bad else len(rows)), rows


def check(P, ranges, nodes, forms=(False, True), want=None):
    """both forms against the definition, every output exactly -> the definition's rows"""
    exp, counts, rows = expected(ranges, nodes)
    ctx = _ctx(P)
    for dev in forms:
        rc, got, tot = Raw(P, dev, ranges, nodes).call(ctx, want)
        assert rc == OK, (dev, rc, ctx._lib.phant_last_error(ctx.handle))
        for k in (ALL if want is None else want):
            assert got[k, "guards"], (dev, k)
            if got[k] != exp[k]:
                w = dict(OUTPUTS)[k]
                i = next(i for i in range(len(rows)) if got[k][w * i:w * i + w] != exp[k][w * i:w * i + w])
                raise AssertionError((dev, k, "range", i, got[k][w * i:w * i + w].hex(), exp[k][w * i:w * i + w].hex()))
        assert tot == counts, (dev, tot, counts)
    return rows


def statuses(rows):
    return [r[0] for r in rows]


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("m", [0, 1, 2, 63, 64, 65, 300])
def test_leaves_per_range(P, m):
    """ranges of m leaves cut from the middle of a trie of m + 40 random keys: from a key, from between two keys, to the trie's end"""
    t = trie("random", m + 40, seed=m)
    a, na = t.served(t.keys[7], m)
    b, nb = t.served(between(t.keys[10], t.keys[11]), m)
    c, nc = t.served(t.keys[len(t.keys) - m] if m else bytes([255]) * 32, m)
    rows = check(P, [a, b, c], na + nb + nc)
    # (no leaves where some exist: a mismatch; nothing at or above ff..ff: true)
    assert statuses(rows) == ([R.VALID] * 3 if m else [R.ROOT_MISMATCH, R.ROOT_MISMATCH, R.VALID]) and [r[1] for r in rows] == [int(m > 0), int(m > 0), 0]


def test_one_large_range(P):
    m = suite.scale(5000, 300)
    t = trie("random", m + 100, seed=77, vlen=80)
    r, nodes = t.served(t.keys[50], m)
    rows = check(P, [r], nodes)
    assert rows[0][:2] == (R.VALID, 1) and rows[0][2] == t.root


@pytest.mark.parametrize("n_ranges", [1, 3, 70])
def test_ranges_per_call(P, n_ranges):
    """70 ranges: more than a wave of walkers; every third range fails in a way of its own"""
    t = trie("random", 400, seed=5)
    ranges, nodes = [], []
    for i in range(n_ranges):
        r, nd = t.served(t.keys[5 * i], 1 + i % 6)
        if i % 3 == 2:
            r = (r[0], r[1], r[2][1:] if i % 2 else r[2] + [(bytes([255]) * 32, b"x")], True)
        ranges.append(r)
        nodes += nd
    rows = check(P, ranges, nodes)
    assert statuses(rows).count(R.VALID) == n_ranges - n_ranges // 3


def malformed_nodes():
    """nodes that are canonical RLP and no trie node: a branch with a value, a list of 16 items, an extension with an empty path, a leaf
    whose path ends before nibble 64"""
    ref = b"\xa0" + h("child", 0)
    return [R.rlp_list(ref * 2 + b"\x80" * 14 + b"\x01"), R.rlp_list(ref * 2 + b"\x80" * 14), R.rlp_list(R.rlp_str(b"\x00") + ref),
            R.rlp_list(R.rlp_str(R.hex_prefix((1,) * 60, True)) + R.rlp_str(b"value"))]


def one_of_every_status():
    """-> [(the status the definition gives, range, nodes)]: every status, each range in a trie of its own where it needs its own nodes"""
    t = trie("random", 120, seed=9)
    ok, nodes = t.served(t.keys[20], 30)
    root, origin, leaves, _ = ok
    out = [(R.VALID, ok, nodes)]
    swap = leaves[:4] + [leaves[5], leaves[4]] + leaves[6:]
    out.append((R.EMPTY_VALUE, (root, origin, leaves[:3] + [(leaves[3][0], b"")] + leaves[4:], True), nodes))
    out.append((R.VALUE_TOO_LONG, (root, origin, leaves[:9] + [(leaves[9][0], bytes(561))] + leaves[10:], True), nodes))
    out.append((R.BAD_ORDER, (root, origin, swap, True), nodes))
    out.append((R.BELOW_ORIGIN, (root, t.keys[21], leaves, True), nodes))
    out.append((R.ROOT_MISMATCH, (root, origin, leaves[:7] + leaves[8:], True), nodes))
    lone = trie("random", 90, seed=10)  # nobody else's nodes: one of them is left out
    r, nd = lone.served(lone.keys[30], 12)
    out.append((R.MISSING_NODE, r, [x for x in nd if x != nd[1]]))
    for bad in malformed_nodes():
        out.append((R.BAD_NODE, (R.oracle.keccak256(bad), bytes(32), [(h("k", 1), b"v")], True), [bad]))
    return out


def test_every_status_mixed_in_one_call_and_isolation(P):
    """valid and invalid ranges of every status in one call; every range gives the same answers as when it is called alone"""
    cases = one_of_every_status()
    valid = [trie("random", 60, seed=20 + i).served(h("origin", i), 5 + i) for i in range(4)]
    ranges = [c[1] for c in cases] + [v[0] for v in valid]
    ranges = ranges[1::2] + ranges[0::2]  # (mixed)
    nodes = [x for c in cases for x in c[2]] + [x for v in valid for x in v[1]]
    rows = check(P, ranges, nodes)
    assert sorted(set(statuses(rows))) == sorted({c[0] for c in cases})
    assert statuses(rows).count(R.VALID) == 5
    first = 0
    for r, row in zip(ranges, rows):
        alone = check(P, [r], nodes, forms=(True,))[0]
        assert alone[:3] == row[:3] and (alone[3] == R.NO_LEAF) == (row[3] == R.NO_LEAF) and (row[3] == R.NO_LEAF or row[3] - first == alone[3])
        first += len(r[2])


def test_status_precedence(P):
    """one case per adjacent pair of the order: EMPTY_VALUE < VALUE_TOO_LONG < BAD_ORDER < BELOW_ORIGIN at one leaf, the least leaf
    first, the leaf rules before the walks, MISSING_NODE / BAD_NODE before a mismatch, the origin's walk before the last key's"""
    t = trie("random", 50, seed=31)
    (root, origin, leaves, _), nodes = t.served(t.keys[10], 8)
    k = [x for x, _ in leaves]
    cases = [
        ([(k[1], b"")] + leaves[1:], t.keys[12], R.EMPTY_VALUE, 0),                        # empty and below the origin
        ([(k[0], b"v"), (k[0], bytes(561))] + leaves[2:], origin, R.VALUE_TOO_LONG, 1),    # too long and out of order
        ([(k[1], b"v"), (k[0], b"v")] + leaves[2:], t.keys[12], R.BELOW_ORIGIN, 0),        # leaf 0 below the origin, leaf 1 out of order
        ([(k[0], b"v"), (k[0], b"w"), (k[1], b"")], origin, R.BAD_ORDER, 1),                 # the least bad leaf, whatever comes behind
    ]
    ranges = [(root, o, ls, True) for ls, o, _, _ in cases]
    rows = check(P, ranges, nodes)
    first = np.concatenate([[0], np.cumsum([len(r[2]) for r in ranges])])
    assert [(r[0], r[3] - int(f)) for r, f in zip(rows, first)] == [(c[2], c[3]) for c in cases]
    # a leaf rule in front of a missing node; a missing node in front of a mismatch (a leaf dropped as well)
    gone = check(P, [(root, origin, [(k[0], b"")], True), (root, origin, leaves[:3] + leaves[4:], True)], [])
    assert statuses(gone) == [R.EMPTY_VALUE, R.MISSING_NODE]
    # the origin's walk in front of the last key's: a root branch by hand whose slot 3 is a malformed node and whose slot 9 is in no set
    bad = malformed_nodes()[0]
    refs = {3: R.oracle.keccak256(bad), 9: h("nowhere", 0)}
    top = R.rlp_list(b"".join(b"\xa0" + refs[s] if s in refs else b"\x80" for s in range(16)) + b"\x80")
    lo, hi = b"\x30" + bytes(31), b"\x90" + bytes(31)
    rows = check(P, [(R.oracle.keccak256(top), lo, [(hi, b"v")], True), (R.oracle.keccak256(top), lo, [(lo, b"v")], True),
                     (R.oracle.keccak256(top), hi, [(hi, b"v")], True)], [top, bad])
    assert statuses(rows) == [R.BAD_NODE, R.BAD_NODE, R.MISSING_NODE]


def test_tries_sharing_one_node_set_with_garbage(P):
    """ranges of different tries and several ranges of the same trie over one node set, with unrelated and garbage nodes added"""
    a, b = trie("random", 200, seed=40), trie("deep", 80, seed=41)
    parts = [a.served(a.keys[0], 50), a.served(a.keys[50], 50), a.served(a.keys[100], 100), b.served(bytes(32), 30), b.served(b.keys[30], 50)]
    other = trie("random", 64, seed=42)
    junk = other.prove(other.keys[3]) + [b"", b"\x80", b"\xc0", bytes(40), h("junk", 1, 600), b"\xf9\xff\xff" + bytes(100)] + malformed_nodes()
    nodes = junk[:5] + [x for p in parts for x in p[1]] + junk[5:]
    rows = check(P, [p[0] for p in parts], nodes)
    assert statuses(rows) == [R.VALID] * 5 and [r[1] for r in rows] == [1, 1, 0, 1, 0]


@pytest.mark.parametrize("vlen", [1, 31, 32, 33, 55, 56, 110, 560])
def test_value_lengths(P, vlen):
    t = trie("random", 40, seed=50 + vlen, vlen=vlen)
    if vlen == 1:  # a byte that is its own encoding and one that is not
        t = T(t.keys, [b"\x7f" if i % 2 else b"\x80" for i in range(len(t.keys))])
    r, nodes = t.served(t.keys[3], 30)
    w, _ = t.served(bytes(32), None, has_proof=False)
    rows = check(P, [r, w], nodes)
    assert statuses(rows) == [R.VALID, R.VALID] and rows[1][2] == _oracle().mptize(t.keys, t.vals)


def test_value_of_561_bytes(P):
    t = trie("random", 40, seed=60, vlen=20)
    (root, origin, leaves, _), nodes = t.served(t.keys[3], 10)
    rows = check(P, [(root, origin, leaves[:4] + [(leaves[4][0], bytes(561))] + leaves[5:], True)], nodes)
    assert rows[0] == (R.VALUE_TOO_LONG, 0, R.ZERO, 4)
    # a leaf of the PROOF beyond what the build carries (the origin's walk leaves the path at it): a mismatch, where 560 bytes are fine
    for vlen, want in ((600, R.ROOT_MISMATCH), (560, R.VALID)):
        t = trie("random", 40, seed=61, vlen=vlen)
        above = (int.from_bytes(t.keys[-1], "big") + 1).to_bytes(32, "big")
        r, nodes = t.served(above, 0)
        assert statuses(check(P, [r], nodes)) == [want]


def test_embedded_leaves_and_a_root_extension(P):
    """last-byte clusters with 1-byte values: leaves and small branches embed in their parents; 56 shared nibbles: the root is an extension"""
    c, d = trie("clusters", 60, seed=70), trie("deep", 70, seed=71)
    parts = []
    for t in (c, d):
        parts += [t.served(t.keys[0], 20), t.served(between(t.keys[19], t.keys[20]), 25), t.served(t.keys[45], None), t.served(bytes(32), None, has_proof=False)]
    rows = check(P, [p[0] for p in parts], [x for p in parts for x in p[1]])
    assert statuses(rows) == [R.VALID] * 8
    # a middle leaf of a cluster dropped, a value changed
    (root, origin, leaves, _), nodes = parts[0]
    rows = check(P, [(root, origin, leaves[:5] + leaves[6:], True), (root, origin, leaves[:5] + [(leaves[5][0], b"\x00")] + leaves[6:], True)], nodes)
    assert statuses(rows) == [R.ROOT_MISMATCH] * 2


def test_origins(P):
    """the origin at a key, just below one, between two, zero and beyond the last key; no leaves where some exist; the empty trie"""
    t = trie("random", 90, seed=80)
    k = t.keys
    parts = [t.served(k[30], 10), t.served(below(k[30]), 10), t.served(between(k[29], k[30]), 10), t.served(bytes(32), 10), t.served(bytes([255]) * 32, 10),
             t.served(k[-1], 5), t.served(k[30], 0)]
    empty = T([], [])
    parts += [empty.served(h("o", 3), 0), empty.served(bytes(32), None, has_proof=False)]
    rows = check(P, [p[0] for p in parts], [x for p in parts for x in p[1]])
    assert statuses(rows) == [R.VALID] * 6 + [R.ROOT_MISMATCH] + [R.VALID] * 2
    assert [r[1] for r in rows] == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert rows[4][2] == t.root and rows[7][2] == R.EMPTY_ROOT


def test_whole_tries(P):
    """has_proof = 0 over whole tries against oracle.mptize; a proof given for a whole trie; a trie of one key; two keys sharing 0 and 63 nibbles"""
    o = _oracle()
    two0 = T([b"\x10" + bytes(31), b"\x20" + bytes(31)], [b"a", b"b"])
    two63 = T([bytes(31) + b"\x10", bytes(31) + b"\x11"], [b"a" * 40, b"b"])
    tries = [trie("random", n, seed=90 + n) for n in (1, 2, 17, 200)] + [trie("clusters", 30, seed=95), trie("ends", 40, seed=96), two0, two63]
    parts = [t.served(bytes(32), None, has_proof=False) for t in tries] + [t.served(bytes(32), None) for t in tries]
    rows = check(P, [p[0] for p in parts], [x for p in parts for x in p[1]])
    assert statuses(rows) == [R.VALID] * len(parts) and all(r[1] == 0 for r in rows)
    assert [r[2] for r in rows] == [o.mptize(t.keys, t.vals) for t in tries] * 2
    # without a proof a missing leaf is a mismatch, and nothing of the node set is looked at
    t = tries[3]
    rows = check(P, [(t.root, bytes(32), list(zip(t.keys, t.vals))[1:], False)], [])
    assert statuses(rows) == [R.ROOT_MISMATCH]


def test_one_context_small_large_small(P):
    """one context through a small, a large and the same small call again, in both forms: the arenas grow and are carved anew"""
    s = trie("random", 30, seed=100)
    small = [s.served(s.keys[3], 8), s.served(s.keys[20], None)]
    n = suite.scale(3000, 250)
    big = trie("random", n, seed=101)
    large = [big.served(big.keys[i * (n // 8)], n // 8) for i in range(8)]
    first = check(P, [p[0] for p in small], [x for p in small for x in p[1]])
    rows = check(P, [p[0] for p in large], [x for p in large for x in p[1]])
    assert statuses(rows) == [R.VALID] * 8
    assert check(P, [p[0] for p in small], [x for p in small for x in p[1]]) == first


def test_every_output_as_null(P):
    cases = one_of_every_status()[:7]
    ranges, nodes = [c[1] for c in cases], [x for c in cases for x in c[2]]
    for k in ALL:
        check(P, ranges, nodes, want=tuple(x for x in ALL if x != k))
    check(P, ranges, nodes, want=())


def crowded():
    """-> (ranges, nodes, items): twenty-four proven ranges of three leaves that break no leaf rule (every fifth lacks its middle leaf: a
    mismatch), so that what the walks leave beside their paths outnumbers the leaves by far; items = the length of the call's item list
    by the definition's own walks"""
    t = trie("random", 400, seed=140)
    ranges, nodes = [], []
    for i in range(24):
        (root, origin, leaves, _), nd = t.served(between(t.keys[15 * i], t.keys[15 * i + 1]), 3)
        ranges.append((root, origin, leaves[:1] + leaves[2:] if i % 5 == 4 else leaves, True))
        nodes += nd
    table = R.table_of(nodes)
    items = sum(len(R.walk(r[0], r[1], table, False)) + len(r[2]) + len(R.walk(r[0], r[2][-1][0], table, True)) for r in ranges)
    return ranges, nodes, items


def test_the_item_list_outgrows_its_room(P):
    """PHANT_DIAG_RANGES_ITEMS_PER_RANGE = 0: the call has room for its leaves and 64 items more, the walks of these ranges leave several
    hundred: the first run counts, the call runs once more with the counted room, and every output is what it is with the estimate
    (tests/test_emu_ranges.py asserts that the kernels ran twice)"""
    ctx = _ctx(P)
    ranges, nodes, items = crowded()
    n_leaves = sum(len(r[2]) for r in ranges)
    assert items > n_leaves + 64 + 300 and items < n_leaves + 482 * len(ranges)  # beyond the room without the estimate, within it with
    want = check(P, ranges, nodes)
    assert statuses(want) == [R.ROOT_MISMATCH if i % 5 == 4 else R.VALID for i in range(24)]
    ctx.diag_set("ranges_items_per_range", 0)
    try:
        assert check(P, ranges, nodes) == want
        for k in ALL:  # ... and with an output left out, in both forms
            check(P, ranges, nodes, want=tuple(x for x in ALL if x != k))
    finally:
        ctx.diag_set("ranges_items_per_range", -1)
    assert check(P, ranges, nodes) == want


def test_the_leaf_pass_switched_off(P):
    """PHANT_DIAG_RANGES_NO_LEAF_PASS: every leaf goes through the lane that builds its parent; no answer changes"""
    ctx = _ctx(P)
    cases = one_of_every_status()
    ranges, nodes = [c[1] for c in cases], [x for c in cases for x in c[2]]
    want = check(P, ranges, nodes)
    ctx.diag_set("ranges_no_leaf_pass", 1)
    try:
        assert check(P, ranges, nodes) == want
    finally:
        ctx.diag_set("ranges_no_leaf_pass", 0)


def test_refused_arguments(P):
    """one refusal per rule of the header, in both forms; nothing is written.  (The emulated module runs them before any GPU does: an
    offset that got past the check would be a fault there, not a failed assertion.)"""
    t = trie("random", 50, seed=110)
    parts = [t.served(t.keys[3], 8), t.served(t.keys[20], 10), t.served(t.keys[40], 0)]
    ranges, nodes = [p[0] for p in parts], [x for p in parts for x in p[1]]
    ctx = _ctx(P)
    arrays, counts = arrays_of(ranges, nodes)

    def refused(dev, replace=None, **kw):
        rc, got, tot = Raw(P, dev, ranges, nodes, replace).call(ctx, **kw)
        assert rc == E_INVALID_ARG, (dev, kw, replace and list(replace), rc)
        assert all(set(got[k]) <= {0xEE} for k in ALL) and tot == (UNSET, UNSET), (dev, kw)
        assert ctx._lib.phant_last_error(ctx.handle)

    def bent(name, at, value):
        a = arrays[name].copy()
        a[at] = value
        return {name: a}

    for dev in (False, True):
        probe = Raw(P, dev, ranges, nodes)
        refused(dev, sizes=(8, C.sizeof(probe.L.PhantRangesOut)))                # a wrong struct_size, either struct
        refused(dev, sizes=(C.sizeof(probe.L.PhantRangesIn), 8))
        refused(dev, reserved=(1, 0))
        refused(dev, reserved=(0, 1))
        refused(dev, out_reserved=(0, 1))
        for name in INPUTS:
            refused(dev, null=(name,))                                           # a NULL input whose count is not zero
        for name, last in (("leaf_first", counts["n_ranges"]), ("val_off", counts["n_leaves"]), ("node_off", counts["n_nodes"])):
            refused(dev, bent(name, 0, 1))                                       # does not begin at 0
            refused(dev, bent(name, last, int(arrays[name][last]) + 1))          # does not end at its total
            refused(dev, bent(name, last, int(arrays[name][last]) - 1))
            refused(dev, bent(name, 1, int(arrays[name][2]) + 1))                # goes backwards
        refused(dev, lens={"vals_len": int(arrays["vals"].size) + 1})
        refused(dev, lens={"nodes_len": int(arrays["nodes"].size) - 1})
        # ... and no refusal where the count is zero
        rc, got, tot = Raw(P, dev, [], []).call(ctx, null=INPUTS)
        assert rc == OK and tot == (0, 0)
        whole = [(t.root, bytes(32), list(zip(t.keys, t.vals)), False)]
        rc, got, tot = Raw(P, dev, whole, []).call(ctx, null=("nodes", "node_off") + (() if dev else ("origins",)))
        assert rc == OK and tot == (0, 1) and got["status"] == bytes([R.VALID])
        rc, got, tot = Raw(P, dev, [parts[2][0]], parts[2][1]).call(ctx, null=("keys", "vals", "val_off"))
        assert rc == OK and got["status"] == bytes([R.ROOT_MISMATCH])
    refused(True, skew={"val_off": 4})                                           # device form: a misaligned array
    refused(True, skew={"node_off": 4})
    refused(True, skew={"leaf_first": 2})
    refused(True, skew={"bad_leaf": 2})


def test_end_to_end_with_the_library_s_own_prover(P):
    """mpt.prove_range over a trie walked chunk by chunk until has_more is 0: every chunk valid, the union the key set, every computed root
    the trie's; then one chunk with a leaf removed is rejected"""
    from phant_amd import mpt
    n = suite.scale(20000, 400)
    t = trie("random", n, seed=120, vlen=70)
    kvs = [mpt.KeyVal.init(k, v) for k, v in zip(t.keys, t.vals)]
    chunk = suite.scale(3000, 90)
    origin, seen, chunks = bytes(32), [], []
    while True:
        p = mpt.prove_range(kvs, origin, max_leaves=chunk)
        assert p.root == t.root and p.has_proof
        res = mpt.verify_ranges([p.range()], p.nodes)
        assert res.valid(0) and res.computed_root[0].tobytes() == t.root and res.n_failed == 0 and res.first_failed == 1, (len(seen), int(res.status[0]))
        seen += [k for k, _ in p.leaves]
        chunks.append(p)
        if not res.has_more[0]:
            break
        origin = (int.from_bytes(p.leaves[-1][0], "big") + 1).to_bytes(32, "big")
    assert seen == t.keys and len(chunks) == -(-n // chunk)
    # all chunks in one call over the union of their node sets; then one with a leaf removed
    res = mpt.verify_ranges([p.range() for p in chunks], [x for p in chunks for x in p.nodes])
    assert all(res.valid(i) for i in range(len(chunks))) and list(res.has_more) == [1] * (len(chunks) - 1) + [0]
    p = chunks[len(chunks) // 2]
    res = mpt.verify_ranges([mpt.Range(p.root, p.origin, p.leaves[:7] + p.leaves[8:], True)], p.nodes)
    assert int(res.status[0]) == R.ROOT_MISMATCH and not res.valid(0) and res.computed_root[0].tobytes() == R.ZERO and res.first_failed == 0
    # the serving side's other answers: the whole trie from zero needs no proof; nothing at or above an origin beyond the last key
    small = kvs[:50]
    whole = mpt.prove_range(small, bytes(32))
    assert not whole.has_proof and whole.nodes == [] and mpt.verify_ranges([whole.range()], []).valid(0)
    none = mpt.prove_range(small, bytes([255]) * 32)
    res = mpt.verify_ranges([none.range()], none.nodes)
    assert none.leaves == [] and none.has_proof and res.valid(0) and not res.has_more[0]
    capped = mpt.prove_range(small, small[3].key, limit=small[9].key)
    assert [k for k, _ in capped.leaves] == [kv.key for kv in small[3:10]] and mpt.verify_ranges([capped.range()], capped.nodes).has_more[0] == 1
