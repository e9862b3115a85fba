"""tests/range_ref.py, the definition the range-proof tests compare the library with, held against answers that owe nothing to it: for a
trie the test built itself (oracle.Trie, proofs from its prover) a range is valid iff its leaves are exactly the trie's keys in
[origin, last], and has_more iff a greater key exists.  No GPU and no library of the project's is involved."""
import numpy as np
import pytest

from tests import range_ref as R


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o
    o.build()
    o.lib()
    return o


SHAPES = ("random", "deep", "ends", "clusters")


def make(rng, shape, n):
    if shape == "random":
        keys = {rng.bytes(32) for _ in range(n)}
    elif shape == "deep":  # 56 shared leading nibbles
        pre = rng.bytes(28)
        keys = {pre + rng.bytes(4) for _ in range(n)}
    elif shape == "ends":  # one byte, 30 zero bytes, one byte
        keys = {rng.bytes(1) + bytes(30) + rng.bytes(1) for _ in range(n)}
    else:  # clusters that differ in the last byte only, with 1-byte values: leaves embed in their parents
        heads = [rng.bytes(31) for _ in range(max(1, n // 6))]
        keys = {heads[int(rng.integers(0, len(heads)))] + rng.bytes(1) for _ in range(n)}
    keys = sorted(keys)
    vals = [bytes([int(rng.integers(1, 256))]) if shape == "clusters" else rng.bytes(int(rng.integers(1, 90))) for _ in keys]
    return keys, vals


def dec(k):
    return max(0, int.from_bytes(k, "big") - 1).to_bytes(32, "big")


def truth(val, origin, leaves):
    """what is true of a claim, from the trie's contents {key: value} alone -> (valid, has_more)"""
    if not leaves:
        return not any(k >= origin for k in val), False
    want = [(k, val[k]) for k in sorted(val) if origin <= k <= leaves[-1][0]]
    return leaves == want, any(k > leaves[-1][0] for k in val)


@pytest.mark.parametrize("shape", SHAPES)
def test_true_and_damaged_ranges_over_tries_of_every_shape(O, shape):
    rng = np.random.default_rng(SHAPES.index(shape) + 11)
    accepted = rejected = 0
    for trial in range(60):
        keys, vals = make(rng, shape, int(rng.integers(1, 120)))
        val = dict(zip(keys, vals))
        t = O.Trie(keys, vals)
        root = t.root()
        assert root == O.mptize(keys, vals) == R.build_root([(R.nibbles(k), "leaf", v) for k, v in zip(keys, vals)])
        for kind in range(5):
            i = int(rng.integers(0, len(keys)))
            j = int(rng.integers(i, len(keys)))
            mid = ((int.from_bytes(keys[i - 1], "big") + int.from_bytes(keys[i], "big")) // 2).to_bytes(32, "big") if i else bytes(32)
            origin = [keys[i], dec(keys[i]), mid, bytes(32), bytes([255]) * 32][kind]
            lo = next((x for x, k in enumerate(keys) if k >= origin), len(keys))
            hi = max(lo, j + 1) if lo < len(keys) else lo
            leaves = [(k, val[k]) for k in keys[lo:hi]]
            nodes = t.prove(origin) + (t.prove(leaves[-1][0]) if leaves else [])
            table = R.table_of(nodes)
            st, more, got, bad = R.verify(root, origin, leaves, True, table)
            ok, has_more = truth(val, origin, leaves)
            assert ok and (st, more, got, bad) == (R.VALID, int(has_more), root, R.NO_LEAF), (shape, trial, kind, st)
            accepted += 1
            damaged = []
            if len(leaves) > 2:
                damaged.append((origin, leaves[:1] + leaves[2:], table))                     # a middle leaf dropped
                damaged.append((origin, [leaves[1], leaves[0]] + leaves[2:], table))         # two leaves swapped
            if leaves:
                damaged.append((origin, leaves[1:], table))                                  # the first leaf dropped
                damaged.append((origin, [(leaves[0][0], leaves[0][1] + b"\x01")] + leaves[1:], table))  # a value changed
                damaged.append((origin, [], table))                                          # "no leaves" where some exist
                damaged.append((origin, leaves, R.table_of([x for x in nodes if x != nodes[0]])))  # proof nodes removed: the root ...
                if len(nodes) > 1 and nodes[-1] != nodes[0]:
                    damaged.append((origin, leaves, R.table_of([x for x in nodes if x != nodes[-1]])))  # ... the deepest of the last key's
                extra = (int.from_bytes(leaves[-1][0], "big") + 1).to_bytes(32, "big") if leaves[-1][0] != bytes([255]) * 32 else None
                if extra and extra not in val:
                    damaged.append((origin, leaves + [(extra, b"x")], R.table_of(nodes + t.prove(extra))))  # an extra leaf
                if lo:
                    damaged.append((keys[lo - 1], leaves, R.table_of(nodes + t.prove(keys[lo - 1]))))       # the origin moved to the key before
                    damaged.append((origin, [(keys[lo - 1], val[keys[lo - 1]])] + leaves, table)) if origin > keys[lo - 1] else None  # a leaf below the origin
            for o2, l2, tb in damaged:
                st2, more2, got2, _ = R.verify(root, o2, l2, True, tb)
                assert not truth(val, o2, l2)[0] or tb is not table
                assert st2 != R.VALID and more2 == 0 and got2 == R.ZERO, (shape, trial, kind, st2, len(l2), len(leaves), o2 == origin)
                rejected += 1
        # without a proof the leaves are the whole trie
        assert R.verify(root, b"", list(zip(keys, vals)), False, {})[:3] == (R.VALID, 0, root)
        if len(keys) > 1:
            assert R.verify(root, b"", list(zip(keys, vals))[:-1], False, {})[0] == R.ROOT_MISMATCH
    assert accepted == 300 and rejected > 1000


def _by_hand(O):
    """a trie of five keys whose shape is known: a root branch; under nibble 1 an extension "234" over a branch with the leaves
    1234 5.. and 1234 9..; under nibble 7 a lone leaf 7777..; under nibble a the leaves a0.. and a8.."""
    keys = sorted(bytes.fromhex(x.ljust(64, "0")) for x in ("12345", "12349", "7777", "a0", "a8"))
    vals = [b"value of " + k[:3] * 12 for k in keys]
    return keys, vals, O.Trie(keys, vals)


def test_divergences_by_hand(O):
    keys, vals, t = _by_hand(O)
    root, val = t.root(), dict(zip(keys, vals))
    k = lambda x: bytes.fromhex(x.ljust(64, "0"))  # noqa: E731

    def claim(origin, served):
        leaves = [(x, val[x]) for x in served]
        nodes = t.prove(origin) + (t.prove(served[-1]) if served else [])
        return R.verify(root, origin, leaves, True, R.table_of(nodes))

    # the ORIGIN diverges at the leaf 7777: below it (the leaf is greater: in the range), above it (smaller: an item of the proof)
    assert claim(k("76"), keys[2:]) == (R.VALID, 0, root, R.NO_LEAF)
    assert claim(k("76"), keys[3:])[0] == R.ROOT_MISMATCH
    assert claim(k("78"), keys[3:]) == (R.VALID, 0, root, R.NO_LEAF)
    # ... at the extension 1|234: below it (greater: its two leaves are in the range), above it (smaller: its child is an item)
    assert claim(k("1230"), keys) == (R.VALID, 0, root, R.NO_LEAF)
    assert claim(k("1230"), keys[1:])[0] == R.ROOT_MISMATCH
    assert claim(k("1235"), keys[2:]) == (R.VALID, 0, root, R.NO_LEAF)
    assert claim(k("1235"), keys[2:3]) == (R.VALID, 1, root, R.NO_LEAF)
    # the LAST KEY's walk meets the same four cases when a claimed last key is not in the trie: whatever it leaves out or adds, no root
    for fake in ("76", "78", "1230", "1235"):
        served = sorted([x for x in keys if x < k(fake)] + [k(fake)])
        leaves = [(x, val.get(x, b"fake")) for x in served]
        st = R.verify(root, bytes(32), leaves, True, R.table_of(t.prove(bytes(32)) + t.prove(k(fake))))
        assert st[0] == R.ROOT_MISMATCH and st[1:] == (0, R.ZERO, R.NO_LEAF)
    # ... and with true last keys: the leaf 7777 greater than the last key (has_more), the extension's leaves behind 12345
    assert claim(bytes(32), keys[:2]) == (R.VALID, 1, root, R.NO_LEAF)
    assert claim(bytes(32), keys[:1]) == (R.VALID, 1, root, R.NO_LEAF)
    assert claim(bytes(32), keys[:3]) == (R.VALID, 1, root, R.NO_LEAF)
    assert claim(bytes(32), keys) == (R.VALID, 0, root, R.NO_LEAF)
    right = R.walk(root, keys[0], R.table_of(t.prove(keys[0])), True)
    assert [(len(p), kind) for p, kind, _ in right] == [(5, "ref"), (1, "ref"), (1, "ref")]
    left = R.walk(root, k("78"), R.table_of(t.prove(k("78"))), False)
    assert [(len(p), kind) for p, kind, _ in left] == [(1, "ref"), (64, "leaf")]
    left = R.walk(root, k("1235"), R.table_of(t.prove(k("1235"))), False)
    assert [(len(p), kind) for p, kind, _ in left] == [(4, "branch")]


def test_small_tries_by_hand(O):
    one = bytes.fromhex("42" * 32)
    root = O.mptize([one], [b"v"])
    for origin, more in ((bytes(32), 0), (one, 0)):
        assert R.verify(root, origin, [(one, b"v")], True, R.table_of(O.Trie([one], [b"v"]).prove(origin))) == (R.VALID, more, root, R.NO_LEAF)
    assert R.verify(root, bytes([255]) * 32, [], True, R.table_of(O.Trie([one], [b"v"]).prove(one))) == (R.VALID, 0, root, R.NO_LEAF)
    assert R.verify(root, bytes(32), [], True, R.table_of(O.Trie([one], [b"v"]).prove(one)))[0] == R.ROOT_MISMATCH
    for a, b in ((b"\x10" + bytes(31), b"\x20" + bytes(31)), (bytes(31) + b"\x10", bytes(31) + b"\x11")):  # 0 and 63 shared nibbles
        t = O.Trie([a, b], [b"x" * 40, b"y"])
        assert R.verify(t.root(), bytes(32), [(a, b"x" * 40)], True, R.table_of(t.prove(bytes(32)) + t.prove(a))) == (R.VALID, 1, t.root(), R.NO_LEAF)
        assert R.verify(t.root(), b, [(b, b"y")], True, R.table_of(t.prove(b))) == (R.VALID, 0, t.root(), R.NO_LEAF)
        assert R.verify(t.root(), bytes(32), [(a, b"x" * 40), (b, b"y")], False, {}) == (R.VALID, 0, t.root(), R.NO_LEAF)
    # the empty trie with and without a proof
    assert R.verify(R.EMPTY_ROOT, one, [], True, {}) == (R.VALID, 0, R.EMPTY_ROOT, R.NO_LEAF)
    assert R.verify(R.EMPTY_ROOT, one, [], False, {}) == (R.VALID, 0, R.EMPTY_ROOT, R.NO_LEAF)
    assert R.verify(R.EMPTY_ROOT, bytes(32), [(one, b"v")], True, {})[0] == R.ROOT_MISMATCH
    assert R.EMPTY_ROOT == O.keccak256(b"\x80")


def test_malformed_roots_and_the_order_of_the_statuses(O):
    ref = b"\xa0" + O.keccak256(b"child")
    bad = [R.rlp_list(ref * 2 + b"\x80" * 14 + b"\x01"),                                  # a branch with a value
           R.rlp_list(ref * 2 + b"\x80" * 14),                                            # a list of 16 items
           R.rlp_list(R.rlp_str(b"\x00") + ref),                                          # an extension with an empty path
           R.rlp_list(R.rlp_str(R.hex_prefix((1,) * 60, True)) + R.rlp_str(b"value")),    # a leaf whose path ends before nibble 64
           b"\xc2\x81\x05"]                                                               # not canonical RLP
    key = bytes.fromhex("11" * 32)
    for node in bad:
        # (a branch's value and a path's length are the walk's to refuse: they depend on the keys being 32 bytes)
        assert (R.decode_node(node) is None) == (node not in (bad[0], bad[3]))
        assert R.verify(O.keccak256(node), bytes(32), [(key, b"v")], True, R.table_of([node])) == (R.BAD_NODE, 0, R.ZERO, R.NO_LEAF)
    keys, vals, t = _by_hand(O)
    root, table = t.root(), R.table_of(t.prove(keys[0]) + t.prove(keys[-1]))
    leaves = list(zip(keys, vals))
    v = lambda origin, ls, tb=table: R.verify(root, origin, ls, True, tb)[::3]  # noqa: E731  (status, bad_leaf)
    # at one leaf: EMPTY_VALUE < VALUE_TOO_LONG < BAD_ORDER < BELOW_ORIGIN
    assert v(keys[1], [(keys[0], b"")] + leaves[1:]) == (R.EMPTY_VALUE, 0)
    assert v(keys[0], [leaves[0], (keys[0], bytes(561))]) == (R.VALUE_TOO_LONG, 1)
    assert v(keys[0], [leaves[0], (keys[0], bytes(560))]) == (R.BAD_ORDER, 1)
    assert v(keys[2], [leaves[1], leaves[0]]) == (R.BELOW_ORIGIN, 0)
    # the least leaf decides
    assert v(keys[0], [leaves[0], leaves[0], (keys[2], b"")]) == (R.BAD_ORDER, 1)
    # the leaf rules before the walks, the walks before the root, the origin's walk before the last key's
    assert v(keys[0], [(keys[0], b"")], {}) == (R.EMPTY_VALUE, 0)
    assert v(keys[0], leaves[:1] + leaves[2:], {}) == (R.MISSING_NODE, R.NO_LEAF)
    assert v(keys[0], leaves[:1] + leaves[2:]) == (R.ROOT_MISMATCH, R.NO_LEAF)
    top = R.rlp_list(b"".join(b"\xa0" + {3: O.keccak256(bad[0]), 9: O.keccak256(b"nowhere")}[s] if s in (3, 9) else b"\x80" for s in range(16)) + b"\x80")
    lo, hi = b"\x30" + bytes(31), b"\x90" + bytes(31)
    tb = R.table_of([top, bad[0]])
    assert R.verify(O.keccak256(top), lo, [(hi, b"v")], True, tb)[0] == R.BAD_NODE
    assert R.verify(O.keccak256(top), hi, [(hi, b"v")], True, tb)[0] == R.MISSING_NODE
    # a leaf of the proof itself beyond 560 bytes cannot be carried over: a mismatch
    big = O.Trie(keys, [bytes(600)] * 5)
    assert R.verify(big.root(), keys[2], leaves[2:], True, R.table_of(big.prove(keys[2]) + big.prove(keys[-1])))[0] == R.ROOT_MISMATCH
