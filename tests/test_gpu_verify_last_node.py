"""A proof's last node is decoded by the lane of the deep tier that hashes it (verify_hash.hip.h: decode_last_leaf) and the walk
takes the result from last[proof] instead of decoding the node itself (mpt_verify_v3.hip: walk_kernel's fast exit).  Every
status, value offset and value length must be the oracle's, whatever the node is: every case here is a batch of at most 200
proofs of depth 2-4 whose last nodes are built by hand -- well-formed leaves of every header form, leaves that prove absence,
and malformed nodes whose parent commits to their hash, so that the decoder is really reached and has to decline.

Every proof has a root of its own: full 532-byte branches with random slots lead to the last node, and the slot for the key's
nibble holds the Keccak-256 (the oracle's) of the node below.  A wave of 64 proofs whose last nodes have one length rides
(the decoder runs behind the parent's permutation); other waves take a trip of their own.  All cases run in the two-tier form
with 1 and 2 levels deduplicated and in the S = 0 form with the lane-per-node kernel forced (tests/test_gpu_verify_grids.py)."""
import numpy as np
import pytest

from tests.test_gpu_verify import _Mode
from tests.witness_util import pack_proofs

pytestmark = pytest.mark.gpu

PRESENT, ABSENT = 1, 2  # include/phant_gpu.h


@pytest.fixture(scope="module", params=["levels1", "levels2", "levels0"])
def M(request):
    import phant_amd
    ctx = phant_amd.Context(dedup_levels=int(request.param[6:]))
    if request.param == "levels0":
        ctx.diag_set("verify_no_coop", 1)  # hash_deep_kernel<true>, whatever the batch's size
    yield _Mode(phant_amd.mpt, ctx, request.param)
    ctx.close()


# ---------------------------------------------------------------- nodes by hand
def _hdr(base, n):
    if n <= 55:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def _str(b):
    return b if len(b) == 1 and b[0] < 0x80 else _hdr(0x80, len(b)) + b


def _list(items):
    pay = b"".join(items)
    return _hdr(0xc0, len(pay)) + pay


def _nibbles(key):
    return [x for b in key for x in (b >> 4, b & 15)]


def _hp(nibs, flag):
    """hex-prefix: flag 2 (leaf) or 0 (extension), + 1 for an odd path"""
    if len(nibs) % 2:
        head, rest = bytes([((flag | 1) << 4) | nibs[0]]), nibs[1:]
    else:
        head, rest = bytes([flag << 4]), nibs
    return head + bytes(rest[i] << 4 | rest[i + 1] for i in range(0, len(rest), 2))


def _leaf(key, pos, value):
    return _list([_str(_hp(_nibbles(key)[pos:], 2)), _str(value)])


def _proof(oracle, rng, key, depth, last_node):
    """(root, nodes): depth - 1 canonical full branches on the key's path, then last_node, committed to by its parent"""
    nib = _nibbles(key)
    nodes, h = [last_node], oracle.keccak256(last_node)
    for d in range(depth - 2, -1, -1):
        slots = [rng.bytes(32) for _ in range(16)]
        slots[nib[d]] = h
        br = b"\xf9\x02\x11" + b"".join(b"\xa0" + s for s in slots) + b"\x80"
        nodes.insert(0, br)
        h = oracle.keccak256(br)
    return h, nodes


def _batch(oracle, seed, n, depth, key_len=32, value_len=70, last=None):
    """n proofs of `depth` nodes for random keys; last(i, key, pos, value) -> the last node's bytes (default: the leaf);
    depth may be a function of i"""
    rng = np.random.default_rng(seed)
    roots, keys, proofs = [], [], []
    for i in range(n):
        key = rng.bytes(key_len)
        d = depth(i) if callable(depth) else depth
        value = bytes(rng.integers(0x80, 256, value_len, dtype=np.uint8))
        node = last(i, key, d - 1, value) if last else None
        root, nodes = _proof(oracle, rng, key, d, node if node is not None else _leaf(key, d - 1, value))
        roots.append(root)
        keys.append(key)
        proofs.append(nodes)
    return roots, keys, proofs


def _check(M, oracle, roots, keys, proofs, key_len=32):
    """statuses, value offsets and value lengths of the library == the oracle's; -> the oracle's statuses"""
    assert len(proofs) <= 200 and all(2 <= len(p) <= 4 for p in proofs)
    nodes, node_off, pfn = pack_proofs(proofs)
    r = np.frombuffer(b"".join(roots), np.uint8)
    k = np.frombuffer(b"".join(keys), np.uint8)
    ri = np.arange(len(roots), dtype=np.uint32)
    got = M.verify_batch(r, ri, k, key_len, nodes, node_off, pfn)
    want = oracle.mpt_verify_batch(r, ri, k, key_len, nodes, node_off, pfn)
    bad = np.flatnonzero(np.asarray(got[0]) != np.asarray(want[0]))
    assert bad.size == 0, (bad[:8], np.asarray(got[0])[bad[:8]], np.asarray(want[0])[bad[:8]])
    assert np.array_equal(got[1], want[1]), np.flatnonzero(np.asarray(got[1]) != np.asarray(want[1]))[:8]
    assert np.array_equal(got[2], want[2]), np.flatnonzero(np.asarray(got[2]) != np.asarray(want[2]))[:8]
    assert M._ctx.verify_path_stats()[0] == 0  # no proof verified from scratch
    return np.asarray(want[0])


# ---------------------------------------------------------------- well-formed leaves
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_wave_sizes(M, oracle, n):
    """up to, at and beyond a wave's edge, uniform length: the leaf rides"""
    want = _check(M, oracle, *_batch(oracle, 100 + n, n, 4))
    assert (want == PRESENT).all()


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_leaf_index(M, oracle, depth):
    """an odd index (flag 3) and an even one (flag 2); depth 2 with two levels deduplicated: a last node of the shallow tier"""
    roots, keys, proofs = _batch(oracle, 200 + depth, 130, depth)
    leaf = proofs[0][-1]
    assert leaf[0] == 0xf8 and leaf[2] > 0x81 and leaf[3] >> 4 == (3 if (depth - 1) % 2 else 2)  # list, path header, flag
    want = _check(M, oracle, roots, keys, proofs)
    assert (want == PRESENT).all()


@pytest.mark.parametrize("value_len", [1, 55, 56, 100])
@pytest.mark.parametrize("depth", [3, 4])
def test_value_length(M, oracle, depth, value_len):
    """across the short / long boundary of the string header (55 | 56) and of the list header (20-byte keys: payload 21 ..
    122); a value of one byte with a header (>= 0x80) and, every third proof, without one"""
    def last(i, key, pos, value):
        return _leaf(key, pos, b"\x05") if value_len == 1 and i % 3 == 0 and i >= 64 else None
    roots, keys, proofs = _batch(oracle, 300 + value_len, 130, depth, key_len=20, value_len=value_len, last=last)
    want = _check(M, oracle, roots, keys, proofs, key_len=20)
    assert (want == PRESENT).all()


@pytest.mark.parametrize("key_len,depth", [(1, 2), (1, 3), (20, 4), (32, 3), (32, 4), (33, 3), (33, 4)])
def test_key_length(M, oracle, key_len, depth):
    """(a key of one byte is used up after two branches: the leaf of depth 3 has the empty path)"""
    roots, keys, proofs = _batch(oracle, 400 + 10 * key_len + depth, 70, depth, key_len=key_len, value_len=40)
    want = _check(M, oracle, roots, keys, proofs, key_len=key_len)
    assert (want == PRESENT).all()


# ---------------------------------------------------------------- absence
def _other_path(kind):
    def last(i, key, pos, value):
        nib = _nibbles(key)[pos:]
        if kind == "first":
            nib[0] ^= 1
        elif kind == "last":
            nib[-1] ^= 8
        elif kind == "odd":  # the nibble that shares its byte with the flag (odd paths), the second one otherwise
            nib[0 if len(nib) % 2 else 1] ^= 4
        elif kind == "short":
            nib = nib[:-1]
        elif kind == "long":
            nib = nib + [7]
        return _list([_str(_hp(nib, 2)), _str(value)])
    return last


@pytest.mark.parametrize("depth", [3, 4])
def test_absence(M, oracle, depth):
    """a leaf whose path differs from the key's in its first, its last and its odd nibble, is a nibble short or a nibble long: a
    wave of each kind alone (those of the leaf's own length ride), then all of them mixed with leaves that match"""
    kinds = ["first", "last", "odd", "short", "long"]
    for kind in kinds:
        want = _check(M, oracle, *_batch(oracle, 500 + depth, 64, depth, last=_other_path(kind)))
        assert (want == ABSENT).all(), kind
    def last(i, key, pos, value):
        return _other_path(kinds[i % 7])(i, key, pos, value) if i % 7 < 5 else None
    want = _check(M, oracle, *_batch(oracle, 510 + depth, 130, depth, last=last))
    assert [(int(s) == ABSENT) for s in want] == [i % 7 < 5 for i in range(130)]


# ---------------------------------------------------------------- malformed last nodes
def _malformed(kind):
    def last(i, key, pos, value):
        path, good = _str(_hp(_nibbles(key)[pos:], 2)), _leaf(key, pos, value)
        if kind == "b8_short":  # the long string header over fewer than 56 bytes
            return _list([path, b"\xb8\x28" + value[:40]])
        if kind == "81_low":    # a header in front of a byte that is its own encoding
            return _list([path, b"\x81\x05"])
        if kind in ("list_len+1", "list_len-1"):
            nd = bytearray(good)
            nd[1 if nd[0] >= 0xf8 else 0] += 1 if kind.endswith("+1") else -1
            return bytes(nd)
        if kind == "three_items":
            return _list([path, _str(value), b"\x05"])
        if kind == "item1_list":
            return _list([path, _list([_str(value[:20])])])
        if kind.startswith("flag"):  # 0 and 1: an extension; 4 and 15: nothing
            nd = bytearray(good)
            at = len(good) - len(_str(value)) - len(path) + (0 if len(path) == 1 else 1)
            nd[at] = (int(kind[4:]) << 4) | (nd[at] & 15)
            return bytes(nd)
        if kind == "pad":  # an even flag with a pad nibble
            nib = _nibbles(key)[pos:]
            nib = nib if len(nib) % 2 == 0 else nib[1:]
            hp = bytearray(_hp(nib, 2))
            hp[0] |= 3
            return _list([_str(bytes(hp)), _str(value)])
        if kind == "empty":
            return b"\x80"
        raise AssertionError(kind)
    return last


MALFORMED = ["b8_short", "81_low", "list_len+1", "list_len-1", "three_items", "item1_list", "flag0", "flag1", "flag4", "flag15",
             "pad", "empty"]


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("value_len", [20, 70])
def test_malformed_last_nodes(M, oracle, depth, value_len):
    """each kind in a wave of its own (one length: it rides, the decoder sees it) and mixed with intact leaves; the hashes
    match, so what the proof is depends on the node's bytes alone"""
    for kind in MALFORMED:
        bad = _malformed(kind)
        want = _check(M, oracle, *_batch(oracle, 600 + depth, 64, depth, value_len=value_len, last=bad))
        assert (want != PRESENT).all(), kind
        def last(i, key, pos, value):
            return bad(i, key, pos, value) if i % 3 == 1 else None
        want = _check(M, oracle, *_batch(oracle, 610 + depth, 70, depth, value_len=value_len, last=last))
        assert [(int(s) == PRESENT) for s in want] == [i % 3 != 1 for i in range(70)], kind


# ---------------------------------------------------------------- mixed batches, stale records
def test_mixed_batches(M, oracle):
    """depth 4 but for: one proof a node shorter in the first wave (its lanes do not all end behind the depth-2 node: no ride)
    and one of two nodes (with two levels deduplicated its last node is the shallow tier's); in the second wave one last
    node of another length (hashed with the other lanes' loop: it leaves no record); the third wave rides"""
    def depth(i):
        return 3 if i == 5 else 2 if i == 40 else 4
    def last(i, key, pos, value):
        return _leaf(key, pos, value[:33]) if i == 64 + 17 else None
    roots, keys, proofs = _batch(oracle, 700, 130, depth, last=last)
    assert sum(len(p) for p in proofs) == 4 * 130 - 3
    want = _check(M, oracle, roots, keys, proofs)
    assert (want == PRESENT).all()


def test_stale_records(M, oracle):
    """one context: witness X, then Y of the same shape with other leaves, every fifth proof damaged (a byte of the leaf, of its
    parent's slot for it, or the leaf replaced by one for another key with the parent committing to it), then a batch small
    enough for the wave-per-node kernels, which record nothing: every result comes from the bytes of its own launch"""
    want = _check(M, oracle, *_batch(oracle, 800, 130, 4))
    assert (want == PRESENT).all()
    def last(i, key, pos, value):
        return _leaf(bytes(b ^ 0x5a for b in key), pos, value) if i % 15 == 10 else None
    roots, keys, proofs = _batch(oracle, 801, 130, 4, value_len=40, last=last)
    for i in range(0, 130, 15):
        nd = bytearray(proofs[i][3])
        nd[len(nd) // 2] ^= 0x20
        proofs[i][3] = bytes(nd)
    for i in range(5, 130, 15):
        nd = bytearray(proofs[i][2])
        nd[4 + 33 * _nibbles(keys[i])[2] + 9] ^= 0x01
        proofs[i][2] = bytes(nd)
    want = _check(M, oracle, roots, keys, proofs)
    assert [(int(s) == PRESENT) for s in want] == [i % 5 != 0 for i in range(130)]
    if M.mode == "levels0":
        M._ctx.diag_set("verify_no_coop", 0)
    try:
        def last3(i, key, pos, value):
            return _other_path("last")(i, key, pos, value) if i == 2 else None
        want = _check(M, oracle, *_batch(oracle, 802, 5, 4, value_len=40, last=last3))
        assert want.tolist() == [PRESENT, PRESENT, ABSENT, PRESENT, PRESENT]
    finally:
        if M.mode == "levels0":
            M._ctx.diag_set("verify_no_coop", 1)
    # ... and X's shape again, on whatever the small batch left
    want = _check(M, oracle, *_batch(oracle, 803, 130, 4))
    assert (want == PRESENT).all()
