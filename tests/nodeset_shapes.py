"""TEST INFRASTRUCTURE: node sets built to reach one thing each in the node-set verifier (phant_amd/csrc/mpt_verify_nodeset.hip), in plain
Python plus the oracle's Keccak-256.  No GPU.  tests/test_gpu_nodeset_choices.py runs them under every hash path.

The central trick is the SINGLE-LEAF TRIE: node j = rlp([hp(whole key j), value j]), its root = keccak256(node j), root_idx[j] = j and
n_roots = the node count.  Every node is looked up by exactly one key, so a wrong digest, record or length for node j shows as a
wrong status or value range of key j and of nothing else.

Every builder returns a NodeSet (or a list of them): the six arrays of a call -- `astuple()` = (roots, root_idx, keys, key_len, blob,
node_off) -- and the facts the tests assert about the shape: the nodes per list by the library's rule (`lists`), whether the nodes
are pairwise different (`distinct`), and `facts`, which every builder documents."""
import numpy as np

from tests.witness_util import _rlp_list, _rlp_str

RATE = 136
BRANCH_LEN = 532
N_LIST = 9
# status codes (include/phant_gpu.h)
PRESENT, ABSENT, MISSING_NODE, BAD_INPUT = 1, 2, 20, 21


def node_list(n: int) -> int:
    """the list a node of n bytes is hashed from (verify_hash.hip.h: node_list): exactly 532 bytes -> list 8, else rate blocks - 1,
    eight or more blocks -> 7"""
    return 8 if n == BRANCH_LEN else min(n // RATE, 7)


def hp(nibbles, leaf: bool) -> bytes:
    """hex-prefix encoding of a nibble path"""
    flag = 2 if leaf else 0
    if len(nibbles) % 2:
        out = [((flag + 1) << 4) | nibbles[0]]
        rest = nibbles[1:]
    else:
        out = [flag << 4]
        rest = nibbles
    out += [(rest[i] << 4) | rest[i + 1] for i in range(0, len(rest), 2)]
    return bytes(out)


def nibbles_of(key: bytes):
    return [x for b in key for x in (b >> 4, b & 15)]


def leaf_node(path_nibbles, value: bytes) -> bytes:
    return _rlp_list([_rlp_str(hp(path_nibbles, True)), _rlp_str(value)])


def _value(rng, n: int) -> bytes:
    v = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    if n == 1:
        v[0] |= 0x80  # (a single byte below 0x80 is its own encoding: the node would be a byte shorter)
    return bytes(v)


class NodeSet:
    def __init__(self, roots, root_idx, keys, key_len, nodes, distinct=True, facts=None):
        self.nodes = list(nodes)
        self.roots = list(roots)
        self.keys = list(keys)
        self.key_len = key_len
        self.r = np.frombuffer(b"".join(self.roots), np.uint8).copy()
        self.ridx = None if root_idx is None else np.asarray(root_idx, np.uint32)
        self.karr = np.frombuffer(b"".join(self.keys), np.uint8).copy()
        self.off = np.zeros(len(self.nodes) + 1, np.uint64)
        if self.nodes:
            self.off[1:] = np.cumsum([len(x) for x in self.nodes])
        self.blob = np.frombuffer(b"".join(self.nodes), np.uint8).copy()
        self.lists = [0] * N_LIST
        for nd in self.nodes:
            self.lists[node_list(len(nd))] += 1
        self.distinct = distinct
        self.facts = facts or {}
        self._want = None

    @property
    def n_nodes(self):
        return len(self.nodes)

    @property
    def n(self):
        return len(self.keys)

    def astuple(self):
        return self.r, self.ridx, self.karr, self.key_len, self.blob, self.off

    def want(self, oracle):
        """the oracle's (status, value_off, value_len) on these arrays: computed once, shared by every test and setting"""
        if self._want is None:
            blob = self.blob if self.blob.size else np.zeros(1, np.uint8)
            self._want = oracle.mpt_verify_nodeset(self.r, self.ridx, self.karr, self.key_len, blob, self.off)
        return self._want

    def stripe_counts(self):
        """{(list, stripe): nodes}: classify workgroup b takes nodes [256 b, 256 b + 256) and appends to stripe b mod 8"""
        out = {}
        for j, nd in enumerate(self.nodes):
            k = (node_list(len(nd)), (j // 256) % 8)
            out[k] = out.get(k, 0) + 1
        return out


def _digests(oracle, nodes):
    blob = np.frombuffer(b"".join(nodes), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in nodes])]).astype(np.uint64)
    if blob.size == 0:
        return [oracle.keccak256(x) for x in nodes]
    return [bytes(d) for d in oracle.keccak256_batch(blob, off)]


def single_leaf_set(oracle, keys, values, order=None, extra_nodes=(), facts=None):
    """one single-leaf trie per (key, value); node j at place order[j] of the blob; `extra_nodes` (never referenced) behind them"""
    key_len = len(keys[0])
    nodes = [leaf_node(nibbles_of(k), v) for k, v in zip(keys, values)]
    roots = _digests(oracle, nodes)
    placed = nodes if order is None else [nodes[i] for i in order]
    return NodeSet(roots, np.arange(len(keys)), keys, key_len, list(placed) + list(extra_nodes),
                   distinct=len(set(placed) | set(extra_nodes)) == len(placed) + len(extra_nodes), facts=facts)


def leaf_lengths(key_len: int, max_value: int):
    """{node length: value length} of the single-leaf nodes with a key of key_len bytes (the shortest value that gives the length)"""
    out = {}
    key = bytes(key_len)
    for v in range(1, max_value + 1):
        out.setdefault(len(leaf_node(nibbles_of(key), b"\x80" * v)), v)
    return out


def _keys(rng, n, key_len):
    return [rng.integers(0, 256, key_len, dtype=np.uint8).tobytes() for _ in range(n)]


def _leaf_of_length(rng, key_len, length, by_len=None):
    by_len = by_len or leaf_lengths(key_len, length)
    assert length in by_len, f"no single-leaf node of {length} bytes with a {key_len}-byte key"
    k = _keys(rng, 1, key_len)[0]
    return k, _value(rng, by_len[length])


# ---------------------------------------------------------------- every length
def every_length(oracle, key_len, lo, hi, seed=1):
    """One single-leaf trie per reachable node length in [lo, hi], shuffled.  facts: `lengths` (sorted), `unreachable`."""
    rng = np.random.default_rng([seed, key_len, lo, hi])
    by_len = leaf_lengths(key_len, hi)
    lengths = [n for n in range(lo, hi + 1) if n in by_len]
    keys = _keys(rng, len(lengths), key_len)
    values = [_value(rng, by_len[n]) for n in lengths]
    s = single_leaf_set(oracle, keys, values, order=rng.permutation(len(lengths)),
                        facts={"lengths": lengths, "unreachable": [n for n in range(lo, hi + 1) if n not in by_len]})
    assert sorted(len(x) for x in s.nodes) == lengths
    return s


# ---------------------------------------------------------------- the rate boundaries, at both ends of the blob
BOUNDARY_LENGTHS = sorted({RATE * k + d for k in range(1, 10) for d in (-1, 0, 1)} | {531, 532, 533, 543, 544, 545, 191, 192, 193})
LONG_NODE = 5000  # (about: the nearest length a leaf can have)


def lengths_at_boundaries(oracle, key_len, firsts=None, seed=2):
    """The lengths around every rate-block boundary up to nine blocks (136 k - 1, 136 k, 136 k + 1), around the 532-byte list
    (531 .. 533), the 544-byte class boundary, the walk's staging edge (191 .. 193) and one node of about 5 000 bytes: three different
    nodes of every length.  One blob per (shift, length L): a first filler node of `shift` = 0 .. 3 bytes (it moves every other node's
    alignment), then a node of L bytes -- the first real node of the blob --, then one node of every length in a shuffled middle, and
    a second node of L bytes as the LAST node of the blob: the one whose final rate block must be read with narrow loads
    (hash_any: p + RATE > safe_end, at an alignment that changes with the shift) and whose 16-byte padded copy would cross the
    blob's end (the walk's staging test).  `firsts`: the lengths L that take the two ends (default: all of them).
    -> a list of NodeSets; facts: `lengths` (of the middle), `shift`, `end_length`."""
    rng = np.random.default_rng([seed, key_len])
    by_len = leaf_lengths(key_len, LONG_NODE + 16)
    long_len = min(n for n in by_len if n >= LONG_NODE)
    lengths = BOUNDARY_LENGTHS + [long_len]
    assert all(n in by_len for n in lengths)
    trio = {n: [_leaf_of_length(rng, key_len, n, by_len) for _ in range(3)] for n in lengths}
    out = []
    for shift in range(4):
        filler = rng.integers(0, 256, shift, dtype=np.uint8).tobytes()
        for L in (firsts if firsts is not None else lengths):
            middle = [trio[n][1] for n in lengths]
            middle = [middle[i] for i in rng.permutation(len(middle))]
            kv = [trio[L][0]] + middle + [trio[L][2]]
            keys, values = [k for k, _ in kv], [v for _, v in kv]
            nodes = [leaf_node(nibbles_of(k), v) for k, v in kv]
            roots = _digests(oracle, nodes)
            out.append(NodeSet(roots, np.arange(len(kv)), keys, key_len, [filler] + nodes,
                               facts={"lengths": lengths, "shift": shift, "end_length": L}))
            assert len(set(out[-1].nodes)) == out[-1].n_nodes
    return out


# ---------------------------------------------------------------- chosen counts per list and stripe
SHORT_LEN = {0: 70, 1: 200, 2: 300, 3: 450, 4: 560, 5: 700, 6: 850, 7: 1000, 8: BRANCH_LEN}  # a node length of every list


def list_counts(oracle, plan, pad_list=0, tail=0, seed=3, lengths=None):
    """A set in which classify workgroup b (nodes [256 b, 256 b + 256), stripe b mod 8) holds exactly plan[b][l] nodes of list l; the
    rest of every workgroup but the last is padding of list `pad_list`, the last workgroup gets `tail` padding nodes.  Inside a
    workgroup the nodes are shuffled.  lengths: {list: node length} (default SHORT_LEN).
    facts: `per_stripe` {(list, stripe): count} as planned (the test compares it with NodeSet.stripe_counts())."""
    rng = np.random.default_rng([seed, pad_list, tail, len(plan)])
    lengths = dict(SHORT_LEN, **(lengths or {}))
    by_len = leaf_lengths(32, max(lengths.values()))
    keys, values, per_stripe = [], [], {}
    for b, want in enumerate(plan):
        last = b + 1 == len(plan)
        cls = [l for l, c in sorted(want.items()) for _ in range(c)]
        assert len(cls) <= 256
        cls += [pad_list] * (tail if last else 256 - len(cls))
        assert last or len(cls) == 256
        cls = [cls[i] for i in rng.permutation(len(cls))]
        for l in cls:
            n = lengths[l]
            assert node_list(n) == l
            keys.append(_keys(rng, 1, 32)[0])
            values.append(_value(rng, by_len[n]))
            per_stripe[(l, b % 8)] = per_stripe.get((l, b % 8), 0) + 1
    return single_leaf_set(oracle, keys, values, facts={"per_stripe": per_stripe})


CHUNK_EDGES = (1, 63, 64, 65, 128, 129)


def list_count_sets(oracle, lists=range(N_LIST)):
    """For every list l: six workgroups, workgroup b holds CHUNK_EDGES[b] nodes of list l -- stripe b of list l is a chunk queue of 1,
    63, 64, 65, 128, 129 nodes -- and padding of the shortest other list.  Then one set of 2 305 nodes (ten workgroups): workgroup 0
    leaves 65 nodes of list 2 in stripe 0, workgroup 8 appends 64 more behind them, workgroup 9 holds a single node."""
    out = [list_counts(oracle, [{l: c} for c in CHUNK_EDGES], pad_list=1 if l == 0 else 0, seed=30 + l) for l in lists]
    plan = [{2: 65}] + [{3: 5}] * 7 + [{2: 64}] + [{}]
    out.append(list_counts(oracle, plan, pad_list=0, tail=1, seed=40))
    assert out[-1].n_nodes == 2305
    return out


def short_uniform_sets(oracle, seed=4):
    """64 short leaves of one length in one chunk of list 0, with a longer node behind them in the blob so that every lane may read a
    whole rate block (hash_short_uniform runs); and the same with one leaf of another length among the 64 (it does not)."""
    out = []
    for odd in (False, True):
        rng = np.random.default_rng([seed, odd])
        by_len = leaf_lengths(32, 300)
        lens = [70] * 64
        if odd:
            lens[37] = 71
        lens.append(300)
        keys = _keys(rng, 65, 32)
        values = [_value(rng, by_len[n]) for n in lens]
        out.append(single_leaf_set(oracle, keys, values, facts={"uniform": not odd}))
        assert out[-1].lists[0] == 64 and out[-1].lists[2] == 1 and len(out[-1].nodes[-1]) == 300
    return out


# ---------------------------------------------------------------- nodes that are almost the canonical full branch
MARKERS = [0, 1, 2] + [3 + 33 * k for k in range(16)] + [531]


def not_quite_branches(oracle, seed=5):
    """The canonical full branch f9 02 11 | 16 x (a0 | 32 bytes) | 80 whose child 0 is a leaf of the set (key = 32 zero bytes: PRESENT),
    and for each of its 20 marker bytes copies with that byte altered (^ 0x01, ^ 0x80, ^ 0x10): 532 bytes long, NOT canonical --
    none of them may be walked by taking 32 bytes at 4 + 33 x nibble.  Every copy is a committed root of its own.  Further: a
    532-byte LEAF (it begins f9 02 11 a1) and 532-byte branches with one empty child and a 32-byte value (the empty child at nibble 0,
    at nibble 15).
    Asserts that for every marker position an altered copy has an oracle status different from the canonical node's (^ 0x80 at byte
    531 is the branch with value 0x00, which walks on like the canonical one: a case, not counted).
    facts: `cases` [(name, marker position or None)], in root order; `canonical_status`; `distinguishing` {position: [names]}."""
    rng = np.random.default_rng(seed)
    key = bytes(32)
    child = leaf_node([0] * 63, _value(rng, 40))
    refs = [oracle.keccak256(child)] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(15)]
    canon = b"\xf9\x02\x11" + b"".join(b"\xa0" + r for r in refs) + b"\x80"
    assert len(canon) == BRANCH_LEN
    cases = [("canonical", None, canon)]
    for q in MARKERS:
        for name, f in (("xor01", lambda b: b ^ 0x01), ("xor80", lambda b: b ^ 0x80), ("xor10", lambda b: b ^ 0x10)):
            nd = bytearray(canon)
            nd[q] = f(nd[q])
            cases.append((f"{name}@{q}", q, bytes(nd)))
    k532, v532 = _leaf_of_length(rng, 32, BRANCH_LEN)
    leaf532 = leaf_node(nibbles_of(k532), v532)
    assert len(leaf532) == BRANCH_LEN and leaf532[:4] == b"\xf9\x02\x11\xa1"
    value = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    for name, empty in (("empty_child0_value32", 0), ("empty_child15_value32", 15)):
        items = [b"\x80" if i == empty else b"\xa0" + refs[i] for i in range(16)]
        nd = b"\xf9\x02\x11" + b"".join(items) + b"\xa0" + value
        assert len(nd) == BRANCH_LEN
        cases.append((name, None, nd))
    nodes = [c[2] for c in cases] + [leaf532]
    roots = _digests(oracle, nodes)
    keys = [key] * len(cases) + [k532]
    s = NodeSet(roots, np.arange(len(nodes)), keys, 32, nodes + [child])
    assert len(set(s.nodes)) == s.n_nodes
    st = s.want(oracle)[0]
    assert st[0] == PRESENT and st[-1] == PRESENT
    distinguishing = {q: [] for q in MARKERS}
    for i, (name, q, _) in enumerate(cases):
        if q is not None and st[i] != st[0] and name != "xor80@531":
            distinguishing[q].append(name)
    assert all(distinguishing[q] for q in MARKERS), distinguishing
    s.facts = {"cases": [(n_, q) for n_, q, _ in cases] + [("leaf532", None)], "canonical_status": int(st[0]),
               "distinguishing": distinguishing}
    return s


# ---------------------------------------------------------------- a chain of canonical full branches
def deep_chain(oracle, depth, key_len, seed=6, end="leaf"):
    """A hand-built chain of `depth` canonical full branches along one key: child nibble_i of branch i = keccak256(the next node), the
    other fifteen children random; behind the last branch a leaf with the rest of the key (end = "leaf"; depth = 2 key_len: the
    empty path) or -- depth = 2 key_len only -- one more canonical full branch, met with the key used up (end = "branch": it has no
    value, the key is ABSENT).  Queries: the key; for every level a key that leaves the chain there (its sibling is not in the set:
    MISSING_NODE); keys that differ from the key only inside the leaf's path (ABSENT).
    facts: `expected` (status per query, which the test also compares with the oracle's), `depth`."""
    rng = np.random.default_rng([seed, depth, key_len, end == "leaf"])
    nn = 2 * key_len
    assert depth <= nn and (end == "leaf" or depth == nn)
    key = _keys(rng, 1, key_len)[0]
    nib = nibbles_of(key)
    value = _value(rng, 33)

    def branch(at, child_ref):
        refs = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(16)]
        if at is not None:
            refs[at] = child_ref
        return b"\xf9\x02\x11" + b"".join(b"\xa0" + r for r in refs) + b"\x80"

    nodes = [leaf_node(nib[depth:], value) if end == "leaf" else branch(None, None)]
    for i in reversed(range(depth)):
        nodes.append(branch(nib[i], oracle.keccak256(nodes[-1])))
    root = oracle.keccak256(nodes[-1])

    def with_nibble(i, x):
        nb = list(nib)
        nb[i] = x
        return bytes((nb[2 * t] << 4) | nb[2 * t + 1] for t in range(key_len))

    queries, expected = [key], [PRESENT if end == "leaf" else ABSENT]
    for i in range(depth):
        queries.append(with_nibble(i, (nib[i] + 1 + int(rng.integers(0, 15))) % 16))
        expected.append(MISSING_NODE)
    for i in sorted({depth, (depth + nn) // 2, nn - 1}):
        if end == "leaf" and depth <= i < nn:
            queries.append(with_nibble(i, nib[i] ^ 1))
            expected.append(ABSENT)
    nodes = [nodes[i] for i in rng.permutation(len(nodes))]
    s = NodeSet([root], None, queries, key_len, nodes, facts={"expected": expected, "depth": depth})
    assert s.lists[8] == depth + (end == "branch")
    return s


DEEP_CHAINS = [(15, 32, "leaf"), (16, 32, "leaf"), (17, 32, "leaf"), (20, 32, "leaf"), (20, 40, "leaf"), (1, 1, "leaf")] + \
              [(2 * k, k, e) for k in (1, 4, 7, 8, 9) for e in ("leaf", "branch")]


# ---------------------------------------------------------------- copies
def copies(oracle, distinct, c, flood, key_len=32, seed=7):
    """`distinct` different single-leaf nodes, every one `c` times, plus `flood` further copies of the first, shuffled.  One key per
    distinct node; which copy a value range points into is the verifier's choice (the tests compare the bytes).
    facts: `values` (per key), `total`, `distinct`."""
    rng = np.random.default_rng([seed, distinct, c, flood])
    keys = _keys(rng, distinct, key_len)
    values = [_value(rng, int(rng.integers(1, 120))) for _ in range(distinct)]
    nodes = [leaf_node(nibbles_of(k), v) for k, v in zip(keys, values)]
    assert len(set(nodes)) == distinct
    roots = _digests(oracle, nodes)
    shipped = [nd for nd in nodes for _ in range(c)] + [nodes[0]] * flood
    shipped = [shipped[i] for i in rng.permutation(len(shipped))]
    return NodeSet(roots, np.arange(distinct), keys, key_len, shipped, distinct=len(shipped) == distinct,
                   facts={"values": values, "total": len(shipped), "distinct": distinct})
