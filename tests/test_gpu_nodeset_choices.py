"""The node-set verifier (phant_amd/csrc/mpt_verify_nodeset.hip) under every hash path it has, each FORCED on the GPU over node sets
chosen for it (tests/nodeset_shapes.py), bit-exact against the oracle -- and, through Context.nodeset_stats() (phant_nodeset_stats),
the proof that the call took the path the case names: a wave per node in workgroups of one or of four waves, or the class lists;
the nodes per list; the overflow count; the hash grid.

Without the knobs a set of up to 3 500 nodes never sees set_classify_kernel / set_hash_kernel, the alternatives of
phant_nodeset_tune (the plain and the requested-ahead form of the 532-byte hash, the rising queue order, a capped grid whose waves
stride over the chunk queue) run nowhere, and no referenced node is longer than 532 bytes.  The settings:

    wave     nodeset_wave_max = 2^20                          a wave per node at every size
    lists    nodeset_wave_max = 0, the default tune           classify + a lane per node
    plain    ... form 0, no idle LDS                          ahead    ... form 2 (hash_b532_ahead)
    rising   ... order 1                                      stride1  ... a grid of ONE workgroup striding over the queue
    stride3  ... order 1, no idle LDS, a grid of three

tests/test_emu_nodeset_choices.py runs the same bodies over the emulated library at the sizes tests/suite.py gives emulated runs."""
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

from tests import nodeset_shapes as S
from tests import suite

pytestmark = pytest.mark.gpu

KIB40 = 40 * 1024
DEFAULT_TUNE = (1, 0, KIB40, 0)
SETTINGS = {  # name: (nodeset_wave_max, nodeset_tune(form, order, hash_lds, resident_wgs))
    "wave": (1 << 20, DEFAULT_TUNE),
    "lists": (0, DEFAULT_TUNE),
    "plain": (0, (0, 0, 0, 0)),
    "ahead": (0, (2, 0, KIB40, 0)),
    "rising": (0, (1, 1, KIB40, 0)),
    "stride1": (0, (1, 0, KIB40, 1)),
    "stride3": (0, (1, 1, 0, 3)),
}
BOTH = ("wave", "lists")
N_QUEUE = 72  # nine lists x eight stripes: the hash grid is the classify grid + a short chunk per queue entry, in workgroups of four waves


def default_wave_max():
    if suite.EMULATED and not suite.FULL:
        from tests import emu
        return emu.EMU_NODESET_WAVE_NODES
    return 3500


@contextmanager
def forced(ctx, setting):
    wave_max, tune = SETTINGS[setting]
    try:
        ctx.diag_set("nodeset_wave_max", wave_max)
        ctx.nodeset_tune(*tune)
        yield
    finally:
        ctx.diag_set("nodeset_wave_max", default_wave_max())
        ctx.nodeset_tune(*DEFAULT_TUNE)


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def new_context(P):
    """A Context of the test's own (the emulated library's under tests/test_emu_nodeset_choices.py)."""
    if suite.EMULATED:
        from tests import emu
        return emu.mirror_context(emu.mirror_lib())
    return P.Context(0)


@pytest.fixture(scope="module")
def ctx(P):
    c = new_context(P)
    yield c
    c.close()


# ---- what a call must report, from the set and the setting ----
def expect_stats(s, setting, st, what):
    n = s.n_nodes
    wave_max, tune = SETTINGS[setting]
    ng = (n + 255) // 256 if n else 1
    if n and n <= wave_max:
        path, grid = (1, n) if n <= 512 else (2, (n + 3) // 4)
    else:
        every = ng + (N_QUEUE + 3) // 4
        path, grid = 3, (min(tune[3], every) if tune[3] else every) if n else 0
    assert st[0] == path, f"{what}: path {st[0]}, forced {path}"
    assert st[1:10] == s.lists, f"{what}: nodes per list {st[1:10]}, expected {s.lists}"
    assert st[11] == grid, f"{what}: hash grid {st[11]}, expected {grid}"
    assert st[12] == n, f"{what}: {st[12]} nodes offered, expected {n}"
    if s.distinct:
        assert st[10] == 0, f"{what}: {st[10]} nodes on the overflow list of a set of distinct nodes"


def run(P, ctx, oracle, s, setting, what, table=None):
    """one call under a setting in force: results = the oracle's, statistics = the forced path's; -> (results, statistics)"""
    got = P.mpt.verify_nodeset(*s.astuple(), ctx=ctx)
    st = ctx.nodeset_stats()
    want = s.want(oracle)
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, f"{what}: status of keys {bad[:8].tolist()}: {got[0][bad[:8]].tolist()}, oracle {want[0][bad[:8]].tolist()}"
    assert np.array_equal(got[2], want[2]), f"{what}: value_len of keys {np.nonzero(got[2] != want[2])[0][:8].tolist()}"
    if s.distinct:
        assert np.array_equal(got[1], want[1]), f"{what}: value_off of keys {np.nonzero(got[1] != want[1])[0][:8].tolist()}"
    else:  # (which copy a value range points into is the verifier's choice)
        for i in np.nonzero(want[0] == S.PRESENT)[0]:
            a, b, m = int(got[1][i]), int(want[1][i]), int(want[2][i])
            assert a + m <= s.blob.size and s.blob[a:a + m].tobytes() == s.blob[b:b + m].tobytes(), f"{what}: value of key {i}"
    expect_stats(s, setting, st, what)
    if table is not None:
        table.append((what, setting, st))
    return got, st


# ---- the shapes of the matrix: name -> list of sets (built once) ----
BOUNDARY_KEY_LENS = (1, 32, 40)
EVERY_LENGTH = {1: (6, 1308), 32: (37, 1339), 40: (45, 1347)}
# the emulated default suite: a window of lengths around the 532-byte list and the 544-byte class boundary, one around the first rate
# boundary with the shortest keys, the last class boundary with the longest; the boundary lengths that take the two ends of a blob
# thinned to one of every kind (below a block, a whole block, 532, the longest)
EVERY_LENGTH_EMULATED = {1: (120, 150), 32: (525, 550), 40: (1080, 1095)}
BOUNDARY_ENDS_EMULATED = (135, 136, 192, 532, 1088)


@lru_cache(maxsize=None)
def _shape(oracle, name, full):
    kind, _, arg = name.partition("_k")
    if kind == "every_length":
        lo, hi = (EVERY_LENGTH if full else EVERY_LENGTH_EMULATED)[int(arg)]
        return [S.every_length(oracle, int(arg), lo, hi)]
    if kind == "boundaries":
        sets = S.lengths_at_boundaries(oracle, int(arg), firsts=None if full else BOUNDARY_ENDS_EMULATED)
        return sets if full else [s for s in sets if s.facts["shift"] == BOUNDARY_ENDS_EMULATED.index(s.facts["end_length"]) % 4]
    if name == "list_counts":
        return S.list_count_sets(oracle) if full else S.list_count_sets(oracle, lists=(0, 8))[:2]
    if name == "short_uniform":
        return S.short_uniform_sets(oracle)
    if name == "not_quite_branches":
        return [S.not_quite_branches(oracle)]
    raise KeyError(name)


def shape(oracle, name, full=None):
    return _shape(oracle, name, suite.scale(True, False) if full is None else full)


SHAPES = ["every_length_k1", "every_length_k32", "every_length_k40", "boundaries_k1", "boundaries_k32", "boundaries_k40",
          "list_counts", "short_uniform", "not_quite_branches"]
STATS_TABLE = []  # (what, setting, nodeset_stats()) of this module's calls, for whoever runs it and wants the record


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", SHAPES)
def test_shape_under_every_setting(P, ctx, oracle, name, setting):
    sets = shape(oracle, name)
    with forced(ctx, setting):
        for k, s in enumerate(sets):
            got, st = run(P, ctx, oracle, s, setting, f"{name}[{k}] under {setting}")
            if k == 0 or name == "list_counts":
                STATS_TABLE.append((f"{name}[{k}]", setting, st))
    if name == "not_quite_branches":  # (what the comparison with the oracle already says, spelled out)
        cases = sets[0].facts["cases"]
        for i, (case, q) in enumerate(cases):
            if q is not None and case in sets[0].facts["distinguishing"][q]:
                assert got[0][i] != got[0][0], f"{case} walked on like the canonical full branch under {setting}"


def test_the_shapes_reach_what_they_aim_at(oracle):
    """The builders, on the CPU, at the sizes of the GPU run: a shape that no longer reaches its edge fails here, not silently."""
    for key_len, (lo, hi) in EVERY_LENGTH.items():
        s = shape(oracle, f"every_length_k{key_len}", full=True)[0]
        assert all(c > 0 for c in s.lists), (key_len, s.lists)
        lens = set(s.facts["lengths"])
        assert {lo, hi, 532, 543, 544, 545} <= lens and all({136 * k - 1, 136 * k, 136 * k + 1} <= lens for k in range(1, 10) if 136 * k - 1 >= lo)
        assert len(s.facts["unreachable"]) == 4 and 57 in s.facts["unreachable"] and s.n_nodes == hi - lo + 1 - 4
        assert s.distinct and (s.want(oracle)[0] == S.PRESENT).all()
    for key_len in BOUNDARY_KEY_LENS:
        sets = shape(oracle, f"boundaries_k{key_len}", full=True)
        lengths = sets[0].facts["lengths"]
        assert set(S.BOUNDARY_LENGTHS) < set(lengths) and 4990 < max(lengths) < 5030
        assert {(s.facts["shift"], s.facts["end_length"]) for s in sets} == {(sh, n) for sh in range(4) for n in lengths}
        for s in sets:
            got = [len(x) for x in s.nodes]
            assert got[0] == s.facts["shift"] and got[1] == got[-1] == s.facts["end_length"] and sorted(got[2:-1]) == sorted(lengths)
            assert s.distinct and (s.want(oracle)[0] == S.PRESENT).all()
        # the last node's final rate block starts at every alignment
        assert {int(s.off[-2] + (len(s.nodes[-1]) // 136) * 136) & 3 for s in sets} == {0, 1, 2, 3}
    sets = shape(oracle, "list_counts", full=True)
    for l, s in enumerate(sets[:-1]):
        assert s.stripe_counts() == s.facts["per_stripe"]
        assert tuple(s.facts["per_stripe"][(l, b)] for b in range(6)) == S.CHUNK_EDGES
    big = sets[-1]
    assert big.n_nodes >= 2305 and big.stripe_counts() == big.facts["per_stripe"] and big.facts["per_stripe"][(2, 0)] == 129
    assert [S.node_list(len(x)) for x in big.nodes[:256]].count(2) == 65 and [S.node_list(len(x)) for x in big.nodes[2048:2304]].count(2) == 64
    uni, odd = shape(oracle, "short_uniform", full=True)
    assert len({len(x) for x in uni.nodes[:64]}) == 1 and len({len(x) for x in odd.nodes[:64]}) == 2
    assert all(int(s.off[64]) + 136 <= s.blob.size for s in (uni, odd))  # (every lane of the chunk may read a whole rate block)
    nq = shape(oracle, "not_quite_branches", full=True)[0]
    assert sorted(nq.facts["distinguishing"]) == sorted(S.MARKERS) and all(nq.facts["distinguishing"].values())
    assert nq.lists[8] == nq.n_nodes - 1
    for depth, key_len, end in S.DEEP_CHAINS:
        s = S.deep_chain(oracle, depth, key_len, end=end)
        assert s.want(oracle)[0].tolist() == s.facts["expected"], (depth, key_len, end)


def _short_leaves(oracle, n, seed):
    rng = np.random.default_rng([11, n, seed])
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    values = [rng.integers(0, 256, int(rng.integers(2, 60)), dtype=np.uint8).tobytes() for _ in range(n)]
    return S.single_leaf_set(oracle, keys, values)


def test_wave_grid_edges(P, ctx, oracle):
    """A wave per node: workgroups of one wave up to 512 nodes, of four beyond -- whose last workgroup is not full at 513, 514, 515."""
    with forced(ctx, "wave"):
        for n in suite.scale((1, 2, 511, 512, 513, 514, 515), (1, 2, 512, 513, 514)):
            s = _short_leaves(oracle, n, 0)
            _, st = run(P, ctx, oracle, s, "wave", f"{n} nodes", STATS_TABLE)
            assert st[0] == (1 if n <= 512 else 2) and st[11] == (n if n <= 512 else (n + 3) // 4)


@pytest.mark.parametrize("setting", BOTH)
def test_overflow_counts(P, ctx, oracle, setting):
    """Copies: the record table takes one of them, every other goes to the overflow list and the second table."""
    with forced(ctx, setting):
        for n in suite.scale((2, 64, 65, 3000), (2, 64, 65, 300)):
            s = S.copies(oracle, 1, 1, n - 1)
            got, st = run(P, ctx, oracle, s, setting, f"{n} copies of one node under {setting}", STATS_TABLE)
            assert st[10] == n - 1 and got[0].tolist() == [S.PRESENT]
        d = suite.scale(600, 150)
        s = S.copies(oracle, d, 2, 0)
        got, st = run(P, ctx, oracle, s, setting, f"{d} nodes twice under {setting}", STATS_TABLE)
        # (a copy may land in a second record slot when a higher tag has passed over the first: both are found, neither is wrong)
        assert 1 <= st[10] <= s.facts["total"] - s.facts["distinct"], st[10]
        assert (got[0] == S.PRESENT).all()
        for i, v in enumerate(s.facts["values"]):
            assert s.blob[int(got[1][i]):int(got[1][i]) + int(got[2][i])].tobytes() == v


def test_an_older_launch_never_answers(P, oracle):
    """A record, a claim word or a second-table entry of an older launch must never resolve a reference: one context, twelve
    launches alternating the class lists and the wave per node, over A, A without node X, B (disjoint from A), A, A with X only as
    a pair of copies (one of them lives in the second table), that set without the pair -- twice, with a launch of keys but no
    nodes in between, so that every path meets both parities of the epoch twice."""
    from tests.witness_util import random_kv
    rng = np.random.default_rng(77)
    ka, va = random_kv(rng, 60, 32, 1, 90)
    kb, vb = random_kv(rng, 60, 32, 1, 90)
    ta, tb = oracle.Trie(ka, va), oracle.Trie(kb, vb)
    proofs_a = [ta.prove(k) for k in ka]
    set_a = list(dict.fromkeys(nd for p in proofs_a for nd in p))
    set_b = list(dict.fromkeys(nd for k in kb for nd in tb.prove(k)))
    assert not set(set_a) & set(set_b)
    x = proofs_a[0][1]  # a child of A's root
    through_x = np.array([x in p for p in proofs_a] + [False] * len(kb))
    assert 0 < through_x.sum() < len(ka)
    without_x = [nd for nd in set_a if nd != x]
    keys = ka + kb
    ridx = np.array([0] * len(ka) + [1] * len(kb), np.uint32)
    roots = [ta.root(), tb.root()]

    def nodeset(nodes, distinct=True):
        nodes = [nodes[i] for i in rng.permutation(len(nodes))]
        return S.NodeSet(roots, ridx, keys, 32, nodes, distinct=distinct)

    sequence = [("A", set_a, True), ("A without X", without_x, False), ("B", set_b, False), ("A again", set_a, True),
                ("A, X as a pair", without_x + [x, x], True), ("... without the pair", without_x, False)]
    c = new_context(P)
    seen = {}
    try:
        step = 0
        for half in range(2):
            for what, nodes, has_x in sequence:
                setting = BOTH[1 - step % 2]
                s = nodeset(nodes, distinct=len(set(nodes)) == len(nodes))
                with forced(c, setting):
                    got, st = run(P, c, oracle, s, setting, f"launch {step} ({what}, {setting})")
                    assert (got[0][through_x] == (S.PRESENT if has_x else S.MISSING_NODE)).all(), (step, what, setting)
                    assert st[10] <= (0 if s.distinct else 1)  # (the pair: its second copy on the overflow list, or in a second record slot)
                    seen[(st[0] == 3, st[13] & 1)] = seen.get((st[0] == 3, st[13] & 1), 0) + 1
                    epoch = st[13]
                    # nodes but no keys: nothing to do, no launch
                    e = np.zeros(0, np.uint8)
                    P.mpt.verify_nodeset(s.r, np.zeros(0, np.uint32), e, 32, s.blob, s.off, ctx=c)
                    assert c.nodeset_stats()[13] == epoch
                    if step == 5:  # keys but no nodes: a launch (every key's root is missing), and the parity of the rest moves on
                        empty = S.NodeSet(roots, ridx, keys, 32, [])
                        got = P.mpt.verify_nodeset(*empty.astuple(), ctx=c)
                        assert (got[0] == S.MISSING_NODE).all()
                        st = c.nodeset_stats()
                        assert st[13] == epoch + 1 and st[12] == 0 and st[1:11] == [0] * 10
                step += 1
    finally:
        c.close()
    assert all(seen.get((lists, parity), 0) >= 2 for lists in (False, True) for parity in (0, 1)), seen


@pytest.mark.parametrize("setting", BOTH)
def test_verdict_counters(P, ctx, oracle, setting):
    """phant_mpt_verify_nodeset_verdict_dev: the failures per root, counted by the walk into a buffer the launch itself clears."""
    import torch
    from tests.witness_util import random_kv
    rng = np.random.default_rng(88)
    n_roots = 5
    tries, keys, ridx, nodes = [], [], [], []
    for t in range(n_roots):
        k, v = random_kv(rng, 40, 32, 1, 90)
        tr = oracle.Trie(k, v)
        tries.append(tr)
        ask = k[:25] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(5)]
        keys += ask
        ridx += [t] * len(ask)
        nodes += [nd for q in ask for nd in tr.prove(q)]
    nodes = list(dict.fromkeys(nodes))
    drop = set(int(i) for i in rng.permutation(len(nodes))[: len(nodes) // 6])  # (their keys: MISSING_NODE)
    nodes = [nd for i, nd in enumerate(nodes) if i not in drop]
    nodes = [nodes[i] for i in rng.permutation(len(nodes))]
    ridx = np.array(ridx, np.uint32)
    order = rng.permutation(len(keys))
    keys, ridx = [keys[i] for i in order], ridx[order]
    ridx_bad = ridx.copy()
    ridx_bad[[3, 50, 97]] = [n_roots, 1 << 31, (1 << 32) - 1]  # BAD_INPUT, counted against root 0
    roots = np.frombuffer(b"".join(t.root() for t in tries), np.uint8).copy()
    blob = np.frombuffer(b"".join(nodes), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(x) for x in nodes])]).astype(np.uint64)
    karr = np.frombuffer(b"".join(keys), np.uint8).copy()
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    d_blob, d_off, d_keys = dev(blob), dev(off.astype(np.int64)), dev(karr.reshape(-1, 32))
    with forced(ctx, setting):
        for what, r, ri in (("five roots", roots, ridx), ("five roots, indices out of range", roots, ridx_bad),
                            ("one root, root_idx of zeros", roots[:32], np.zeros(len(keys), np.uint32)), ("one root, no root_idx", roots[:32], None)):
            want = oracle.mpt_verify_nodeset_checked(r, np.zeros(len(keys), np.uint32) if ri is None else ri, karr, 32, blob, off)
            nr = r.size // 32
            failed = ~np.isin(want[0], (S.PRESENT, S.ABSENT))
            rr = np.zeros(len(keys), np.int64) if ri is None else np.where(ri < nr, ri, 0).astype(np.int64)
            counts = np.bincount(rr[failed], minlength=nr)
            assert counts.sum() > 0 and (ri is not ridx_bad or (want[0][[3, 50, 97]] == S.BAD_INPUT).all())
            fc = dev(np.full(nr, 777, np.int32))
            vo, vl = dev(np.zeros(len(keys), np.int64)), dev(np.zeros(len(keys), np.int32))
            st = P.mpt.verify_nodeset_dev(dev(r), None if ri is None else dev(ri.view(np.int32)), d_keys, d_blob,
                                          d_off, ctx=ctx, value_off=vo, value_len=vl, fail_count=fc)
            ctx.sync()
            assert np.array_equal(st.cpu().numpy(), want[0]), what
            assert np.array_equal(vo.cpu().numpy().view(np.uint64), want[1]) and np.array_equal(vl.cpu().numpy().view(np.uint32), want[2]), what
            assert fc.cpu().numpy().tolist() == counts.tolist(), (what, setting, fc.cpu().numpy().tolist(), counts.tolist())
            stats = ctx.nodeset_stats()
            assert stats[0] == (3 if setting == "lists" else 1 if len(nodes) <= 512 else 2) and stats[12] == len(nodes)


@pytest.mark.parametrize("setting", BOTH)
def test_deep_chains_and_key_lengths(P, ctx, oracle, setting):
    """The walk's state machine beyond 16 nibbles in registers, with keys that are not in LDS (40 bytes), shorter than the eight
    bytes it preloads, and used up at a canonical full branch."""
    with forced(ctx, setting):
        for depth, key_len, end in S.DEEP_CHAINS:
            s = S.deep_chain(oracle, depth, key_len, end=end)
            got, _ = run(P, ctx, oracle, s, setting, f"chain of {depth} branches, {key_len}-byte keys, ends in a {end}, under {setting}", STATS_TABLE)
            assert got[0].tolist() == s.facts["expected"]
