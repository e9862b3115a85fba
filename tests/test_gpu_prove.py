"""Witness generation (phant_mpt_prove_nodeset): the HIP prover behind the trie hasher against the oracle's prover -- set equality of
node bytes, exact counts, roots and statuses -- and round trips through the library's own node-set verifier.  Every comparison is
exact.  (tests/test_emu_prove.py runs the same bodies on the emulated library.)"""
import ctypes as C

import numpy as np
import pytest

from tests import golden, poststate_ref as Q, prestate_ref as R, prove_ref, suite
from tests.witness_util import random_kv

pytestmark = pytest.mark.gpu

EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")


@pytest.fixture(scope="module")
def M():
    import phant_amd
    return phant_amd.mpt


def _ctx():
    from phant_amd.context import default_context
    return default_context()


def _small_default():
    """the bound of the two-launch build pass as the context came: the library's own on the GPU, the emulated suite's on the CPU"""
    return -1 if (suite.FULL or not suite.EMULATED) else 300


@pytest.fixture(params=["small_pass_default", "general_pass_only"])
def build_pass(request):
    _ctx().diag_set("trie_small_max_keys", _small_default() if request.param == "small_pass_default" else 0)
    yield request.param
    _ctx().diag_set("trie_small_max_keys", _small_default())


def _kv(M, keys, vals):
    return [M.KeyVal(k, v) for k, v in zip(keys, vals)]


def _shape(name, rng):
    """-> sorted (keys, vals)"""
    if name.startswith("golden"):
        v = golden.mpt_vectors()[int(name[6:])]
        kv = sorted(zip([bytes.fromhex(k) for k in v["keys"]], [bytes.fromhex(x) for x in v["values"]]))
        return [k for k, _ in kv], [x for _, x in kv]
    if name.startswith("random"):
        n = int(name[6:])
        if n == 5000:
            n = suite.scale(5000, 700)
        return random_kv(rng, n, 32, 1, 80)
    if name == "short_keys_embedded":  # keys of 1 .. 4 bytes, 1-byte values: most nodes are under 32 bytes and live in their parents
        ks = sorted({bytes(rng.integers(0, 256, int(rng.integers(1, 5)), dtype=np.uint8)) for _ in range(220)})
        return ks, [bytes([int(rng.integers(1, 128))]) for _ in ks]
    if name == "prefix_keys":  # keys that are proper prefixes of others: branch values
        base = bytes(rng.integers(0, 256, 6, dtype=np.uint8))
        ks = sorted({base[:2], base[:3], base[:4], base, base[:3] + b"\x01\x02", base[:2] + b"\xff" * 30, base + b"\x00" * 26,
                     base + b"\x10" * 26, b"\x00", b"\x00\x00"})
        return ks, [bytes(rng.integers(1, 256, int(rng.integers(1, 60)), dtype=np.uint8)) for _ in ks]
    if name == "share63":  # two keys sharing 63 nibbles: one long extension at the root
        a = bytes(rng.integers(0, 256, 31, dtype=np.uint8))
        return [a + b"\x50", a + b"\x5f"], [b"x" * 40, b"y" * 3]
    raise KeyError(name)


SHAPES = [f"golden{i}" for i in range(7)] + ["random1", "random2", "random3", "random17", "random300", "random5000",
                                              "short_keys_embedded", "prefix_keys", "share63"]


def _check_trie(M, oracle, keys, vals, queries, got, t=0, flags=None):
    trie = oracle.Trie(keys, vals)
    want = prove_ref.oracle_union(trie, queries) if keys else set()
    if flags is not None and keys:
        want |= prove_ref.sibling_nodes(oracle, trie, keys, queries, flags)
    nodes = got.trie_nodes(t)
    assert set(nodes) == want
    assert len(nodes) == len(want)  # every position once
    assert got.roots[t].tobytes() == (oracle.mptize(keys, vals) if keys else EMPTY_ROOT)
    return want


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_parity(M, oracle, shape, build_pass):
    rng = np.random.default_rng(sum(map(ord, shape)))
    keys, vals = _shape(shape, rng)
    queries = prove_ref.query_list(keys, rng)
    got = M.prove_nodeset(_kv(M, keys, vals), queries)
    want = _check_trie(M, oracle, keys, vals, queries, got)
    assert got.total_nodes == len(want)
    assert np.array_equal(got.q_status, prove_ref.statuses(keys, queries))
    assert int(got.trie_first_node[0]) == 0 and int(got.trie_first_node[1]) == got.total_nodes
    # the oracle's verifier over the oracle's proof says the same
    trie = oracle.Trie(keys, vals)
    for j in range(0, len(queries), max(1, len(queries) // 40)):
        st, _ = oracle.mpt_verify(trie.root(), queries[j], trie.prove(queries[j]))
        assert st == got.q_status[j]


def _forest(rng, n_tries=40):
    tries = []
    for t in range(n_tries):
        n = 0 if t in (3, 17, 39) else int(rng.integers(1, suite.scale(201, 60)))
        tries.append(random_kv(rng, n, 32, 1, 70) if n else ([], []))
    tries[11] = tries[5]  # two byte-identical tries
    return tries


def test_forests(M, oracle):
    rng = np.random.default_rng(40)
    tries = _forest(rng)
    keys = [k for ks, _ in tries for k in ks]
    vals = [v for _, vs in tries for v in vs]
    seg = np.cumsum([0] + [len(ks) for ks, _ in tries]).astype(np.uint32)
    per_trie, queries, q_trie = {}, [], []
    for t, (ks, _) in enumerate(tries):
        if t in (7, 20):  # no queries
            continue
        qs = (list(ks[::3]) + prove_ref.absent_queries(ks, rng, many=4)[:12]) if ks else [b"\x12" * 32, b""]
        if t == 11:
            qs = list(per_trie[5])  # the identical tries are asked the same: their node lists must then be equal
        per_trie[t] = qs
        queries += qs
        q_trie += [t] * len(qs)
    order = rng.permutation(len(queries))
    queries, q_trie = [queries[int(i)] for i in order], np.array([q_trie[int(i)] for i in order], np.uint32)
    got = M.prove_nodeset(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    total = 0
    for t, (ks, vs) in enumerate(tries):
        want = _check_trie(M, oracle, ks, vs, per_trie.get(t, []), got, t)
        if not ks or t not in per_trie:
            assert not want and got.trie_first_node[t] == got.trie_first_node[t + 1]
        total += len(want)
    assert got.total_nodes == total and int(got.trie_first_node[0]) == 0 and int(got.trie_first_node[-1]) == total
    assert got.trie_nodes(5) == got.trie_nodes(11) and got.trie_nodes(5)  # the identical tries both have their nodes
    for j, q in enumerate(queries):
        assert got.q_status[j] == (prove_ref.PRESENT if q in set(tries[int(q_trie[j])][0]) else prove_ref.ABSENT)


def _verify(M, got, queries, q_trie, order=None):
    """the emitted set (its nodes in `order`) through phant_mpt_verify_nodeset under the emitted roots"""
    idx = list(range(got.total_nodes)) if order is None else list(order)
    nodes = [got.node(j) for j in idx]
    off = np.zeros(len(nodes) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in nodes])
    blob = np.frombuffer(b"".join(nodes), np.uint8) if nodes else np.zeros(0, np.uint8)
    karr = np.frombuffer(b"".join(queries), np.uint8)
    st, vo, vl = M.verify_nodeset(got.roots.reshape(-1), q_trie, karr, 32, blob, off)
    return st, vo, vl, blob


def test_round_trip_through_the_verifier(M, oracle):
    rng = np.random.default_rng(3)
    n = suite.scale(300, 40)
    tries = [random_kv(rng, n, 32, 1, 80), random_kv(rng, 25, 32, 1, 80), ([], [])]
    keys = [k for ks, _ in tries for k in ks]
    vals = [v for _, vs in tries for v in vs]
    seg = np.cumsum([0] + [len(ks) for ks, _ in tries]).astype(np.uint32)
    queries, q_trie = [], []
    for t, (ks, _) in enumerate(tries):
        qs = list(ks) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(30)]
        queries += qs
        q_trie += [t] * len(qs)
    q_trie = np.array(q_trie, np.uint32)
    got = M.prove_nodeset(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    st, vo, vl, blob = _verify(M, got, queries, q_trie, rng.permutation(got.total_nodes))
    assert np.array_equal(st, got.q_status)
    value_of = [dict(zip(ks, vs)) for ks, vs in tries]
    for j, q in enumerate(queries):
        if st[j] == M.PROOF_PRESENT:
            assert blob[int(vo[j]):int(vo[j]) + int(vl[j])].tobytes() == value_of[int(q_trie[j])][q]
    assert (st == M.PROOF_PRESENT).sum() == len(keys)
    # minimality: without any one of its nodes the set no longer proves every query
    for drop in range(got.total_nodes):
        st2, _, _, _ = _verify(M, got, queries, q_trie, [j for j in range(got.total_nodes) if j != drop])
        assert (st2 == M.PROOF_MISSING_NODE).any(), drop


def _raw(M, L, ctx, keys, vals, queries, seg=None, q_trie=None, q_flags=None, max_nodes=4096, nodes_cap=1 << 20, null=(),
         struct_size=None, n_tries=None):
    """the C call itself -> (rc, out struct, buffers)"""
    from phant_amd.context import _np_ptr
    kb, ko = M._pack(list(keys), np.uint32)
    vb, vo = M._pack(list(vals), np.uint64)
    qb, qo = M._pack(list(queries), np.uint32)
    nt = n_tries if n_tries is not None else (1 if seg is None else len(seg) - 1)
    buf = {"nodes": np.full(max(nodes_cap, 1), 0xEE, np.uint8), "node_off": np.full(max_nodes + 1, 0xEEEEEEEE, np.uint64),
           "trie_first_node": np.full(nt + 1, 0xEEEEEEEE, np.uint32), "roots": np.full(32 * max(nt, 1), 0xEE, np.uint8),
           "q_status": np.full(max(len(queries), 1), 0xEE, np.uint8)}
    p = {k: (None if k in null else _np_ptr(v)) for k, v in buf.items()}
    o = L.PhantProveOut(C.sizeof(L.PhantProveOut) if struct_size is None else struct_size, max_nodes, nodes_cap, p["nodes"], p["node_off"],
                        p["trie_first_node"], p["roots"], p["q_status"], 0, 0, 0)
    seg_a = None if seg is None else np.ascontiguousarray(seg, np.uint32)
    qt = None if q_trie is None else np.ascontiguousarray(q_trie, np.uint32)
    qf = None if q_flags is None else np.ascontiguousarray(q_flags, np.uint8)
    rc = ctx._lib.phant_mpt_prove_nodeset(ctx.handle, _np_ptr(kb), _np_ptr(ko), _np_ptr(vb), _np_ptr(vo), len(keys),
                                          None if seg_a is None else _np_ptr(seg_a), nt, _np_ptr(qb), _np_ptr(qo),
                                          None if qt is None else _np_ptr(qt), None if qf is None else _np_ptr(qf), len(queries), C.byref(o))
    return rc, o, buf


def test_capacity_and_arguments(M, oracle):
    from phant_amd import _lib as L
    ctx = _ctx()
    rng = np.random.default_rng(11)
    keys, vals = random_kv(rng, 60, 32, 1, 80)
    queries = list(keys[::2]) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(10)]
    rc, o, full = _raw(M, L, ctx, keys, vals, queries)
    assert rc == 0 and o.total_nodes > 0
    tn, nl = int(o.total_nodes), int(o.nodes_len)
    want = prove_ref.oracle_union(oracle.Trie(keys, vals), queries)
    emitted = lambda b: {b["nodes"][int(b["node_off"][j]):int(b["node_off"][j + 1])].tobytes() for j in range(tn)}  # noqa: E731
    assert emitted(full) == want and len(want) == tn and int(full["node_off"][tn]) == nl
    # one too small, either way: OK, exact counts, nothing written; the counts then suffice
    for mn, nc in ((tn - 1, nl), (tn, nl - 1)):
        rc, o, b = _raw(M, L, ctx, keys, vals, queries, max_nodes=mn, nodes_cap=nc)
        assert rc == 0 and (o.total_nodes, o.nodes_len) == (tn, nl)
        assert (b["nodes"] == 0xEE).all() and (b["node_off"] == 0xEEEEEEEE).all()
        assert np.array_equal(b["q_status"], full["q_status"]) and np.array_equal(b["roots"], full["roots"])
    rc, o, b = _raw(M, L, ctx, keys, vals, queries, max_nodes=tn, nodes_cap=nl)
    assert rc == 0 and emitted(b) == want
    assert np.array_equal(b["nodes"][:nl], full["nodes"][:nl])  # the same input twice: identical bytes
    # each output pointer NULL in turn
    for name in ("nodes", "node_off", "trie_first_node", "roots", "q_status"):
        rc, o, b = _raw(M, L, ctx, keys, vals, queries, null=(name,))
        assert rc == 0 and (o.total_nodes, o.nodes_len) == (tn, nl), name
        for other in ("trie_first_node", "roots", "q_status"):
            if other != name:
                assert np.array_equal(b[other], full[other]), (name, other)
        if name == "nodes":
            assert np.array_equal(b["node_off"][:tn + 1], full["node_off"][:tn + 1])
        if name == "node_off":
            assert np.array_equal(b["nodes"][:nl], full["nodes"][:nl])
    # no queries; no keys
    rc, o, b = _raw(M, L, ctx, keys, vals, [])
    assert rc == 0 and (o.total_nodes, o.nodes_len) == (0, 0) and list(b["trie_first_node"]) == [0, 0]
    assert b["roots"].tobytes() == oracle.mptize(keys, vals) and int(b["node_off"][0]) == 0
    rc, o, b = _raw(M, L, ctx, [], [], [b"\x01" * 32, b""])
    assert rc == 0 and (o.total_nodes, o.nodes_len) == (0, 0) and b["roots"].tobytes() == EMPTY_ROOT
    assert list(b["q_status"]) == [M.PROOF_ABSENT, M.PROOF_ABSENT] and list(b["trie_first_node"]) == [0, 0]
    # refused
    rc, _, _ = _raw(M, L, ctx, [keys[1], keys[0]] + keys[2:], vals, queries)
    assert rc == L.E_UNSORTED
    rc, _, _ = _raw(M, L, ctx, keys, vals, queries, seg=[0, 30, 60], q_trie=[0] * (len(queries) - 1) + [2])
    assert rc == L.E_INVALID_ARG
    for size in (0, C.sizeof(L.PhantProveOut) - 8, C.sizeof(L.PhantProveOut) + 8):
        rc, _, _ = _raw(M, L, ctx, keys, vals, queries, struct_size=size)
        assert rc == L.E_INVALID_ARG
    rc, _, _ = _raw(M, L, ctx, keys, vals, queries, seg=[0, 30, 60], q_trie=None)
    assert rc == L.E_INVALID_ARG


def _raw_dev(M, L, ctx, keys, vals, queries, seg=None, q_trie=None, max_nodes=4096, nodes_cap=1 << 18, null=(), batch=False):
    """the device form's C call itself (batch: phant_mpt_prove_batch_dev), every array in device memory, 0xEE in the outputs
    -> (rc, out struct, the buffers as they are afterwards, in host memory and under the names _raw gives them)"""
    import torch
    kb, ko = M._pack(list(keys), np.uint32)
    vb, vo = M._pack(list(vals), np.uint64)
    qb, qo = M._pack(list(queries), np.uint32)
    n, nq, nt = len(keys), len(queries), 1 if seg is None else len(seg) - 1
    first = "proof_first_node" if batch else "trie_first_node"
    buf = {"nodes": np.full(max(nodes_cap, 1), 0xEE, np.uint8), "node_off": np.full(max_nodes + 1, 0xEEEEEEEE, np.uint64),
           first: np.full((nq if batch else nt) + 1, 0xEEEEEEEE, np.uint32), "roots": np.full(32 * nt, 0xEE, np.uint8),
           "q_status": np.full(max(nq, 1), 0xEE, np.uint8)}
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    ins = [dev(a) for a in (kb, ko, vb, vo, None if seg is None else np.asarray(seg, np.uint32), qb, qo,
                            None if q_trie is None else np.asarray(q_trie, np.uint32))]
    d = {k: dev(v) for k, v in buf.items()}
    p = {k: (None if k in null else ptr(t)) for k, t in d.items()}
    Out = L.PhantProveBatchOut if batch else L.PhantProveOut
    o = Out(C.sizeof(Out), max_nodes, nodes_cap, p["nodes"], p["node_off"], p[first], p["roots"], p["q_status"], 0, 0, 0)
    head = [ctx.handle, ptr(ins[0]), ptr(ins[1]), int(ko[-1]), ptr(ins[2]), ptr(ins[3]), int(vo[-1]), n, ptr(ins[4]), nt, ptr(ins[5]), ptr(ins[6]),
            int(qo[-1]), ptr(ins[7])]
    if batch:
        rc = ctx._lib.phant_mpt_prove_batch_dev(*head, nq, C.byref(o))
    else:
        rc = ctx._lib.phant_mpt_prove_nodeset_dev(*head, None, nq, C.byref(o))
    torch.cuda.synchronize()
    return rc, o, {k: t.cpu().numpy().view(buf[k].dtype).copy() for k, t in d.items()}


def device_form_edge_cases(M, oracle, L, ctx, host, dev, first):
    """The device form of either prover against its host form, call by call on the same arguments: the same code, the same totals and
    the same five buffers to the last 0xEE (`host` / `dev`: the two _raw functions, `first`: the first-node table's name); what the
    host form returns is held to the oracle here or in the host form's own test_capacity_and_arguments.  -> the full call's buffers"""
    rng = np.random.default_rng(12)
    keys, vals = random_kv(rng, 60, 32, 1, 80)
    queries = list(keys[::2]) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(9)] + [b""]
    names = ("nodes", "node_off", first, "roots", "q_status")

    def both(k, v, q, **kw):
        kw.setdefault("nodes_cap", 1 << 18)
        rh, oh, bh = host(M, L, ctx, k, v, q, **kw)
        rd, od, bd = dev(M, L, ctx, k, v, q, **kw)
        assert rd == rh == 0 and (od.total_nodes, od.nodes_len) == (oh.total_nodes, oh.nodes_len), kw
        for name in names:
            assert np.array_equal(bd[name], bh[name]), (name, kw)
        return od, bd

    o, full = both(keys, vals, queries, nodes_cap=1 << 18)
    tn, nl = int(o.total_nodes), int(o.nodes_len)
    assert tn > 0 and int(full["node_off"][tn]) == nl and full["roots"].tobytes() == oracle.mptize(keys, vals)
    assert np.array_equal(full["q_status"], prove_ref.statuses(keys, queries))
    # exact capacity
    o, b = both(keys, vals, queries, max_nodes=tn, nodes_cap=nl)
    assert np.array_equal(b["nodes"], full["nodes"][:nl]) and np.array_equal(b["node_off"], full["node_off"][:tn + 1])
    # one node too few, one byte too few: the totals, the laid-out buffers untouched, roots and q_status still written
    for mn, nc in ((tn - 1, nl), (tn, nl - 1)):
        o, b = both(keys, vals, queries, max_nodes=mn, nodes_cap=nc)
        assert (o.total_nodes, o.nodes_len) == (tn, nl)
        assert (b["nodes"] == 0xEE).all() and (b["node_off"] == 0xEEEEEEEE).all()
        assert first == "trie_first_node" or (b[first] == 0xEEEEEEEE).all()
        assert np.array_equal(b["q_status"], full["q_status"]) and np.array_equal(b["roots"], full["roots"])
    # each output NULL in turn, then all of them
    for null in [(name,) for name in names] + [names]:
        o, b = both(keys, vals, queries, nodes_cap=1 << 18, null=null)
        assert (o.total_nodes, o.nodes_len) == (tn, nl), null
        for name in names:
            if name in null:
                assert (b[name] == (0xEE if b[name].dtype == np.uint8 else 0xEEEEEEEE)).all(), null
            elif first == "proof_first_node" or name in (first, "roots", "q_status"):
                assert np.array_equal(b[name], full[name]), (null, name)
    # no queries; no keys with two queries
    o, b = both(keys, vals, [])
    assert (o.total_nodes, o.nodes_len) == (0, 0) and not b[first].any() and int(b["node_off"][0]) == 0
    assert b["roots"].tobytes() == oracle.mptize(keys, vals) and (b["node_off"][1:] == 0xEEEEEEEE).all()
    o, b = both([], [], [b"\x01" * 32, b""])
    assert (o.total_nodes, o.nodes_len) == (0, 0) and b["roots"].tobytes() == EMPTY_ROOT and not b[first].any()
    assert list(b["q_status"]) == [M.PROOF_ABSENT, M.PROOF_ABSENT] and int(b["node_off"][0]) == 0
    # three tries, the queries all of the empty one
    seg = [0, 30, 30, 60]
    o, b = both(keys, vals, queries, seg=seg, q_trie=[1] * len(queries))
    assert (o.total_nodes, o.nodes_len) == (0, 0) and not b[first].any() and int(b["node_off"][0]) == 0
    assert (b["q_status"] == M.PROOF_ABSENT).all() and (b["nodes"] == 0xEE).all()
    assert b["roots"].tobytes() == oracle.mptize(keys[:30], vals[:30]) + EMPTY_ROOT + oracle.mptize(keys[30:], vals[30:])
    # a q_trie entry that names no trie
    bad = [0] * (len(queries) - 1) + [3]
    assert host(M, L, ctx, keys, vals, queries, seg=seg, q_trie=bad)[0] == L.E_INVALID_ARG
    assert dev(M, L, ctx, keys, vals, queries, seg=seg, q_trie=bad)[0] == L.E_INVALID_ARG
    return tn, full


def test_device_capacity_and_arguments(M, oracle):
    """test_capacity_and_arguments for phant_mpt_prove_nodeset_dev"""
    from phant_amd import _lib as L
    tn, full = device_form_edge_cases(M, oracle, L, _ctx(), _raw, _raw_dev, "trie_first_node")
    assert list(full["trie_first_node"]) == [0, tn]


def test_one_context_small_large_small(M, oracle):
    import phant_amd
    from phant_amd.context import Context, default_context
    rng = np.random.default_rng(21)
    sets = []
    for n in (12, suite.scale(6000, 500), 30):
        keys, vals = random_kv(rng, n, 32, 1, 80)
        sets.append((keys, vals, list(keys[::5]) + prove_ref.absent_queries(keys, rng, many=3)))

    def run(ctx, i):
        keys, vals, q = sets[i]
        g = M.prove_nodeset(_kv(M, keys, vals), q, ctx=ctx)
        return g.nodes.tobytes(), g.node_off.tobytes(), g.roots.tobytes(), g.q_status.tobytes()

    ctx = default_context()
    first = run(ctx, 0)
    assert M.mptize(_kv(M, *sets[1][:2]), ctx=ctx) == oracle.mptize(*sets[1][:2])
    large = run(ctx, 1)
    keys, vals, q = sets[2]
    g = M.prove_nodeset(_kv(M, keys, vals), list(keys))
    st, _, _, _ = _verify(M, g, list(keys), np.zeros(len(keys), np.uint32))
    assert (st == M.PROOF_PRESENT).all()
    again = run(ctx, 0)
    assert first == again
    fresh = type(ctx)() if suite.EMULATED else Context(ctx.device)
    try:
        assert run(fresh, 0) == first and run(fresh, 1) == large
    finally:
        fresh.close()


def _flag_case(M, oracle, keys, vals, queries, flags):
    got = M.prove_nodeset(_kv(M, keys, vals), queries, q_flags=np.array(flags, np.uint8))
    plain = M.prove_nodeset(_kv(M, keys, vals), queries)
    want = _check_trie(M, oracle, keys, vals, queries, got, flags=flags)
    assert got.total_nodes == len(want)
    assert set(plain.trie_nodes(0)) <= set(got.trie_nodes(0)) and np.array_equal(plain.q_status, got.q_status)
    return got, plain


def test_may_remove_adds_the_siblings(M, oracle, build_pass):
    rng = np.random.default_rng(77)
    v = lambda: bytes(rng.integers(1, 256, 40, dtype=np.uint8))  # noqa: E731
    # a branch of two children: the removed leaf, and a hashed sub-trie nobody queries
    a = bytes(rng.integers(0, 256, 30, dtype=np.uint8))
    keys = sorted([b"\x11" + a + b"\x00", b"\x12" + a + b"\x01", b"\x12" + a + b"\x02", b"\x12" + a[:20] + b"\xff" * 11])
    vals = [v() for _ in keys]
    got, plain = _flag_case(M, oracle, keys, vals, [keys[0]], [1])
    assert got.total_nodes == plain.total_nodes + 1
    # ... the same query without the flag, and a flag on a query that is absent, add nothing
    got, plain = _flag_case(M, oracle, keys, vals, [keys[0], b"\x13" + a + b"\x00"], [0, 1])
    assert got.total_nodes == plain.total_nodes
    # the other child is a leaf, on every level of the flagged key's path: the leaf beside it, the leaf beside its sub-trie, the
    # leaf beside that
    got, plain = _flag_case(M, oracle, keys, vals, [keys[1]], [1])
    assert got.total_nodes == plain.total_nodes + 3
    # three children, two sub-trees flagged entirely: the third joins (the cascading case); with only one flagged it does not
    keys3 = sorted(keys + [b"\x13" + a + b"\x05", b"\x13" + a + b"\x06"])
    vals3 = [v() for _ in keys3]
    in1 = [k for k in keys3 if k[0] == 0x11]
    in3 = [k for k in keys3 if k[0] == 0x13]
    got, plain = _flag_case(M, oracle, keys3, vals3, in1 + in3, [1] * (len(in1) + len(in3)))
    assert got.total_nodes == plain.total_nodes + 1
    got, plain = _flag_case(M, oracle, keys3, vals3, in1 + in3, [1] * len(in1) + [0] * len(in3))
    assert got.total_nodes == plain.total_nodes
    # the surviving position is the branch's value, or an embedded child: nothing to add
    pk = [b"\x20", b"\x20\x01" + a, b"\x55"]
    got, plain = _flag_case(M, oracle, pk, [v(), v(), v()], [pk[1]], [1])
    sk = [b"\x31", b"\x32"]
    got, plain = _flag_case(M, oracle, sk, [b"\x01", b"\x02"], [sk[0]], [1])
    assert got.total_nodes == plain.total_nodes == 1
    # random tries: flags on every stored key leave nothing outside the masks; flags on a few match the rule's own reference
    keys, vals = random_kv(rng, suite.scale(300, 120), 32, 1, 80)
    got, plain = _flag_case(M, oracle, keys, vals, list(keys), [1] * len(keys))
    assert got.total_nodes == plain.total_nodes
    some = [keys[int(i)] for i in rng.choice(len(keys), 25, replace=False)] + prove_ref.absent_queries(keys, rng, many=3)[:10]
    flags = [int(rng.integers(0, 2)) for _ in some]
    _flag_case(M, oracle, keys, vals, some, flags)
    ks, vs = _shape("short_keys_embedded", rng)
    some = [ks[int(i)] for i in rng.choice(len(ks), 40, replace=False)]
    _flag_case(M, oracle, ks, vs, some, [1] * len(some))


def test_device_form(M, oracle):
    import torch
    rng = np.random.default_rng(5)
    keys, vals = random_kv(rng, suite.scale(3000, 350), 32, 1, 80)
    queries = list(keys[::7]) + prove_ref.absent_queries(keys, rng, many=5)
    host = M.prove_nodeset(_kv(M, keys, vals), queries)
    kb, ko = M._pack(keys, np.uint32)
    vb, vo = M._pack(vals, np.uint64)
    qb, qo = M._pack(queries, np.uint32)
    dev = lambda a, dt: torch.from_numpy(a.astype(dt)).cuda()  # noqa: E731
    d = [dev(kb, np.uint8), dev(ko, np.int32), dev(vb, np.uint8), dev(vo, np.int64)]
    dq = [dev(qb, np.uint8), dev(qo, np.int32)]
    tn, nl = M.prove_nodeset_dev(*d, None, *dq, None, None, None, None)
    assert (tn, nl) == (host.total_nodes, len(host.nodes))
    nodes, off = torch.zeros(nl, dtype=torch.uint8).cuda(), torch.zeros(tn + 1, dtype=torch.int64).cuda()
    first, roots, st = torch.zeros(2, dtype=torch.int32).cuda(), torch.zeros(32, dtype=torch.uint8).cuda(), torch.zeros(len(queries), dtype=torch.uint8).cuda()
    assert M.prove_nodeset_dev(*d, None, *dq, None, None, nodes, off, first, roots, st) == (tn, nl)
    torch.cuda.synchronize()
    assert nodes.cpu().numpy().tobytes() == host.nodes.tobytes() and off.cpu().numpy().astype(np.uint64).tobytes() == host.node_off.tobytes()
    assert roots.cpu().numpy().tobytes() == host.roots.tobytes() and np.array_equal(st.cpu().numpy(), host.q_status)
    assert list(first.cpu().numpy()) == [0, tn]
    bad = dev(np.array([0] * (len(queries) - 1) + [1], np.uint32), np.int32)
    from phant_amd import _lib as L
    with pytest.raises(L.PhantError) as e:
        M.prove_nodeset_dev(*d, None, *dq, bad, None, None, None)
    assert e.value.code == L.E_INVALID_ARG


# ---------------------------------------------------------------- 5. phant_state_witness: state + touched keys -> a witness
@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _slot_key(addr, s):
    return addr + int(s).to_bytes(32, "big")


def _expected_state_nodes(oracle, accounts, keys):
    """the node set the oracle's prover cuts for `keys`: -> (set of node bytes, number of node positions, state root)"""
    state, _, storage = R.build_tries(oracle, accounts)
    index = {a["addr"]: i for i, a in enumerate(accounts)}
    per_trie = {}
    for k in keys:
        per_trie.setdefault("state", set()).update(state.prove(oracle.keccak256(k[:20])))
        i = index.get(k[:20])
        if len(k) == 52 and i in storage:
            per_trie.setdefault(i, set()).update(storage[i][0].prove(oracle.keccak256(k[20:])))
    return set().union(*per_trie.values()) if per_trie else set(), sum(len(x) for x in per_trie.values()), state.root()


def _nodes_of(info):
    b, off = info["nodes"].tobytes(), info["node_off"]
    return [b[int(off[j]):int(off[j + 1])] for j in range(info["total_nodes"])]


def _info_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _state_witness_case(P, oracle, accounts, keys, fixture_root=None):
    S = P.stateless
    w = S.build_witness(accounts, keys)
    try:
        info = w.info()
        want_set, want_count, want_root = _expected_state_nodes(oracle, accounts, keys)
        assert w.state_root == want_root == P.state.state_root(accounts)
        if fixture_root is not None:
            assert w.state_root.hex() == fixture_root
        nodes = _nodes_of(info)
        assert set(nodes) == want_set and len(nodes) == want_count
        pre = w.prestate(None, w.state_root)
        assert (pre.n_failed, pre.n_missing_code, pre.n_unused_codes) == (0, 0, 0)
        # the resolved accounts, slot values and codes are exactly the touched part of the input state
        by = {a["addr"]: a for a in accounts}
        touched, slots = list(dict.fromkeys(k[:20] for k in keys)), {}
        for k in keys:
            if len(k) == 52:
                slots.setdefault(k[:20], set()).add(int.from_bytes(k[20:], "big"))
        assert pre.addresses == touched
        assert pre.absent == [a for a in touched if a not in by]
        assert [a.addr for a in pre.accounts] == [a for a in touched if a in by]
        for got in pre.accounts:
            a = by[got.addr]
            assert (got.nonce, got.balance, got.code) == (a["nonce"], a["balance"], bytes(a["code"]))
            assert got.storage == {s: int(a["storage"][s]) for s in slots.get(got.addr, ()) if int(a["storage"].get(s, 0))}
        assert info["n_codes"] == len({bytes(by[a]["code"]) for a in touched if a in by and by[a]["code"]})
        # to_json -> parse_json: the same object
        text = w.to_json()
        back = S.StatelessWitness.parse_json(text)
        try:
            _info_equal(info, back.info())
        finally:
            back.close()
        # an account nobody touched is not resolvable from this witness (its leaf is a hashed node no path of the set ends in)
        other = next((a["addr"] for a in accounts if a["addr"] not in touched), None)
        if other is not None:
            import json
            doc = json.loads(text)
            doc["keys"].append("0x" + other.hex())
            more = S.StatelessWitness.parse_json(json.dumps(doc))
            try:
                r = more.prestate_arrays(None, w.state_root)
                assert r["n_failed"] == 1 and r["account_status"][-1] not in (Q.PRESENT, Q.ABSENT)
            finally:
                more.close()
    finally:
        w.close()


def test_state_witness_of_every_fixture_alloc(P, oracle):
    fx = golden.fixtures()
    cases = fx["cases"][:suite.scale(len(fx["cases"]), 6)]
    rng = np.random.default_rng(61)
    for c in cases:
        accounts = golden.accounts_of(c["pre"], fx["codes"])
        keys = []
        for a in accounts:
            keys.append(a["addr"])
            keys += [_slot_key(a["addr"], s) for s in a["storage"]]
            keys.append(_slot_key(a["addr"], int(rng.integers(1 << 40, 1 << 62))))  # a slot it does not have
        ghost = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
        keys += [ghost, _slot_key(ghost, 1), keys[0]]  # an address the state does not hold, a slot under it, a duplicate
        _state_witness_case(P, oracle, accounts, keys, c["genesis_state_root"])
        if len(accounts) > 1:  # ... and a witness of one account only: the others stay unresolvable
            _state_witness_case(P, oracle, accounts, keys[:1], c["genesis_state_root"])


def test_state_witness_of_a_block_shaped_state(P, oracle):
    rng = np.random.default_rng(62)
    doc, root, accounts = R.block_witness_doc(oracle, rng, n_accounts=suite.scale(1500, 160), n_contracts=suite.scale(40, 8),
                                              max_slots=suite.scale(60, 12), n_touched=suite.scale(300, 40), n_absent=suite.scale(30, 6))
    keys = [bytes.fromhex(k[2:]) for k in doc["keys"]]
    for a in accounts[:5]:  # zero-valued slots: in the state's arrays, not in the trie, and touched
        for _ in range(3):
            s = int(rng.integers(1 << 62, 1 << 63))
            a["storage"][s] = 0
            keys += [a["addr"], _slot_key(a["addr"], s)]
    assert P.state.state_root(accounts) == root
    _state_witness_case(P, oracle, accounts, keys)


def test_state_witness_arguments(P, oracle):
    from phant_amd import _lib as L
    S = P.stateless
    rng = np.random.default_rng(63)
    accounts = [{"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": 1, "balance": 2, "code": b"", "storage": {}} for _ in range(5)]
    for bad in (b"\x01" * 32, b"\x01" * 19, b"", b"\x01" * 53):
        with pytest.raises(L.PhantError) as e:
            S.build_witness(accounts, [accounts[0]["addr"], bad])
        assert e.value.code == L.E_INVALID_ARG and "key 1" in str(e.value)
    w = S.build_witness(accounts, [])  # no keys: a witness without nodes, the root all the same
    assert w.info()["total_nodes"] == 0 and w.info()["n_accounts"] == 0 and w.state_root == P.state.state_root(accounts)
    w.close()
    w = S.build_witness([], [accounts[0]["addr"]])  # the empty state: every key absent under the empty root
    assert w.state_root == EMPTY_ROOT and w.info()["total_nodes"] == 0
    pre = w.prestate(None, w.state_root)
    assert pre.n_failed == 0 and pre.absent == [accounts[0]["addr"]]
    w.close()


# ---------------------------------------------------------------- 6. removals: the flagged witness against its one consumer
def _addr_with_prefix(oracle, want, start):
    i = start
    while not oracle.keccak256(i.to_bytes(20, "big")).hex().startswith(want):
        i += 1
    return i.to_bytes(20, "big")


def _slots_with_prefixes(oracle, prefixes):
    out, s = [], 0
    for pfx in prefixes:
        while not oracle.keccak256(s.to_bytes(32, "big")).hex().startswith(pfx):
            s += 1
        out.append(s)
        s += 1
    return out


def _removal_case(P, oracle, accounts, writes, keys, extra_nodes):
    """The witness of `keys` alone is too thin to re-root after `writes`; with every key flagged it carries exactly `extra_nodes`
    more nodes and phant_exec_witness_poststate gives the root of the post state."""
    S = P.stateless
    after = Q.apply_writes(accounts, writes)
    thin, full = S.build_witness(accounts, keys), S.build_witness(accounts, keys, may_remove=keys)
    try:
        info = thin.info()
        got = thin.poststate_arrays(None, thin.state_root, Q.write_arrays(oracle, info, writes))
        st = list(got["account_status"]) + list(got["slot_status"])
        assert got["n_failed"] >= 1 and Q.MISSING_SIBLING in st and set(st) <= {Q.PRESENT, Q.MISSING_SIBLING}, st
        assert got["state_root"] == bytes(32)
        info = full.info()
        assert full.state_root == thin.state_root
        assert set(_nodes_of(thin.info())) <= set(_nodes_of(info)) and info["total_nodes"] == thin.info()["total_nodes"] + extra_nodes
        got = full.poststate_arrays(None, full.state_root, Q.write_arrays(oracle, info, writes))
        want = Q.expected(oracle, info, accounts, writes)
        assert got["n_failed"] == 0, (got["account_status"], got["slot_status"])
        assert got["state_root"] == want["state_root"] == (P.state.state_root(after) if after else EMPTY_ROOT)
        for k in ("storage_roots", "account_status", "slot_status"):
            assert np.array_equal(got[k], want[k]), k
    finally:
        thin.close()
        full.close()


def _accounts_at(oracle, prefixes, rng, start=1):
    return [{"addr": _addr_with_prefix(oracle, pfx, start + 1_000_000 * j), "nonce": int(rng.integers(0, 1000)),
             "balance": int(rng.integers(1, 1 << 62)), "code": b"", "storage": {}} for j, pfx in enumerate(prefixes)]


def test_removals_need_the_flag_and_the_flag_suffices(P, oracle):
    rng = np.random.default_rng(64)
    # the state trie: the removed account's branch has two children, the other a hashed BRANCH on no touched path
    acc = _accounts_at(oracle, ["1", "73", "79"], rng)
    _removal_case(P, oracle, acc, {acc[0]["addr"]: None}, [acc[0]["addr"]], 1)
    # ... the other an EXTENSION over a branch: the extension alone joins, the branch under it is known to be one
    acc = _accounts_at(oracle, ["1", "7c3", "7c9"], rng)
    _removal_case(P, oracle, acc, {acc[0]["addr"]: None}, [acc[0]["addr"]], 1)
    # ... the other a LEAF, under an extension: the root becomes that leaf
    acc = _accounts_at(oracle, ["ab1", "ab2"], rng)
    _removal_case(P, oracle, acc, {acc[0]["addr"]: None}, [acc[0]["addr"]], 1)
    # cascading: a branch of three children, two sub-trees removed entirely (a leaf, and a branch of two leaves)
    acc = _accounts_at(oracle, ["1", "2a", "2b", "73", "79"], rng)
    gone = [a["addr"] for a in acc[:3]]
    _removal_case(P, oracle, acc, {a: None for a in gone}, gone, 1)
    # the same shapes in a storage trie, beside other accounts
    for prefixes, n_gone in ((["1", "73", "79"], 1), (["1", "7c3", "7c9"], 1), (["1", "2a", "2b", "73", "79"], 3)):
        slots = _slots_with_prefixes(oracle, prefixes)
        owner = {"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": 1, "balance": 1, "code": b"\x60\x00",
                 "storage": {s: 7 + s for s in slots}}
        acc = [owner] + _accounts_at(oracle, ["0", "f"], rng)
        keys = [_slot_key(owner["addr"], s) for s in slots[:n_gone]]
        _removal_case(P, oracle, acc, {owner["addr"]: ("keep", {s: 0 for s in slots[:n_gone]})}, keys, 1)
