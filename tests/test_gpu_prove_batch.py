"""Per-proof witness generation (phant_mpt_prove_batch): the ordered node list per query, root first -- the eth_getProof shape --
against the oracle's prover, list by list; against the node-set form; and through the library's own per-proof verifier.  Every
comparison is exact.  (tests/test_emu_prove_batch.py runs the same bodies on the emulated library.)"""
import ctypes as C
import json

import numpy as np
import pytest

from tests import golden, prestate_ref as R, prove_ref, suite
from tests.test_gpu_prove import EMPTY_ROOT, SHAPES, M, _ctx, _forest, _kv, _shape, build_pass  # noqa: F401
from tests.witness_util import random_kv

pytestmark = pytest.mark.gpu


def _check_lists(oracle, trie, keys, queries, got, first_query=0):
    """proof j of `got` == the oracle's list for query j, for every query -> (nodes, bytes) of all of them"""
    nodes = size = 0
    for j, q in enumerate(queries, first_query):
        want = trie.prove(q) if keys else []
        assert got.proof(j) == want, (j, q.hex())
        nodes += len(want)
        size += sum(len(x) for x in want)
    return nodes, size


def _check_layout(got, n_queries):
    assert len(got.proof_first_node) == n_queries + 1 and int(got.proof_first_node[0]) == 0
    assert int(got.proof_first_node[-1]) == got.total_nodes
    assert (np.diff(got.proof_first_node.astype(np.int64)) >= 0).all()
    assert int(got.node_off[0]) == 0 and int(got.node_off[-1]) == len(got.nodes)
    assert (np.diff(got.node_off.astype(np.int64)) > 0).all()  # contiguous from 0, no empty node


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_parity(M, oracle, shape, build_pass):
    rng = np.random.default_rng(sum(map(ord, shape)))
    keys, vals = _shape(shape, rng)
    queries = prove_ref.query_list(keys, rng)
    got = M.prove_batch(_kv(M, keys, vals), queries)
    trie = oracle.Trie(keys, vals)
    nodes, size = _check_lists(oracle, trie, keys, queries, got)
    assert (got.total_nodes, len(got.nodes)) == (nodes, size)
    _check_layout(got, len(queries))
    assert np.array_equal(got.q_status, prove_ref.statuses(keys, queries))
    assert got.roots[0].tobytes() == (oracle.mptize(keys, vals) if keys else EMPTY_ROOT)
    # queries of every length: the oracle's verifier over the emitted list of every query
    value_of = dict(zip(keys, vals))
    root = got.roots[0].tobytes()
    for j, q in enumerate(queries):
        st, val = oracle.mpt_verify(root, q, got.proof(j))
        assert st == got.q_status[j] and (val == value_of[q] if st == prove_ref.PRESENT else val is None), j
    # a shape of 32-byte keys: the proofs of all its 32-byte queries go unchanged into both batch verifiers
    if keys and all(len(k) == 32 for k in keys):
        q32 = [q for q in queries if len(q) == 32]
        assert len(q32) >= 2 * len(keys)
        g = M.prove_batch(_kv(M, keys, vals), q32)
        at = {}
        for j, q in enumerate(queries):
            at.setdefault(q, j)
        assert all(g.proof(i) == got.proof(at[q]) for i, q in enumerate(q32))
        karr = np.frombuffer(b"".join(q32), np.uint8)
        for verify in (M.verify_batch, oracle.mpt_verify_batch):
            st, vo, vl = verify(g.roots.reshape(-1), None, karr, 32, g.nodes, g.node_off, g.proof_first_node)
            assert np.array_equal(st[:len(q32)], g.q_status) and np.array_equal(g.q_status, prove_ref.statuses(keys, q32))
            for i, q in enumerate(q32):
                if st[i] == M.PROOF_PRESENT:
                    assert g.nodes[int(vo[i]):int(vo[i]) + int(vl[i])].tobytes() == value_of[q], i


def _forest_case(rng):
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
            qs = list(per_trie[5])  # the identical tries are asked the same
        per_trie[t] = qs
        queries += qs
        q_trie += [t] * len(qs)
    order = rng.permutation(len(queries))
    return tries, keys, vals, seg, per_trie, [queries[int(i)] for i in order], np.array([q_trie[int(i)] for i in order], np.uint32)


def test_forests(M, oracle):
    tries, keys, vals, seg, per_trie, queries, q_trie = _forest_case(np.random.default_rng(40))
    got = M.prove_batch(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    oracles = [oracle.Trie(ks, vs) if ks else None for ks, vs in tries]
    nodes = 0
    for j, q in enumerate(queries):
        t = int(q_trie[j])
        want = oracles[t].prove(q) if oracles[t] else []
        assert got.proof(j) == want, j
        assert got.q_status[j] == (prove_ref.PRESENT if q in set(tries[t][0]) else prove_ref.ABSENT)
        nodes += len(want)
    assert got.total_nodes == nodes
    _check_layout(got, len(queries))
    for t, (ks, vs) in enumerate(tries):  # every trie's root, queried or not
        assert got.roots[t].tobytes() == (oracle.mptize(ks, vs) if ks else EMPTY_ROOT), t
    # the identical tries, asked the same, answer the same
    by = lambda t: [got.proof(j) for j in np.argsort(q_trie, kind="stable") if int(q_trie[j]) == t]  # noqa: E731
    assert sorted(map(tuple, by(5))) == sorted(map(tuple, by(11))) and by(5)


def test_cross_form(M, oracle):
    """the nodes of all proofs of trie t, as a set == what the node-set form emits for the same queries"""
    tries, keys, vals, seg, per_trie, queries, q_trie = _forest_case(np.random.default_rng(41))
    got = M.prove_batch(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    as_set = M.prove_nodeset(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    per = [set() for _ in tries]
    for j in range(len(queries)):
        per[int(q_trie[j])].update(got.proof(j))
    for t in range(len(tries)):
        assert per[t] == set(as_set.trie_nodes(t)), t
    assert np.array_equal(got.q_status, as_set.q_status) and np.array_equal(got.roots, as_set.roots)


def test_through_the_verifier(M, oracle):
    """32-byte keys: the output goes unchanged into phant_mpt_verify_batch and into the oracle's batch verifier"""
    rng = np.random.default_rng(3)
    tries = [random_kv(rng, suite.scale(300, 40), 32, 1, 80), random_kv(rng, 25, 32, 1, 80), random_kv(rng, 1, 32, 1, 80)]
    keys = [k for ks, _ in tries for k in ks]
    vals = [v for _, vs in tries for v in vs]
    seg = np.cumsum([0] + [len(ks) for ks, _ in tries]).astype(np.uint32)
    queries, q_trie = [], []
    for t, (ks, _) in enumerate(tries):
        qs = list(ks) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(30)] + [q for q in prove_ref.absent_queries(ks, rng, many=3) if len(q) == 32]
        queries += qs
        q_trie += [t] * len(qs)
    order = rng.permutation(len(queries))
    queries, q_trie = [queries[int(i)] for i in order], np.array([q_trie[int(i)] for i in order], np.uint32)
    got = M.prove_batch(_kv(M, keys, vals), queries, q_trie=q_trie, seg_first=seg)
    karr = np.frombuffer(b"".join(queries), np.uint8)
    value_of = [dict(zip(ks, vs)) for ks, vs in tries]
    for verify in (M.verify_batch, oracle.mpt_verify_batch):
        st, vo, vl = verify(got.roots.reshape(-1), q_trie, karr, 32, got.nodes, got.node_off, got.proof_first_node)
        assert np.array_equal(st[:len(queries)], got.q_status)
        for j, q in enumerate(queries):
            if st[j] == M.PROOF_PRESENT:
                assert got.nodes[int(vo[j]):int(vo[j]) + int(vl[j])].tobytes() == value_of[int(q_trie[j])][q]
        assert (st == M.PROOF_PRESENT).sum() == len(keys)


def test_device_form_feeds_the_verifier(M, oracle):
    """phant_mpt_prove_batch_dev: the same bytes as the host form, and its buffers go into verify_batch_dev where they lie"""
    import torch
    rng = np.random.default_rng(5)
    keys, vals = random_kv(rng, suite.scale(3000, 350), 32, 1, 80)
    queries = list(keys[::7]) + [q for q in prove_ref.absent_queries(keys, rng, many=5) if len(q) == 32]
    host = M.prove_batch(_kv(M, keys, vals), queries)
    kb, ko = M._pack(keys, np.uint32)
    vb, vo = M._pack(vals, np.uint64)
    qb, qo = M._pack(queries, np.uint32)
    dev = lambda a, dt: torch.from_numpy(a.astype(dt)).cuda()  # noqa: E731
    d = [dev(kb, np.uint8), dev(ko, np.int32), dev(vb, np.uint8), dev(vo, np.int64)]
    dq = [dev(qb, np.uint8), dev(qo, np.int32)]
    tn, nl = M.prove_batch_dev(*d, None, *dq, None, None, None)
    assert (tn, nl) == (host.total_nodes, len(host.nodes))
    # the blob one byte into its allocation: the gather's head and tail at every alignment of the proof blob
    raw = torch.zeros(nl + 1, dtype=torch.uint8).cuda()
    nodes, off = raw[1:], torch.zeros(tn + 1, dtype=torch.int64).cuda()
    first, roots = torch.zeros(len(queries) + 1, dtype=torch.int32).cuda(), torch.zeros(32, dtype=torch.uint8).cuda()
    st = torch.zeros(len(queries), dtype=torch.uint8).cuda()
    assert M.prove_batch_dev(*d, None, *dq, None, nodes, off, first, roots, st) == (tn, nl)
    torch.cuda.synchronize()
    assert nodes.cpu().numpy().tobytes() == host.nodes.tobytes() and off.cpu().numpy().astype(np.uint64).tobytes() == host.node_off.tobytes()
    assert roots.cpu().numpy().tobytes() == host.roots.tobytes() and np.array_equal(st.cpu().numpy(), host.q_status)
    assert np.array_equal(first.cpu().numpy().astype(np.uint32), host.proof_first_node)
    batch = M.ProofBatch(roots.reshape(1, 32), None, dq[0].reshape(len(queries), 32), nodes, off, first)
    verified = M.verify_batch_dev(batch)
    torch.cuda.synchronize()
    assert np.array_equal(verified.cpu().numpy(), host.q_status)
    bad = dev(np.array([0] * (len(queries) - 1) + [1], np.uint32), np.int32)
    from phant_amd import _lib as L
    with pytest.raises(L.PhantError) as e:
        M.prove_batch_dev(*d, None, *dq, bad, None, None)
    assert e.value.code == L.E_INVALID_ARG and "prove_batch" in str(e.value)


def _raw(M, L, ctx, keys, vals, queries, seg=None, q_trie=None, max_nodes=4096, nodes_cap=1 << 20, null=(), struct_size=None):
    """the C call itself -> (rc, out struct, buffers)"""
    from phant_amd.context import _np_ptr
    kb, ko = M._pack(list(keys), np.uint32)
    vb, vo = M._pack(list(vals), np.uint64)
    qb, qo = M._pack(list(queries), np.uint32)
    nt = 1 if seg is None else len(seg) - 1
    buf = {"nodes": np.full(max(nodes_cap, 1), 0xEE, np.uint8), "node_off": np.full(max_nodes + 1, 0xEEEEEEEE, np.uint64),
           "proof_first_node": np.full(len(queries) + 1, 0xEEEEEEEE, np.uint32), "roots": np.full(32 * nt, 0xEE, np.uint8),
           "q_status": np.full(max(len(queries), 1), 0xEE, np.uint8)}
    p = {k: (None if k in null else _np_ptr(v)) for k, v in buf.items()}
    o = L.PhantProveBatchOut(C.sizeof(L.PhantProveBatchOut) if struct_size is None else struct_size, max_nodes, nodes_cap, p["nodes"],
                             p["node_off"], p["proof_first_node"], p["roots"], p["q_status"], 0, 0, 0)
    seg_a = None if seg is None else np.ascontiguousarray(seg, np.uint32)
    qt = None if q_trie is None else np.ascontiguousarray(q_trie, np.uint32)
    rc = ctx._lib.phant_mpt_prove_batch(ctx.handle, _np_ptr(kb), _np_ptr(ko), _np_ptr(vb), _np_ptr(vo), len(keys),
                                        None if seg_a is None else _np_ptr(seg_a), nt, _np_ptr(qb), _np_ptr(qo),
                                        None if qt is None else _np_ptr(qt), len(queries), C.byref(o))
    return rc, o, buf


def test_capacity_and_arguments(M, oracle):
    from phant_amd import _lib as L
    ctx = _ctx()
    rng = np.random.default_rng(11)
    keys, vals = random_kv(rng, 60, 32, 1, 80)
    queries = list(keys[::2]) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(10)] + [keys[0], b""]
    trie = oracle.Trie(keys, vals)
    want = [trie.prove(q) for q in queries]
    tn, nl = sum(map(len, want)), sum(len(x) for w in want for x in w)
    lists = lambda b: [[b["nodes"][int(b["node_off"][k]):int(b["node_off"][k + 1])].tobytes()  # noqa: E731
                        for k in range(int(b["proof_first_node"][j]), int(b["proof_first_node"][j + 1]))] for j in range(len(queries))]
    rc, o, full = _raw(M, L, ctx, keys, vals, queries)
    assert rc == 0 and (int(o.total_nodes), int(o.nodes_len)) == (tn, nl)
    assert lists(full) == want and int(full["node_off"][0]) == 0 and int(full["node_off"][tn]) == nl
    assert (full["nodes"][nl:] == 0xEE).all() and (full["node_off"][tn + 1:] == 0xEEEEEEEE).all()
    # one node or one byte too small: OK, exact totals, the three laid-out buffers untouched; the totals then suffice
    for mn, nc in ((tn - 1, nl), (tn, nl - 1)):
        rc, o, b = _raw(M, L, ctx, keys, vals, queries, max_nodes=mn, nodes_cap=nc)
        assert rc == 0 and (o.total_nodes, o.nodes_len) == (tn, nl)
        assert (b["nodes"] == 0xEE).all() and (b["node_off"] == 0xEEEEEEEE).all() and (b["proof_first_node"] == 0xEEEEEEEE).all()
        assert np.array_equal(b["q_status"], full["q_status"]) and np.array_equal(b["roots"], full["roots"])
    rc, o, b = _raw(M, L, ctx, keys, vals, queries, max_nodes=tn, nodes_cap=nl)
    assert rc == 0 and lists(b) == want
    assert np.array_equal(b["nodes"][:nl], full["nodes"][:nl])  # the same input twice: identical bytes
    # each output pointer NULL in turn
    for name in ("nodes", "node_off", "proof_first_node", "roots", "q_status"):
        rc, o, b = _raw(M, L, ctx, keys, vals, queries, null=(name,))
        assert rc == 0 and (o.total_nodes, o.nodes_len) == (tn, nl), name
        assert (b[name] == (0xEE if b[name].dtype == np.uint8 else 0xEEEEEEEE)).all(), name
        for other in b:  # every wanted buffer as in the full call, sentinels behind the written part included
            if other != name:
                assert np.array_equal(b[other], full[other]), (name, other)
    rc, o, b = _raw(M, L, ctx, keys, vals, queries, null=("nodes", "node_off", "proof_first_node", "roots", "q_status"))
    assert rc == 0 and (o.total_nodes, o.nodes_len) == (tn, nl)
    # no queries; no keys
    rc, o, b = _raw(M, L, ctx, keys, vals, [])
    assert rc == 0 and (o.total_nodes, o.nodes_len) == (0, 0) and list(b["proof_first_node"]) == [0]
    assert b["roots"].tobytes() == oracle.mptize(keys, vals) and int(b["node_off"][0]) == 0
    rc, o, b = _raw(M, L, ctx, [], [], [b"\x01" * 32, b""])
    assert rc == 0 and (o.total_nodes, o.nodes_len) == (0, 0) and b["roots"].tobytes() == EMPTY_ROOT
    assert list(b["q_status"]) == [M.PROOF_ABSENT, M.PROOF_ABSENT] and list(b["proof_first_node"]) == [0, 0, 0]
    assert int(b["node_off"][0]) == 0
    # refused, with the node-set call's codes
    rc, _, _ = _raw(M, L, ctx, [keys[1], keys[0]] + keys[2:], vals, queries)
    assert rc == L.E_UNSORTED
    rc, _, _ = _raw(M, L, ctx, keys, vals, queries, seg=[0, 30, 60], q_trie=[0] * (len(queries) - 1) + [2])
    assert rc == L.E_INVALID_ARG
    for size in (0, C.sizeof(L.PhantProveBatchOut) - 8, C.sizeof(L.PhantProveBatchOut) + 8):
        rc, _, _ = _raw(M, L, ctx, keys, vals, queries, struct_size=size)
        assert rc == L.E_INVALID_ARG
    rc, _, _ = _raw(M, L, ctx, keys, vals, queries, seg=[0, 30, 60], q_trie=None)
    assert rc == L.E_INVALID_ARG
    rc, _, _ = _raw(M, L, ctx, keys + [b"\xff" * 256], vals + [b"v"], queries)  # a key longer than 255 bytes
    assert rc == L.E_UNSUPPORTED


def test_device_capacity_and_arguments(M, oracle):
    """test_capacity_and_arguments for phant_mpt_prove_batch_dev"""
    from functools import partial
    from phant_amd import _lib as L
    from tests.test_gpu_prove import _raw_dev, device_form_edge_cases
    rng = np.random.default_rng(12)  # (the keys and queries of device_form_edge_cases)
    keys, vals = random_kv(rng, 60, 32, 1, 80)
    queries = list(keys[::2]) + [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(9)] + [b""]
    tn, full = device_form_edge_cases(M, oracle, L, _ctx(), _raw, partial(_raw_dev, batch=True), "proof_first_node")
    trie = oracle.Trie(keys, vals)
    want = [trie.prove(q) for q in queries]
    got = [[full["nodes"][int(full["node_off"][k]):int(full["node_off"][k + 1])].tobytes()
            for k in range(int(full["proof_first_node"][j]), int(full["proof_first_node"][j + 1]))] for j in range(len(queries))]
    assert got == want and tn == sum(map(len, want))


def test_one_context_small_large_small(M, oracle):
    from phant_amd.context import Context, default_context
    rng = np.random.default_rng(21)
    sets = []
    for n in (12, suite.scale(6000, 500), 30):
        keys, vals = random_kv(rng, n, 32, 1, 80)
        sets.append((keys, vals, list(keys[::5]) + prove_ref.absent_queries(keys, rng, many=3)))

    def run(ctx, i):
        keys, vals, q = sets[i]
        g = M.prove_batch(_kv(M, keys, vals), q, ctx=ctx)
        return g.nodes.tobytes(), g.node_off.tobytes(), g.proof_first_node.tobytes(), g.roots.tobytes(), g.q_status.tobytes()

    ctx = default_context()
    first = run(ctx, 0)
    assert M.mptize(_kv(M, *sets[1][:2]), ctx=ctx) == oracle.mptize(*sets[1][:2])
    large = run(ctx, 1)
    keys, vals, q = sets[1]
    g = M.prove_batch(_kv(M, keys, vals), q, ctx=ctx)
    _check_lists(oracle, oracle.Trie(keys, vals), keys, q, g)
    keys, vals, q = sets[2]
    g = M.prove_batch(_kv(M, keys, vals), list(keys), ctx=ctx)
    _check_lists(oracle, oracle.Trie(keys, vals), keys, list(keys), g)
    assert M.prove_nodeset(_kv(M, keys, vals), list(keys), ctx=ctx).total_nodes == len({x for j in range(len(keys)) for x in g.proof(j)})
    assert run(ctx, 0) == first
    fresh = type(ctx)() if suite.EMULATED else Context(ctx.device)
    try:
        assert run(fresh, 0) == first and run(fresh, 1) == large
    finally:
        fresh.close()


# ---------------------------------------------------------------- phant_state_proofs: state + keys -> an EIP-1186 witness
@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _slot_key(addr, s):
    return addr + int(s).to_bytes(32, "big")


def _expected_proofs(oracle, accounts, keys):
    """the document the oracle's prover gives for `keys`, in document order: -> ([(root index, preimage, node list, account)],
    [(address, slots in order)], the state root, the storage root of every touched account)"""
    state, _, storage = R.build_tries(oracle, accounts)
    index = {a["addr"]: i for i, a in enumerate(accounts)}
    touched = list(dict.fromkeys(k[:20] for k in keys))
    slots = {a: [] for a in touched}
    for k in keys:
        if len(k) == 52 and k[20:] not in slots[k[:20]]:
            slots[k[:20]].append(k[20:])
    proofs, sroots = [], []
    for t, addr in enumerate(touched):
        proofs.append((0, addr, state.prove(oracle.keccak256(addr)), t))
        i = index.get(addr)
        sroots.append(storage[i][0].root() if i in storage else EMPTY_ROOT)
        for s in slots[addr]:
            proofs.append((1 + t, s, storage[i][0].prove(oracle.keccak256(s)) if i in storage else [], t))
    return proofs, [(a, slots[a]) for a in touched], state.root(), sroots


def _proof_lists(info):
    b, off, first = info["nodes"].tobytes(), info["node_off"], info["proof_first_node"]
    return [[b[int(off[k]):int(off[k + 1])] for k in range(int(first[j]), int(first[j + 1]))] for j in range(info["n_proofs"])]


def _info_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _state_proofs_case(P, oracle, accounts, keys, fixture_root=None, flipped=None):
    """flipped: collects which kinds of proof (storage: True, account: False) had a node byte flipped"""
    EA = P.engine_api
    flipped = set() if flipped is None else flipped
    w = P.state.get_proofs(accounts, keys)
    try:
        info = w.info()
        want, touched, want_root, sroots = _expected_proofs(oracle, accounts, keys)
        assert w.state_root == want_root == P.state.state_root(accounts)
        if fixture_root is not None:
            assert w.state_root.hex() == fixture_root
        # every proof list is the oracle's, in document order, with its root index, account and preimage
        assert not info["node_set"] and info["n_proofs"] == len(want) and info["n_accounts"] == len(touched)
        assert info["n_slots"] == sum(len(s) for _, s in touched) and info["n_roots"] == 1 + len(touched)
        got = _proof_lists(info)
        pre, poff = info["preimages"].tobytes(), info["preimage_off"]
        for j, (ridx, preimage, nodes, account) in enumerate(want):
            assert got[j] == nodes, j
            assert (int(info["root_idx"][j]), int(info["account_of"][j])) == (ridx, account)
            assert pre[int(poff[j]):int(poff[j + 1])] == preimage
        assert info["total_nodes"] == sum(len(x[2]) for x in want) and int(info["node_off"][0]) == 0
        assert info["roots"].tobytes() == want_root + b"".join(sroots)
        # it verifies against the root phant_state_root gives, statuses as the state says
        status, n_failed = w.verify(expected_state_root=P.state.state_root(accounts))
        assert n_failed == 0
        by = {a["addr"]: a for a in accounts}
        want_status = []
        for addr, slots in touched:
            want_status.append(M_PRESENT if addr in by else M_ABSENT)
            want_status += [M_PRESENT if addr in by and int(by[addr]["storage"].get(int.from_bytes(s, "big"), 0)) else M_ABSENT for s in slots]
        assert list(status) == want_status
        # the declarations are the state's
        text = w.to_json()
        doc = json.loads(text)
        assert doc["stateRoot"] == "0x" + want_root.hex() and len(doc["accounts"]) == len(touched)
        for obj, (addr, slots), sr in zip(doc["accounts"], touched, sroots):
            a = by.get(addr)
            assert obj["address"] == "0x" + addr.hex() and obj["storageHash"] == "0x" + sr.hex()
            assert int(obj["nonce"], 16) == (a["nonce"] if a else 0) and int(obj["balance"], 16) == (a["balance"] if a else 0)
            assert obj["codeHash"] == "0x" + oracle.keccak256(bytes(a["code"]) if a else b"").hex()
            assert [sp["key"] for sp in obj["storageProof"]] == ["0x" + s.hex() for s in slots]
            assert [int(sp["value"], 16) for sp in obj["storageProof"]] == [int(a["storage"].get(int.from_bytes(s, "big"), 0)) if a else 0 for s in slots]
        # to_json -> parse_json: the same object, and it verifies again
        back = EA.ExecutionWitness.parse_json(text)
        try:
            _info_equal(info, back.info())
            status2, n_failed2 = back.verify(expected_state_root=want_root)
            assert n_failed2 == 0 and np.array_equal(status, status2)
        finally:
            back.close()
        # one byte of one node flipped: a storage proof fails alone, an account proof takes the storage proofs under it with it --
        # the longest list of either kind (the last of them), its last node
        first_of = [x[3] for x in want]
        for storage_proof in (True, False):
            pick = [x for x in range(len(want)) if (want[x][0] != 0) == storage_proof and want[x][2]]
            if not pick:
                continue
            j = max(pick, key=lambda x: (len(want[x][2]), x))
            t = want[j][3]
            bad_doc = json.loads(text)
            obj = bad_doc["accounts"][t]
            place = obj["storageProof"][j - first_of.index(t) - 1]["proof"] if storage_proof else obj["accountProof"]
            nd = bytearray(bytes.fromhex(place[-1][2:]))
            nd[len(nd) // 2] ^= 0x40
            place[-1] = "0x" + bytes(nd).hex()
            bad = EA.ExecutionWitness.parse_json(json.dumps(bad_doc))
            try:
                status3, _ = bad.verify(expected_state_root=want_root)
                failed = [x for x in range(len(want)) if status3[x] not in (M_PRESENT, M_ABSENT)]
                assert failed == ([j] if storage_proof else [x for x in range(len(want)) if want[x][3] == t])
                assert [status3[x] for x in range(len(want)) if x not in failed] == [status[x] for x in range(len(want)) if x not in failed]
            finally:
                bad.close()
            flipped.add(storage_proof)
    finally:
        w.close()


M_PRESENT, M_ABSENT = prove_ref.PRESENT, prove_ref.ABSENT


def test_state_proofs_of_fixture_allocs(P, oracle):
    fx = golden.fixtures()
    # the first 8 genesis allocs that have storage -- the fixtures hold ONE such alloc, so the eight are filled up with the first
    # allocs in fixture order, and the largest alloc (401 accounts) joins them
    allocs = [(c, golden.accounts_of(c["pre"], fx["codes"])) for c in fx["cases"]]
    with_storage = [c for c, acc in allocs if any(a["storage"] for a in acc)][:8]
    assert with_storage
    rest = [c for c, _ in allocs if c not in with_storage]
    cases = with_storage + rest[:suite.scale(8 - len(with_storage), 3)] + [max(allocs, key=lambda x: len(x[1]))[0]][:suite.scale(1, 0)]
    rng = np.random.default_rng(61)
    for c in cases:
        accounts = golden.accounts_of(c["pre"], fx["codes"])
        keys = []
        for a in accounts:
            keys.append(a["addr"])
            keys += [_slot_key(a["addr"], s) for s in a["storage"]]
            keys.append(_slot_key(a["addr"], int(rng.integers(1 << 40, 1 << 62))))  # a slot it does not have
        ghost = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
        keys += [ghost, _slot_key(ghost, 1), keys[0], keys[1]]  # an address the state does not hold, a slot under it, repeats
        flipped = set()
        _state_proofs_case(P, oracle, accounts, keys, c["genesis_state_root"], flipped)
        assert flipped == ({True, False} if c in with_storage else {False})


def test_state_proofs_of_a_block_shaped_state(P, oracle):
    rng = np.random.default_rng(62)
    n = suite.scale(1500, 120)
    doc, root, accounts = R.block_witness_doc(oracle, rng, n_accounts=n, n_contracts=max(4, n // 40), max_slots=suite.scale(60, 12),
                                              n_touched=max(20, n // 5), n_absent=max(4, n // 50))
    keys = [bytes.fromhex(k[2:]) for k in doc["keys"]]
    for a in accounts[:5]:  # zero-valued slots: in the state's arrays, not in the trie
        for _ in range(3):
            s = int(rng.integers(1 << 62, 1 << 63))
            a["storage"][s] = 0
            keys += [a["addr"], _slot_key(a["addr"], s)]
    keys += keys[:7]  # repeats
    assert P.state.state_root(accounts) == root
    flipped = set()
    _state_proofs_case(P, oracle, accounts, keys, flipped=flipped)
    assert flipped == {True, False}  # a storage proof and an account proof were damaged


def test_state_proofs_arguments(P, oracle):
    from phant_amd import _lib as L
    rng = np.random.default_rng(63)
    accounts = [{"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": 1, "balance": 2, "code": b"", "storage": {}} for _ in range(5)]
    for bad in (b"\x01" * 32, b"\x01" * 19, b"", b"\x01" * 53):
        with pytest.raises(L.PhantError) as e:
            P.state.get_proofs(accounts, [accounts[0]["addr"], bad])
        assert e.value.code == L.E_INVALID_ARG and "key 1" in str(e.value)
    w = P.state.get_proofs(accounts, [])  # no keys: a witness without proofs, the root all the same
    assert w.info()["n_proofs"] == 0 and w.info()["total_nodes"] == 0 and w.state_root == P.state.state_root(accounts)
    assert json.loads(w.to_json()) == {"stateRoot": "0x" + w.state_root.hex(), "accounts": []}
    w.close()
    # no live slot anywhere in the state: the storage proofs are zero-node proofs against the empty root
    _state_proofs_case(P, oracle, accounts, [accounts[1]["addr"], _slot_key(accounts[1]["addr"], 7), _slot_key(b"\x77" * 20, 7)])
    w = P.state.get_proofs([], [accounts[0]["addr"], _slot_key(accounts[0]["addr"], 3)])  # the empty state: every key absent under the empty root
    assert w.state_root == EMPTY_ROOT and w.info()["total_nodes"] == 0 and w.info()["n_proofs"] == 2
    status, n_failed = w.verify(expected_state_root=EMPTY_ROOT)
    assert n_failed == 0 and list(status) == [M_ABSENT, M_ABSENT]
    w.close()
    # the index form of a written document has no decoded nodes to write
    w = P.state.get_proofs(accounts, [accounts[0]["addr"]])
    idx = P.engine_api.ExecutionWitness.index_json(w.to_json())
    with pytest.raises(L.PhantError) as e:
        idx.to_json()
    assert e.value.code == L.E_UNSUPPORTED
    idx.close()
    w.close()
