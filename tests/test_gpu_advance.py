"""phant_exec_witness_advance: the witness of the NEXT block out of the post-state build.  The node set against the full-state
reference tests/advance_ref.py (oracle.Trie over the complete pre- and post-state), the next witness proven against the post root
with phant_exec_witness_prestate, and chains of blocks under one witness (phant_amd.stateless.new_payload_chain)."""
import ctypes as C

import numpy as np
import pytest

from tests import advance_ref as A
from tests import golden, suite
from tests import poststate_ref as Q
from tests import prestate_ref as R
from tests import test_gpu_poststate as T
from tests.test_gpu_poststate import _acc, _block_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _copy(info):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in info.items()}


def _advance(P, oracle, doc, root, writes, ctx=None, keep_old=False):
    """-> (outputs, info of the witness, info of the next witness or None)"""
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    nxt = None
    try:
        info = _copy(w.info())
        got, nxt = w.advance_arrays(ctx, root, Q.write_arrays(oracle, info, writes), keep_old)
        return got, info, None if nxt is None else _copy(nxt.info())
    finally:
        w.close()
        if nxt is not None:
            nxt.close()


def _check(P, oracle, accounts, writes, rng, tries=None, ctx=None, **kw):
    """The two checks of every case: the next witness's nodes are the reference's, and it proves the post alloc under the post root
    (every account and slot of the keys; what the block deleted is ABSENT).  Same signature and result as test_gpu_poststate._check."""
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, tries=tries, **kw)
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    nxt = None
    try:
        info = _copy(w.info())
        got, nxt = w.advance_arrays(ctx, root, Q.write_arrays(oracle, info, writes))
        want = Q.expected(oracle, info, accounts, writes)
        assert got["n_failed"] == 0 and nxt is not None, (got["n_failed"], got["account_status"][:8], got["slot_status"][:8])
        assert got["state_root"] == want["state_root"]
        assert np.array_equal(got["storage_roots"], want["storage_roots"])
        ref = A.expected(oracle, info, accounts, writes)
        ninfo = nxt.info()
        have = A.nodes_of(ninfo)
        assert sorted(have) == sorted(ref["nodes"]), (len(have), len(ref["nodes"]), len(set(have) - set(ref["nodes"])),
                                                      len(set(ref["nodes"]) - set(have)))
        for k in ("addresses", "slot_first", "slots", "codes", "code_off"):
            assert np.array_equal(ninfo[k], info[k]), k
        A.check_prestate(oracle, nxt.prestate_arrays(ctx, got["state_root"]), ninfo, ref["after"])
    finally:
        w.close()
        if nxt is not None:
            nxt.close()
    got["_ref"] = ref
    return got, doc, root


# ---------------------------------------------------------------- 1. fixtures
def test_fixture_post_states(P, oracle):
    """Every fixture case with `post` (built as test_fixture_post_state_roots builds them): the next witness holds the reference's
    nodes and proves the post alloc under the fixture's post root."""
    fx = golden.fixtures()
    cases = [c for c in fx["cases"] if c.get("post") and c.get("post_state_root")]
    assert len(cases) == 73
    cases = cases[:suite.scale(len(cases), 8)]
    rng = np.random.default_rng(1)
    for c in cases:
        pre = golden.accounts_of(c["pre"], fx["codes"])
        post = {a["addr"]: a for a in golden.accounts_of(c["post"], fx["codes"])}
        by = {a["addr"]: a for a in pre}
        writes = {}
        for addr in list(by) + [a for a in post if a not in by]:
            if addr not in post:
                writes[addr] = None
                continue
            a = post[addr]
            old = by.get(addr, {"storage": {}})["storage"]
            st = {s: int(a["storage"].get(s, 0)) for s in set(old) | set(a["storage"])}
            writes[addr] = {"nonce": a["nonce"], "balance": a["balance"], "code": a["code"], "storage": st}
        got, _, root = _check(P, oracle, pre, writes, rng)
        assert root.hex() == c["genesis_state_root"] and got["state_root"].hex() == c["post_state_root"], c["name"]


# ---------------------------------------------------------------- 2. block-shaped states
def _block(oracle, seed):
    rng = np.random.default_rng(seed)
    # (the same sizes emulated, three seconds a case there: what the case must contain depends on them)
    accounts, writes, extra = _block_case(oracle, rng, 200, 12, 9, 40)
    return accounts, writes, extra, rng


# three seeds whose case holds everything asserted below, chosen with the reference alone (of 31 .. 49, seven have no new node beside
# the keys' walks: at these sizes most remnants of a split are themselves keys of the witness)
@pytest.mark.parametrize("seed", [31, 33, 34])
def test_block_shaped_states(P, oracle, seed):
    accounts, writes, extra, rng = _block(oracle, seed)
    got, _, _ = _check(P, oracle, accounts, writes, rng, extra_slots=extra)
    ref = got["_ref"]
    assert ref["beside"] > 0                # a split's remnant or a collapse's survivor: new nodes on no key's walk
    assert ref["created_with_slots"] > 0    # a contract the block creates, with live slots among the keys
    # a storage trie that held slots and is empty afterwards: nothing of it is emitted.  (_block_case zeroes every slot only of
    # touched accounts number 3, 10, 17, ...; with twelve contracts those are a no-op SET and a deleted account, so the trie that goes
    # here is a deleted contract's -- the one the build still walks and the sink must keep quiet about.)
    pre = {a["addr"]: a for a in accounts}
    post = {a["addr"]: a for a in ref["after"]}
    assert any(pre[x]["storage"] and not post.get(x, {"storage": {}})["storage"] for x in writes if x in pre)


# ---------------------------------------------------------------- 3. collapses and splits
def test_collapses_and_splits(P, oracle, monkeypatch):
    """the hand-built shapes of test_gpu_poststate.test_collapses_and_splits, each through the two checks"""
    monkeypatch.setattr(T, "_check", _check)
    T.test_collapses_and_splits(P, oracle)


# ---------------------------------------------------------------- 4. chosen trie keys
def test_embedded_nodes_and_sixty_three_shared_nibbles(P, oracle, monkeypatch):
    """The shapes of test_gpu_poststate's test of the same name, under PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS: the storage trie's members
    are exactly the reference's over the RAW keys (no node under 32 bytes among them), the state trie's the reference's, and the
    next witness re-roots to the same root with nothing written."""
    import copy
    from phant_amd.context import default_context
    from tests.witness_util import _rlp_int
    real_raw_case, seen = T._raw_case, {}

    def run(P_, oracle_, doc, root, writes, ctx=None):
        w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
        nxt = None
        try:
            info = _copy(w.info())
            arr = Q.write_arrays(oracle, info, writes)
            got, nxt = w.advance_arrays(ctx, root, arr)
            A.arrays_equal(got, w.poststate_arrays(ctx, root, arr))
            assert nxt is not None and got["n_failed"] == 0
            seen["nodes"] = A.nodes_of(nxt.info())
            again = nxt.poststate_arrays(ctx, got["state_root"], {"account_op": np.zeros(info["n_accounts"], np.uint8)})
            assert again["n_failed"] == 0 and again["state_root"] == got["state_root"]
            assert np.array_equal(again["storage_roots"], got["storage_roots"])
            return got, info
        finally:
            w.close()
            if nxt is not None:
                nxt.close()

    def raw_case(P_, oracle_, pre_slots, upd, rng, neighbours=True):
        twin = copy.deepcopy(rng)  # (the accounts _raw_case is about to draw)
        owner, others = _acc(twin, {}, b"\x01\x02"), [_acc(twin) for _ in range(12)]
        got, sroot, root = real_raw_case(P_, oracle_, pre_slots, upd, rng, neighbours)
        after = dict(pre_slots)
        after.update(upd)

        def trie(slots):
            kv = sorted((bytes.fromhex(k), _rlp_int(v)) for k, v in slots.items() if v)
            return (oracle.Trie([k for k, _ in kv], [v for _, v in kv]), [k for k, _ in kv]) if kv else (None, [])

        def state(sr):
            kv = sorted([(oracle.keccak256(a["addr"]), R.account_leaf(oracle, a, Q.EMPTY_ROOT)) for a in others]
                        + [(oracle.keccak256(owner["addr"]), R.account_leaf(oracle, owner, sr))])
            return oracle.Trie([k for k, _ in kv], [v for _, v in kv]), [k for k, _ in kv]

        (t0, k0), (t1, k1) = trie(pre_slots), trie(after)
        want, _ = A.trie_nodes(t1, k1, t0, k0, [bytes.fromhex(k) for k in upd], check_distinct=True)
        (s0, sk0), (s1, sk1) = state(t0.root()), state(sroot)
        assert s1.root() == root
        want2, _ = A.trie_nodes(s1, sk1, s0, sk0, [oracle.keccak256(owner["addr"])])
        assert sorted(seen["nodes"]) == sorted(want + want2), (len(seen["nodes"]), len(want), len(want2))
        assert all(len(n) >= 32 or oracle.keccak256(n) in (sroot, root) for n in seen["nodes"])
        return got, sroot, root

    monkeypatch.setattr(T, "_run", run)
    monkeypatch.setattr(T, "_raw_case", raw_case)
    try:
        T.test_embedded_nodes_and_sixty_three_shared_nibbles(P, oracle)
    finally:
        default_context().diag_set("poststate_raw_slot_keys", 0)


# ---------------------------------------------------------------- 5. a chain of blocks under one witness
def _state_of(P, accounts):
    return [P.state.AccountState(addr=a["addr"], nonce=a["nonce"], balance=a["balance"], code=a["code"], storage=dict(a["storage"]))
            for a in accounts]


def _after(P, accounts, writes):
    """accounts_after of one block for new_payload_chain / advance: the written accounts after the block (None: deleted)"""
    post = {a["addr"]: a for a in Q.apply_writes(accounts, writes)}
    out = {}
    for addr in writes:
        a = post.get(addr)
        out[addr] = None if a is None else P.state.AccountState(addr=addr, nonce=a["nonce"], balance=a["balance"], code=a["code"],
                                                                storage=dict(a["storage"]))
    return out


def _keys_of(writes):
    keys = []
    for addr, w in writes.items():
        keys.append(addr)
        upd = {} if w is None else (w[1] if isinstance(w, tuple) else w["storage"])
        keys += [addr + int(s).to_bytes(32, "big") for s in upd]
    return keys


def test_three_blocks_under_one_witness(P, oracle):
    rng = np.random.default_rng(70)
    accounts = [_acc(rng, {int(rng.integers(0, 1 << 62)): T._val(rng) for _ in range(4)} if i < 6 else None, b"\x01" if i < 6 else b"")
                for i in range(150)]
    state, blocks, keys = accounts, [], []
    for b in range(3):
        writes = {}
        for i in rng.choice(len(state), 8, replace=False):
            a = state[int(i)]
            st = {s: (0 if rng.random() < 0.3 else T._val(rng)) for s in list(a["storage"])[:2]}
            if a["storage"]:
                st[int(rng.integers(0, 1 << 62))] = T._val(rng)
            writes[a["addr"]] = {"nonce": a["nonce"] + 1, "balance": T._val(rng), "code": a["code"], "storage": st}
        new = _acc(rng)
        writes[new["addr"]] = {"nonce": 1, "balance": 5 + b, "code": b"", "storage": {}}
        keys += _keys_of(writes)
        after = Q.apply_writes(state, writes)
        blocks.append((_after(P, state, writes), oracle.state_root(after)))
        state = after
    # no removal of an account in this chain: the witness of the union of the keys is enough (slots a later block zeroes keep their
    # neighbours through may_remove)
    w = P.stateless.build_witness(_state_of(P, accounts), keys, may_remove=[k for k in keys if len(k) == 52])
    try:
        text, root = w.to_json(), w.state_root
    finally:
        w.close()
    assert root == oracle.state_root(accounts)
    posts = P.stateless.new_payload_chain(text, root, blocks)
    assert [p.root for p in posts] == [r for _, r in blocks]
    off = bytearray(blocks[1][1])
    off[0] ^= 1
    with pytest.raises(P.stateless.PoststateError, match="block 1"):
        P.stateless.new_payload_chain(text, root, [blocks[0], (blocks[1][0], bytes(off)), blocks[2]])


def test_a_sibling_for_a_later_removal_needs_keep_old(P, oracle):
    """Block 2 removes an account whose branch then holds one other child: the producer shipped that sibling (may_remove).  Block 1's
    writes do not touch it, so it is no node of block 1's post-state walks: only KEEP_OLD carries it to block 2."""
    rng = np.random.default_rng(71)
    accounts = [_acc(rng) for _ in range(150)]
    lone, _ = T._two_child_victims(oracle, accounts)
    victim = accounts[lone[0]]
    vk = oracle.keccak256(victim["addr"]).hex()
    other = next(a for a in accounts if oracle.keccak256(a["addr"]).hex()[:1] != vk[:1])
    w1 = {other["addr"]: {"nonce": other["nonce"] + 1, "balance": 7, "code": b"", "storage": {}}}
    w2 = {victim["addr"]: None}
    s1 = Q.apply_writes(accounts, w1)
    s2 = Q.apply_writes(s1, w2)
    w = P.stateless.build_witness(_state_of(P, accounts), [other["addr"], victim["addr"]], may_remove=[victim["addr"]])
    try:
        root = w.state_root
        results = {}
        for keep in (True, False):
            p1, n1 = w.advance(None, root, _after(P, accounts, w1), keep_old=keep)
            try:
                assert p1.ok and p1.root == oracle.state_root(s1)
                p2, n2 = n1.advance(None, p1.root, _after(P, s1, w2), keep_old=keep)
                if n2 is not None:
                    n2.close()
            finally:
                n1.close()
            results[keep] = p2
    finally:
        w.close()
    assert results[True].ok and results[True].root == oracle.state_root(s2)
    k = [bytes(a) for a in [other["addr"], victim["addr"]]].index(victim["addr"])
    assert not results[False].ok and results[False].account_status[k] == Q.MISSING_SIBLING and results[False].root == bytes(32)


# ---------------------------------------------------------------- 6. failure forms
def test_failures_give_no_next_witness(P, oracle):
    rng = np.random.default_rng(72)
    accounts, writes, extra = _block_case(oracle, rng, suite.scale(300, 80), 6, 8, suite.scale(40, 15))
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)

    def same_as_poststate(doc, writes):
        got, info, nxt = _advance(P, oracle, doc, root, writes)
        assert nxt is None and got["n_failed"] > 0 and got["state_root"] == bytes(32)
        A.arrays_equal(got, T._run(P, oracle, doc, root, writes)[0])
        return got, info

    st = list(doc["state"])  # a damaged node
    b = bytearray(R._unhex(st[3]))
    b[len(b) // 2] ^= 0x10
    st[3] = R._hex(bytes(b))
    same_as_poststate(dict(doc, state=st), writes)
    plain = [_acc(rng) for _ in range(suite.scale(400, 120))]  # a missing sibling
    lone, _ = T._two_child_victims(oracle, plain)
    gone = {plain[lone[0]]["addr"]: None}
    thin, root = Q.witness_doc(oracle, plain, gone, rng, neighbours=False)
    got, _ = same_as_poststate(thin, gone)
    assert (got["account_status"] == Q.MISSING_SIBLING).all()
    ghost = _acc(rng)["addr"]  # a KEEP on an absent account with a slot write
    bad = {ghost: ("keep", {5: 7}), plain[0]["addr"]: None}
    d3, root = Q.witness_doc(oracle, plain, bad, rng)
    got, info = same_as_poststate(d3, bad)
    assert got["account_status"][[bytes(a) for a in info["addresses"]].index(ghost)] == Q.MISMATCH


def test_arguments(P, oracle):
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from phant_amd.stateless import PoststateIO
    rng = np.random.default_rng(73)
    accounts = [_acc(rng) for _ in range(30)]
    writes = {accounts[0]["addr"]: None, accounts[1]["addr"]: {"nonce": 3, "balance": 4, "code": b"", "storage": {1: 2}}}
    doc, root = Q.witness_doc(oracle, accounts, writes, rng)
    ctx = default_context()
    lib = ctx._lib
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    info = w.info()
    arr = Q.write_arrays(oracle, info, writes)
    out_root = np.zeros(32, np.uint8)

    def io(**kw):
        o = PoststateIO()
        o.struct_size = C.sizeof(PoststateIO)
        for k, a in arr.items():
            setattr(o, k, a.ctypes.data)
        o.state_root = out_root.ctypes.data
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    rb = C.create_string_buffer(root, 32)
    h = C.c_void_p()

    def call(c, wh, r, o, flags=0, nxt=True):
        h.value = 0xdead
        rc = lib.phant_exec_witness_advance(c, wh, r, C.byref(o) if o is not None else None, flags, C.byref(h) if nxt else None)
        if rc != L.OK and c is not None and wh is not None and o is not None and nxt:
            assert not h.value  # (no witness on an error the call could report)
        return rc

    assert call(None, w._h, rb, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, None, rb, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, None) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(), nxt=False) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, None, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(struct_size=8)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(struct_size=C.sizeof(PoststateIO) + 8)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(), flags=2) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(), flags=0x80000001) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(account_op=None)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io()) == L.OK and h.value
    assert out_root.tobytes() == Q.expected(oracle, info, accounts, writes)["state_root"]
    lib.phant_exec_witness_free(h)
    w.close()
    # no account among the keys: the root stays, the next witness has no nodes (with KEEP_OLD: the old ones)
    w = P.stateless.StatelessWitness.parse_json(R.dumps({"state": doc["state"], "keys": []}))
    for keep, n in ((False, 0), (True, len(doc["state"]))):
        got, nxt = w.advance_arrays(None, root, {}, keep)
        assert got["state_root"] == root and got["n_failed"] == 0 and nxt.info()["total_nodes"] == n
        nxt.close()
    w.close()


# ---------------------------------------------------------------- 7. the same outputs as phant_exec_witness_poststate
def test_same_outputs_as_poststate_and_keep_old(P, oracle):
    accounts, writes, extra, rng = _block(oracle, 31)
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)
    got, info, nxt = _advance(P, oracle, doc, root, writes)
    A.arrays_equal(got, T._run(P, oracle, doc, root, writes)[0])
    kept, _, both = _advance(P, oracle, doc, root, writes, keep_old=True)
    A.arrays_equal(got, kept)
    new, all_ = A.nodes_of(nxt), A.nodes_of(both)
    assert all_[:len(new)] == new and all_[len(new):] == [R._unhex(x) for x in doc["state"]]


# ---------------------------------------------------------------- 8. determinism and reuse
def _json_of(P, oracle, doc, root, writes, ctx=None):
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        got, nxt = w.advance_arrays(ctx, root, Q.write_arrays(oracle, w.info(), writes))
        try:
            return got, nxt.to_json()
        finally:
            nxt.close()
    finally:
        w.close()


def test_the_same_call_twice_and_one_context_small_large_small(P, oracle):
    from tests import test_gpu_prestate_more as M
    rng = np.random.default_rng(74)
    cases = []
    for n, t in ((40, 6), (suite.scale(1500, 300), suite.scale(250, 45)), (25, 5)):
        accounts, writes, extra = _block_case(oracle, rng, n, 4, 6, t)
        doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)
        cases.append((doc, root, writes))
    set_root, set_keys, set_nodes = M._node_set(oracle, rng, suite.scale(3000, 90))
    fresh = []
    for doc, root, writes in cases:
        c = M._private_context(P)
        try:
            fresh.append(_json_of(P, oracle, doc, root, writes, c))
            assert _json_of(P, oracle, doc, root, writes, c)[1] == fresh[-1][1]  # the same call twice
        finally:
            c.close()
    ctx = M._private_context(P)
    try:
        def call(k):
            got, text = _json_of(P, oracle, *cases[k], ctx)
            A.arrays_equal(got, fresh[k][0])
            assert text == fresh[k][1], k

        call(0)
        call(1)
        A.arrays_equal(T._run(P, oracle, *cases[1], ctx)[0], fresh[1][0])
        call(0)
        w = P.stateless.StatelessWitness.parse_json(R.dumps(cases[1][0]))
        try:
            assert w.prestate_arrays(ctx, cases[1][1])["n_failed"] == 0
        finally:
            w.close()
        call(2)
        st = M._verify_set(P, oracle, ctx, set_root, set_keys, set_nodes)
        assert (st[:-8] == R.PRESENT).all()
        call(1)
        call(2)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 9. the run with the counted sizes
def test_nodes_beyond_the_estimate_are_counted_and_the_call_runs_again(P, oracle):
    from tests import test_gpu_prestate_more as M
    accounts, writes, extra, rng = _block(oracle, 33)
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)
    ctx = M._private_context(P)
    try:
        want = _json_of(P, oracle, doc, root, writes, ctx)
        for estimate in (300, 1):
            ctx.diag_set("advance_estimate_bytes", estimate)
            got = _json_of(P, oracle, doc, root, writes, ctx)
            A.arrays_equal(got[0], want[0])
            assert got[1] == want[1]
        ctx.diag_set("advance_estimate_bytes", 0)
        assert _json_of(P, oracle, doc, root, writes, ctx)[1] == want[1]
    finally:
        ctx.close()
