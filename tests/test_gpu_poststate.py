"""The post-state root of a stateless block (phant_exec_witness_poststate): the HIP pipeline against the reference's fixtures (known
answers) and against the full-state reference tests/poststate_ref.py (oracle.state_root over the complete post-state)."""
import ctypes as C

import numpy as np
import pytest

from tests import golden, suite
from tests import poststate_ref as Q
from tests import prestate_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _run(P, oracle, doc, root, writes, ctx=None):
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        info = w.info()
        got = w.poststate_arrays(ctx, root, Q.write_arrays(oracle, info, writes))
        return got, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in info.items()}
    finally:
        w.close()


def _check(P, oracle, accounts, writes, rng, tries=None, **kw):
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, tries=tries, **kw)
    got, info = _run(P, oracle, doc, root, writes)
    want = Q.expected(oracle, info, accounts, writes)
    assert got["n_failed"] == 0, (got["n_failed"], got["account_status"][:8], got["slot_status"][:8])
    assert got["state_root"] == want["state_root"], (got["state_root"].hex(), want["state_root"].hex())
    for k in ("storage_roots", "account_status", "slot_status"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1))[0][:8])
    return got, doc, root


def _acc(rng, storage=None, code=b""):
    return {"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1000)),
            "balance": int(rng.integers(0, 1 << 62)), "code": code, "storage": storage or {}}


def _val(rng):
    return int.from_bytes(rng.integers(0, 256, int(rng.integers(1, 33)), dtype=np.uint8).tobytes(), "big") or 1


# ---------------------------------------------------------------- 1. known answers
def test_fixture_post_state_roots(P, oracle):
    """Every fixture case with `post` and `post_state_root`: the witness of the genesis alloc for every address and slot of
    pre u post, the writes = the post alloc; the root must be the fixture's."""
    fx = golden.fixtures()
    cases = [c for c in fx["cases"] if c.get("post") and c.get("post_state_root")]
    assert len(cases) == 73
    cases = cases[:suite.scale(len(cases), 8)]
    rng = np.random.default_rng(1)
    kinds = {"insert": 0, "new_slot": 0, "changed": 0, "removed": 0}
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
            kinds["insert"] += addr not in by
            for s, v in st.items():
                o = int(old.get(s, 0))
                kinds["new_slot"] += bool(v and not o)
                kinds["changed"] += bool(v and o and v != o)
                kinds["removed"] += bool(o and not v)
        doc, root = Q.witness_doc(oracle, pre, writes, rng)
        assert root.hex() == c["genesis_state_root"], c["name"]
        got, _ = _run(P, oracle, doc, root, writes)
        assert got["n_failed"] == 0 and got["state_root"].hex() == c["post_state_root"], c["name"]
    if len(cases) == 73:
        assert kinds == {"insert": 105, "new_slot": 69, "changed": 1, "removed": 1}, kinds


# ---------------------------------------------------------------- 2. block-shaped states
def _block_case(oracle, rng, n_accounts, n_contracts, max_slots, n_touched):
    accounts = []
    for i in range(n_accounts):
        st = {int(rng.integers(0, 1 << 62)): _val(rng) for _ in range(int(rng.integers(1, max_slots + 1)))} if i < n_contracts else {}
        accounts.append(_acc(rng, st, rng.integers(0, 256, 40, dtype=np.uint8).tobytes() if i < n_contracts else b""))
    writes, extra = {}, {}
    touched = sorted(set(int(x) for x in rng.integers(0, n_accounts, n_touched)) | set(range(min(n_contracts, 12))))
    for t, i in enumerate(touched):
        a = accounts[i]
        kind = t % 10
        have = list(a["storage"])
        upd = {}
        for s in have[:6]:
            r = rng.random()
            if r < 0.4: upd[s] = _val(rng)          # a changed value
            elif r < 0.6: upd[s] = 0                # zeroed
            elif r < 0.7: upd[s] = a["storage"][s]  # a no-op write
        if have:
            upd[int(rng.integers(0, 1 << 62))] = _val(rng)  # a new slot
            upd[int(rng.integers(0, 1 << 62))] = 0          # a zero write to an absent slot
            extra[a["addr"]] = [int(rng.integers(0, 1 << 62))] + have[6:8]  # read only
        if have and t % 7 == 3:
            upd = {s: 0 for s in have}  # the last slot goes: the storage root becomes the empty root
        if kind == 0:
            writes[a["addr"]] = None
        elif kind in (1, 2) and upd:
            writes[a["addr"]] = ("keep", upd)
        elif kind == 3:
            writes[a["addr"]] = {"nonce": a["nonce"], "balance": a["balance"], "code": a["code"], "storage": {}}  # a no-op SET
        else:
            writes[a["addr"]] = {"nonce": a["nonce"] + 1, "balance": _val(rng), "code": a["code"], "storage": upd}
    for j in range(max(2, n_touched // 10)):
        n = _acc(rng)
        if j % 3 == 0:  # a contract created at an absent address, with slots
            n["code"] = b"\x60\x00" * (j + 1)
            n["storage"] = {int(rng.integers(0, 1 << 62)): _val(rng) for _ in range(3)}
        if j % 3 == 1:
            writes[n["addr"]] = None  # deleting what is not there
        else:
            writes[n["addr"]] = {k: n[k] for k in ("nonce", "balance", "code", "storage")}
    return accounts, writes, extra


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_block_shaped_states(P, oracle, seed):
    rng = np.random.default_rng(seed)
    accounts, writes, extra = _block_case(oracle, rng, suite.scale(1500, 150), suite.scale(40, 8), suite.scale(40, 9),
                                          suite.scale(300, 30))
    got, _, _ = _check(P, oracle, accounts, writes, rng, extra_slots=extra)
    assert (got["storage_roots"] == np.frombuffer(Q.EMPTY_ROOT, np.uint8)).all(1).any()


def test_twenty_thousand_touched_accounts(P, oracle):
    """beyond the small-trie sizes: 20 000 touched accounts of a larger state"""
    rng = np.random.default_rng(34)
    accounts, writes, extra = _block_case(oracle, rng, suite.scale(60_000, 1200), suite.scale(30, 4), 12, suite.scale(23_000, 450))
    assert len(writes) >= suite.scale(20_000, 400)
    _check(P, oracle, accounts, writes, rng, extra_slots=extra)


# ---------------------------------------------------------------- 3. structure
def _addr_with_prefix(oracle, want: str, start: int):
    """an address whose hashed key starts with the hex nibbles `want`"""
    i = start
    while True:
        a = i.to_bytes(20, "big")
        if oracle.keccak256(a).hex().startswith(want):
            return a
        i += 1


def _state(oracle, prefixes, start=1):
    rng = np.random.default_rng(len(prefixes))
    out = []
    for j, pfx in enumerate(prefixes):
        a = _acc(rng)
        a["addr"] = _addr_with_prefix(oracle, pfx, start + 1_000_000 * j)
        out.append(a)
    return out


def _new(rng, addr):
    return {"nonce": 1, "balance": int(rng.integers(1, 1 << 60)), "code": b"", "storage": {}}


def test_collapses_and_splits(P, oracle):
    rng = np.random.default_rng(40)
    # the root is an extension "ab" over a branch of two leaves: removing one collapses the branch onto a LEAF under the extension
    acc = _state(oracle, ["ab1", "ab2"])
    _check(P, oracle, acc, {acc[0]["addr"]: None}, rng)
    # ... removing both: the empty trie
    got, _, _ = _check(P, oracle, acc, {acc[0]["addr"]: None, acc[1]["addr"]: None}, rng)
    assert got["state_root"] == Q.EMPTY_ROOT
    # a branch of a leaf and of an extension "cd" over a branch: the leaf goes, the root becomes ONE extension (two merge; a branch
    # hangs under it)
    acc = _state(oracle, ["1", "7cd3", "7cd9"])
    _check(P, oracle, acc, {acc[0]["addr"]: None}, rng)
    # a branch of a leaf and a branch (no extension between): the survivor is a branch, it hangs under a new one-nibble extension
    acc = _state(oracle, ["1", "73", "79"])
    _check(P, oracle, acc, {acc[0]["addr"]: None}, rng)
    # cascade: "5" -> branch(5a -> leaf, 5b -> extension "cc" -> branch of two leaves); removing 5a and one of the two deep leaves
    # collapses two levels onto one leaf beside "1"
    acc = _state(oracle, ["1", "5a", "5bcc2", "5bcc8"])
    _check(P, oracle, acc, {acc[1]["addr"]: None, acc[3]["addr"]: None}, rng)
    _check(P, oracle, acc, {acc[0]["addr"]: None, acc[1]["addr"]: None, acc[3]["addr"]: None}, rng)
    # inserts that split the extension "abc" at its first, middle and last nibble, and beside a leaf
    acc = _state(oracle, ["abc1", "abc2"])
    for pfx in ("9", "a7", "ab0", "abc5", "abc1"):
        new = _addr_with_prefix(oracle, pfx, 77_000_000)
        if new == acc[0]["addr"]:
            continue
        _check(P, oracle, acc, {new: _new(rng, new)}, rng)
    # an insert and a removal under the same extension in one call
    new = _addr_with_prefix(oracle, "ab0", 78_000_000)
    _check(P, oracle, acc, {new: _new(rng, new), acc[0]["addr"]: None}, rng)
    # the same shapes inside a storage trie: an account whose slots share prefixes is found by search over slot numbers
    slots, want, s = {}, ["3a", "3b", "c"], 0
    while want:
        h = oracle.keccak256(s.to_bytes(32, "big")).hex()
        for w in list(want):
            if h.startswith(w):
                slots[s] = 5 + s
                want.remove(w)
        s += 1
    owner = _acc(rng, slots, b"\x01")
    acc = [owner, _acc(rng), _acc(rng)]
    ks = list(slots)
    for gone in ([ks[0]], [ks[0], ks[1]], [ks[2]], ks):
        got, _, _ = _check(P, oracle, acc, {owner["addr"]: ("keep", {s: 0 for s in gone})}, rng)
    assert (got["storage_roots"][0] == np.frombuffer(Q.EMPTY_ROOT, np.uint8)).all()


# ---------------------------------------------------------------- 4. thin and hostile witnesses
def _two_child_victims(oracle, accounts):
    """-> (accounts whose removal collapses a branch onto an untouched LEAF, accounts whose branch keeps >= 2 other children)"""
    hk = sorted((oracle.keccak256(a["addr"]).hex(), i) for i, a in enumerate(accounts))
    keys = [k for k, _ in hk]
    lcp = lambda a, b: next(j for j in range(65) if j == 64 or a[j] != b[j])  # noqa: E731
    lone, safe = [], []
    for p, (k, i) in enumerate(hk):
        d = max(lcp(k, keys[p - 1]) if p else 0, lcp(k, keys[p + 1]) if p + 1 < len(keys) else 0)
        n = sum(1 for x in keys if x[:d] == k[:d])
        kids = len({x[d] for x in keys if x[:d] == k[:d]})
        if n == 2:
            lone.append(i)
        elif kids >= 3:
            safe.append(i)
    return lone, safe


def test_witness_without_the_neighbour_proofs(P, oracle):
    rng = np.random.default_rng(50)
    accounts = [_acc(rng) for _ in range(suite.scale(400, 120))]
    lone, safe = _two_child_victims(oracle, accounts)
    # (two victims that do not share their branch, so that each one's sibling stays untouched)
    v1 = lone[0]
    k1 = oracle.keccak256(accounts[v1]["addr"]).hex()
    v2 = next(i for i in lone[1:] if oracle.keccak256(accounts[i]["addr"]).hex()[:2] != k1[:2])
    writes = {accounts[v1]["addr"]: None, accounts[v2]["addr"]: None, accounts[safe[0]]["addr"]: None,
              accounts[safe[1]]["addr"]: {"nonce": 9, "balance": 9, "code": b"", "storage": {}}}
    _check(P, oracle, accounts, writes, rng)  # with the neighbours: fine
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, neighbours=False)
    got, info = _run(P, oracle, doc, root, writes)
    addrs = [bytes(a) for a in info["addresses"]]
    want = np.array([Q.MISSING_SIBLING if a in (accounts[v1]["addr"], accounts[v2]["addr"]) else Q.PRESENT for a in addrs], np.uint8)
    assert np.array_equal(got["account_status"], want), (got["account_status"], want)
    assert got["n_failed"] == 2 and got["state_root"] == bytes(32) and not got["storage_roots"].any()


def test_hostile_witnesses(P, oracle):
    rng = np.random.default_rng(51)
    accounts, writes, extra = _block_case(oracle, rng, suite.scale(300, 80), 6, 8, suite.scale(40, 15))
    got, doc, root = _check(P, oracle, accounts, writes, rng, extra_slots=extra)
    # unreachable junk and duplicated nodes, any order: the same root
    junk = [R._hex(rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()) for n in (1, 33, 70, 532, 600)]
    other = Q.witness_doc(oracle, [_acc(rng) for _ in range(50)], {}, rng)[0]["state"]
    d = dict(doc, state=junk + doc["state"][::-1] + doc["state"][:7] + other)
    g2, _ = _run(P, oracle, d, root, writes)
    assert g2["state_root"] == got["state_root"] and g2["n_failed"] == 0
    assert np.array_equal(g2["storage_roots"], got["storage_roots"])
    # a wrong parent root: everything fails as in the pre-state call, no root
    g3, _ = _run(P, oracle, doc, bytes(31) + b"\x01", writes)
    assert (g3["account_status"] == Q.MISSING_NODE).all() and (g3["slot_status"] == Q.MISMATCH).all()
    assert g3["n_failed"] == len(g3["account_status"]) + len(g3["slot_status"]) and g3["state_root"] == bytes(32)
    # a damaged node: the statuses of the pre-state call, no root
    st = list(doc["state"])
    b = bytearray(R._unhex(st[3]))
    b[len(b) // 2] ^= 0x10
    st[3] = R._hex(bytes(b))
    d = dict(doc, state=st)
    g4, _ = _run(P, oracle, d, root, writes)
    pre = R.prestate_ref(oracle, d, root)
    assert pre["n_failed"] > 0 and g4["n_failed"] == pre["n_failed"] and g4["state_root"] == bytes(32)
    assert np.array_equal(g4["account_status"], pre["account_status"]) and np.array_equal(g4["slot_status"], pre["slot_status"])


def test_keep_on_an_absent_account_with_a_slot_write(P, oracle):
    rng = np.random.default_rng(52)
    accounts = [_acc(rng) for _ in range(40)]
    ghost = _acc(rng)["addr"]
    writes = {ghost: ("keep", {5: 7}), accounts[0]["addr"]: None}
    doc, root = Q.witness_doc(oracle, accounts, writes, rng)
    got, info = _run(P, oracle, doc, root, writes)
    k = [bytes(a) for a in info["addresses"]].index(ghost)
    assert got["account_status"][k] == Q.MISMATCH and got["n_failed"] == 1 and got["state_root"] == bytes(32)
    # with SET the account is created and its storage trie starts empty
    writes[ghost] = {"nonce": 0, "balance": 0, "code": b"", "storage": {5: 7}}
    _check(P, oracle, accounts, writes, rng)


# ---------------------------------------------------------------- 5. host path
def test_arguments_and_null_outputs(P, oracle):
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    from phant_amd.stateless import PoststateIO
    rng = np.random.default_rng(60)
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
    call = lambda c, h, r, o: lib.phant_exec_witness_poststate(c, h, r, C.byref(o) if o is not None else None)  # noqa: E731
    assert call(None, w._h, rb, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, None, rb, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, None, io()) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, None) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(struct_size=8)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(struct_size=C.sizeof(PoststateIO) + 8)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(account_op=None)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(nonces=None)) == L.E_INVALID_ARG
    assert call(ctx.handle, w._h, rb, io(slot_vals=None)) == L.E_INVALID_ARG
    bad = arr["account_op"].copy()
    bad[0] = 3
    assert call(ctx.handle, w._h, rb, io(account_op=bad.ctypes.data)) == L.E_INVALID_ARG
    # only the root wanted
    assert call(ctx.handle, w._h, rb, io()) == L.OK
    want = Q.expected(oracle, info, accounts, writes)
    assert out_root.tobytes() == want["state_root"]
    # nothing wanted at all
    o = io(state_root=None)
    assert call(ctx.handle, w._h, rb, o) == L.OK and o.n_failed == 0
    w.close()
    # no account among the keys: the root stays the parent's
    w = P.stateless.StatelessWitness.parse_json(R.dumps({"state": doc["state"], "keys": []}))
    got = w.poststate_arrays(None, root, {})
    assert got["state_root"] == root and got["n_failed"] == 0
    w.close()


def test_one_context_small_large_small(P, oracle):
    """Documents small -> large -> small on ONE private context with pre-state calls and node-set verifies of an unrelated larger set
    (whole, then damaged) in between: every result equals what a freshly created context gives and what the reference says."""
    from tests import test_gpu_prestate_more as M
    rng = np.random.default_rng(61)
    cases = []
    for n, t in ((40, 6), (suite.scale(3000, 400), suite.scale(500, 60)), (25, 5)):
        accounts, writes, extra = _block_case(oracle, rng, n, 4, 6, t)
        doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)
        cases.append((doc, root, writes, accounts))
    set_root, set_keys, set_nodes = M._node_set(oracle, rng, suite.scale(6000, 90))
    fresh = []
    for doc, root, writes, accounts in cases:
        c = M._private_context(P)
        try:
            got, info = _run(P, oracle, doc, root, writes, c)
        finally:
            c.close()
        want = Q.expected(oracle, info, accounts, writes)
        assert got["n_failed"] == 0 and got["state_root"] == want["state_root"]
        assert np.array_equal(got["storage_roots"], want["storage_roots"])
        fresh.append(got)
    ctx = M._private_context(P)
    try:
        def call(k):
            doc, root, writes, _ = cases[k]
            got, _ = _run(P, oracle, doc, root, writes, ctx)
            for key in ("state_root", "n_failed"):
                assert got[key] == fresh[k][key], (k, key)
            for key in ("storage_roots", "account_status", "slot_status"):
                assert np.array_equal(got[key], fresh[k][key]), (k, key)

        call(0)
        call(1)
        w = P.stateless.StatelessWitness.parse_json(R.dumps(cases[1][0]))
        try:
            assert w.prestate_arrays(ctx, cases[1][1])["n_failed"] == 0
        finally:
            w.close()
        call(0)
        st = M._verify_set(P, oracle, ctx, set_root, set_keys, set_nodes)
        assert (st[:-8] == R.PRESENT).all()
        call(2)
        damaged = list(set_nodes)
        for q in range(0, len(damaged), max(1, len(damaged) // 9)):
            b = bytearray(damaged[q])
            b[len(b) // 2] ^= 0x40
            damaged[q] = bytes(b)
        M._verify_set(P, oracle, ctx, set_root, set_keys, damaged[:-3])
        call(1)
        # a wrong parent root in between leaves nothing behind
        doc, root, writes, _ = cases[1]
        bad, _ = _run(P, oracle, doc, bytes(31) + b"\x02", writes, ctx)
        assert bad["state_root"] == bytes(32) and bad["n_failed"] > 0
        call(2)
        call(0)
    finally:
        ctx.close()


def _contract(rng, code):
    return _acc(rng, {int(s): int(s) + 7 for s in rng.integers(1, 1 << 40, 2)}, code)


def small_case(oracle, rng):
    """3 accounts and 4 slots among the keys of a state of ten: a KEEP with two slot writes, a SET with two, a DELETE.
    -> (doc, parent root, accounts, writes)"""
    accounts = [_contract(rng, b"\x01"), _contract(rng, b"\x02")] + [_acc(rng) for _ in range(8)]
    a, b = accounts[0], accounts[1]
    writes = {a["addr"]: ("keep", {list(a["storage"])[0]: 99, 12345: 6}),
              b["addr"]: {"nonce": b["nonce"] + 1, "balance": 5, "code": b["code"], "storage": {list(b["storage"])[1]: 3, 777: 8}},
              accounts[2]["addr"]: None}
    doc, root = Q.witness_doc(oracle, accounts, writes, rng)
    return doc, root, accounts, writes


def test_one_context_prestate_poststate_advance_interleaved(P, oracle):
    """The calls that share the pre-state stage (capi.hip: PrestateStage), interleaved on ONE private context over one witness of
    3 accounts, 4 slots and 2 codes: pre-state, post-state, advance, pre-state, post-state, with a witness of 40 accounts in between
    that grows the arena and the node-set workspace once.  Every result is what the same call gives on a fresh context (and what
    the references say); the second pre-state is the first.  What could go wrong here: pointers into the arena that went when it
    grew, the node-set epoch, the counters' four words against eight."""
    from tests import advance_ref as A
    from tests import test_gpu_prestate_more as M
    rng = np.random.default_rng(62)
    doc, root, accounts, writes = small_case(oracle, rng)
    doc = dict(doc, codes=[R._hex(accounts[0]["code"]), R._hex(accounts[1]["code"])])
    # (40 accounts with 30 slots each: more than the 1 024 nodes the node-set workspace starts with)
    many = [_acc(rng, {int(s): 1 + int(s) % 9 for s in rng.integers(1, 1 << 60, 30)}, b"\x03") for _ in range(40)] + [_acc(rng) for _ in range(20)]
    many_writes = {a["addr"]: ("keep", {s: v + 1 for s, v in a["storage"].items()}) for a in many[:40]}
    big_doc, big_root = Q.witness_doc(oracle, many, many_writes, rng)
    assert len(big_doc["state"]) > 1024 > len(doc["state"])

    def pre(d, r, ctx):
        return M._arrays(P, d, r, ctx)

    infos = {}

    def post(d, r, wr, ctx):
        got, infos[r] = _run(P, oracle, d, r, wr, ctx)
        return got

    def advance(ctx):
        w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
        nxt = None
        try:
            got, nxt = w.advance_arrays(ctx, root, Q.write_arrays(oracle, w.info(), writes))
            return got, nxt.to_json()
        finally:
            w.close()
            if nxt is not None:
                nxt.close()

    calls = {"pre": lambda c: pre(doc, root, c), "post": lambda c: post(doc, root, writes, c), "advance": advance,
             "big pre": lambda c: pre(big_doc, big_root, c), "big post": lambda c: post(big_doc, big_root, many_writes, c)}
    fresh = {}
    for name, call in calls.items():
        c = M._private_context(P)
        try:
            fresh[name] = call(c)
        finally:
            c.close()
    info = infos[root]
    assert (info["n_accounts"], info["n_slots"], info["n_codes"]) == (3, 4, 2) and infos[big_root]["n_accounts"] == 40
    M._same(fresh["pre"], R.prestate_ref(oracle, doc, root, strict=True), "fresh context")
    assert fresh["pre"]["n_failed"] == 0 and fresh["big pre"]["n_failed"] == 0 and len(fresh["big pre"]["account_status"]) == 40
    want = Q.expected(oracle, info, accounts, writes)
    for name in ("post", "advance"):
        got = fresh[name][0] if name == "advance" else fresh[name]
        assert got["n_failed"] == 0 and got["state_root"] == want["state_root"], name
        assert np.array_equal(got["storage_roots"], want["storage_roots"]), name
    assert fresh["big post"]["n_failed"] == 0 and fresh["big post"]["state_root"] == oracle.state_root(Q.apply_writes(many, many_writes))

    ctx = M._private_context(P)
    try:
        def same(name):
            got = calls[name](ctx)
            if name.endswith("pre"):
                M._same(got, fresh[name], "shared context, " + name)
            elif name == "advance":
                A.arrays_equal(got[0], fresh[name][0])
                assert got[1] == fresh[name][1]
            else:
                A.arrays_equal(got, fresh[name])
            return got

        first = same("pre")
        same("post")
        same("big pre")
        same("big post")
        same("advance")
        M._same(same("pre"), first, "the second pre-state against the first")
        same("post")
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3b. chosen trie keys (embedded nodes, 63 shared nibbles)
def _raw_case(P, oracle, pre_slots, upd, rng, neighbours=True):
    """One contract whose storage trie is keyed by the slots' 32 bytes VERBATIM (PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS), inside a
    state of ordinary accounts.  pre_slots / upd: {64 hex nibbles: value}; expected roots from oracle.mptize."""
    from phant_amd.context import default_context
    from tests.witness_util import _rlp_int
    owner = _acc(rng, {}, b"\x01\x02")
    others = [_acc(rng) for _ in range(12)]
    kv = sorted((bytes.fromhex(k), _rlp_int(v)) for k, v in pre_slots.items())
    stor = oracle.Trie([k for k, _ in kv], [v for _, v in kv])
    leaf = lambda sroot: R.account_leaf(oracle, owner, sroot)  # noqa: E731
    hashed = sorted([(oracle.keccak256(a["addr"]), R.account_leaf(oracle, a, Q.EMPTY_ROOT)) for a in others]
                    + [(oracle.keccak256(owner["addr"]), leaf(stor.root()))])
    state = oracle.Trie([k for k, _ in hashed], [v for _, v in hashed])
    nodes = {}
    for nd in state.prove(oracle.keccak256(owner["addr"])):
        nodes[nd] = None
    removed = {bytes.fromhex(k) for k, v in upd.items() if not v and k in pre_slots}
    want_keys = [bytes.fromhex(k) for k in upd]
    if neighbours:
        want_keys += list(Q._neighbours([k for k, _ in kv], removed))
    for k in want_keys:
        for nd in stor.prove(k):
            nodes[nd] = None
    keys = [R._hex(owner["addr"])] + [R._hex(owner["addr"] + bytes.fromhex(k)) for k in upd]
    doc = {"state": [R._hex(x) for x in nodes], "keys": keys}
    after = dict(pre_slots)
    after.update(upd)
    akv = sorted((bytes.fromhex(k), _rlp_int(v)) for k, v in after.items() if v)
    sroot = oracle.mptize([k for k, _ in akv], [v for _, v in akv]) if akv else Q.EMPTY_ROOT
    post = sorted([(k, v) for k, v in hashed if k != oracle.keccak256(owner["addr"])] + [(oracle.keccak256(owner["addr"]), leaf(sroot))])
    want_root = oracle.mptize([k for k, _ in post], [v for _, v in post])
    writes = {owner["addr"]: ("keep", {int(k, 16): v for k, v in upd.items()})}
    ctx = default_context()
    ctx.diag_set("poststate_raw_slot_keys", 1)
    try:
        got, _ = _run(P, oracle, doc, state.root(), writes)
    finally:
        ctx.diag_set("poststate_raw_slot_keys", 0)
    return got, sroot, want_root


def test_embedded_nodes_and_sixty_three_shared_nibbles(P, oracle):
    rng = np.random.default_rng(45)
    stem = "ab" + "0" * 61                 # 63 nibbles
    far = {"c" + "1" * 63: 7, "d" + "2" * 63: 0x1234}
    K1, K2, K3 = stem + "1", stem + "2", stem + "3"

    def ok(pre, upd):
        got, sroot, root = _raw_case(P, oracle, pre, upd, rng)
        assert got["n_failed"] == 0, (got["n_failed"], got["account_status"], got["slot_status"])
        assert got["storage_roots"][0].tobytes() == sroot and got["state_root"] == root
        return got

    # an insert beside a leaf that shares 63 nibbles: two three-byte leaves in a branch small enough to embed in its extension
    ok({**far, K1: 5}, {K2: 6})
    ok({K1: 5}, {K2: 6})                                 # ... the only leaf of the trie: the root becomes that extension
    # embedded children as survivors: the removed key's sibling is a leaf embedded in the branch, merged into a 64-nibble leaf
    ok({**far, K1: 5, K2: 6}, {K2: 0})
    ok({K1: 5, K2: 6}, {K1: 0})
    # ... as untouched neighbours that stay in their slots, and a removal that leaves two of three
    ok({**far, K1: 5, K2: 6, K3: 9}, {K2: 0x77})
    ok({**far, K1: 5, K2: 6, K3: 9}, {K3: 0})
    # a long value beside them: the embedded leaf next to a hashed one
    ok({**far, K1: 5, K2: (1 << 255) + 3}, {K1: 0})
    ok({**far, K1: 5, K2: (1 << 255) + 3}, {K2: 0})
    # an embedded leaf the key diverges from (an insert next to it, one nibble up) and a cascade that removes the whole stem
    ok({**far, K1: 5, K2: 6}, {"ab" + "0" * 60 + "10": 4})
    ok({**far, K1: 5, K2: 6}, {K1: 0, K2: 0})
    # splits of the 61-nibble extension at its first, middle and last nibble
    for at in (2, 30, 62):
        ok({**far, K1: 5, K2: 6}, {stem[:at] + "f" + "0" * (63 - at): 8})


# ---------------------------------------------------------------- 6. the hook
def test_new_payload_poststate_hook(P, oracle):
    fx = golden.fixtures()
    c = next(c for c in fx["cases"] if c.get("post") and c.get("post_state_root") and len(c["post"]) > len(c["pre"]))
    pre = golden.accounts_of(c["pre"], fx["codes"])
    post = golden.accounts_of(c["post"], fx["codes"])
    by = {a["addr"]: a for a in pre}
    after = {a["addr"]: P.state.AccountState(addr=a["addr"], nonce=a["nonce"], balance=a["balance"], code=a["code"],
                                             storage=dict(a["storage"])) for a in post}
    for a in pre:
        after.setdefault(a["addr"], None)
    writes = {addr: (None if s is None else {"nonce": s.nonce, "balance": s.balance, "code": s.code,
                                             "storage": {k: s.storage.get(k, 0) for k in set(s.storage) | set(by.get(addr, {"storage": {}})["storage"])}})
              for addr, s in after.items()}
    doc, root = Q.witness_doc(oracle, pre, writes, np.random.default_rng(70))
    header = bytes.fromhex(c["post_state_root"])
    got = P.stateless.new_payload_poststate(R.dumps(doc), root, after, header)
    assert got.ok and got.root == header
    off = bytearray(header)
    off[31] ^= 1
    with pytest.raises(P.stateless.PoststateError):
        P.stateless.new_payload_poststate(R.dumps(doc), root, after, bytes(off))
