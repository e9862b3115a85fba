"""phant_exec_witness_prestate where tests/test_gpu_prestate.py samples a handful of points: the strict leaf decoders on whole corpora
of mutated bodies against a reference written from the RLP specification (one launch each), the code hashing at every length,
alignment and pairing and in both forms of its sponge, the digest table under thousands of duplicates, calls that share one
context with each other and with phant_mpt_verify_nodeset, degenerate documents and absent output pointers.  Every expectation
comes from tests/prestate_ref.py (the oracle's walks, oracle.keccak256, rlp_decode_strict); tests/test_emu_prestate.py runs the same
bodies on the emulated library at the sizes suite.scale gives it."""
import ctypes as C

import numpy as np
import pytest

from tests import suite
from tests import prestate_ref as R
from tests.witness_util import _rlp_int, _rlp_list, _rlp_str, random_kv

pytestmark = pytest.mark.gpu

ARRAYS = ("account_status", "nonces", "balances", "storage_roots", "code_hashes", "code_index", "slot_status", "slot_vals")
COUNTS = ("n_failed", "n_missing_code", "n_unused_codes")
MISSING_NODE = 20


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _arrays(P, doc, root, ctx=None):
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        return w.prestate_arrays(ctx, root)
    finally:
        w.close()


def _same(got, want, what=""):
    for k in ARRAYS:
        g, w = np.asarray(got[k]).reshape(np.asarray(want[k]).shape), np.asarray(want[k])
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {k} differs in {len(rows)} of {len(w)} rows, first {rows[:8].tolist()}: "
                                 f"got {g[rows[0]].tolist()} want {w[rows[0]].tolist()}")
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def _private_context(P):
    """a context of its own, next to the default one (on the emulated library while that is loaded)"""
    if suite.EMULATED:
        from phant_amd import _lib as L
        from tests import emu
        return emu.mirror_context(L.lib())
    return P.context.Context()


class _code_hash_form:
    def __init__(self, form):
        from phant_amd.context import default_context
        self.ctx, self.form = default_context(), form

    def __enter__(self):
        self.ctx.diag_set("code_hash_form", self.form)

    def __exit__(self, *exc):
        self.ctx.diag_set("code_hash_form", 0)


# ---------------------------------------------------------------- the strict decoders, one launch per corpus
def test_account_leaf_corpus(P, oracle):
    """Every body of prestate_ref.leaf_corpus as a leaf of ONE state trie: PRESENT with the decoded fields or BAD_VALUE with the
    empty account, as rlp_decode_strict + account_of_item say; slots under BAD_VALUE accounts MISMATCH."""
    corpus = R.leaf_corpus(np.random.default_rng(41), suite.scale(3, 32))
    # the conditions on the corpus, by the reference alone
    fam, n_ok, n_bad = R.families(corpus, R.strict_account)
    print(f"account corpus: {len(corpus)} bodies, {n_ok} PRESENT, {n_bad} BAD_VALUE")
    assert len(corpus) >= suite.scale(2000, 300) and 4 * n_ok >= len(corpus) and 4 * n_bad >= len(corpus)
    assert fam == R.LEAF_FAMILIES, fam
    assert any(0xC0 <= b[0] <= 0xF7 and len(b) > 1 for _, b in corpus)  # the kernel's short-list branch is reached
    leaves = {R.address(i): body for i, (_, body) in enumerate(corpus)}
    t, nodes = R.state_of_leaves(oracle, leaves)  # (raises where the trie cannot carry a body: no body is filtered)
    keys = []
    for i in range(len(corpus)):
        keys.append(R._hex(R.address(i)))
        if i % 5 == 0:
            keys.append(R._hex(R.address(i) + (i + 1).to_bytes(32, "big")))
    doc = {"state": [R._hex(x) for x in nodes], "keys": keys}
    want = R.prestate_ref(oracle, doc, t.root(), strict=True)
    assert len(want["account_status"]) == len(corpus) and len(want["slot_status"]) == (len(corpus) + 4) // 5
    got = _arrays(P, doc, t.root())
    j = 0
    for i, (name, body) in enumerate(corpus):
        acc = R.strict_account(body)
        st = int(got["account_status"][i])
        assert st == (R.PRESENT if acc else R.BAD_VALUE), (name, body.hex(), st)
        nonce, bal, sr, ch = acc or (0, 0, R.EMPTY_ROOT, R.EMPTY_CODE)
        have = (int(got["nonces"][i]), int.from_bytes(got["balances"][i].tobytes(), "big"), got["storage_roots"][i].tobytes(),
                got["code_hashes"][i].tobytes())
        assert have == (nonce, bal, sr, ch), (name, body.hex(), have)
        if i % 5 == 0:
            if acc is None:
                assert got["slot_status"][j] == R.MISMATCH, (name, int(got["slot_status"][j]))
            else:  # (no storage node in the set: the empty root proves absence, any other root leads nowhere)
                assert got["slot_status"][j] == (R.ABSENT if sr == R.EMPTY_ROOT else MISSING_NODE), (name, int(got["slot_status"][j]))
            j += 1
    _same(got, want, "account corpus")
    assert got["n_failed"] == n_bad + int((want["slot_status"] != R.ABSENT).sum())


def test_slot_value_corpus(P, oracle):
    """prestate_ref.slot_corpus as the leaves of one storage trie under one good account: every width 1 .. 32 comes back as its
    value, every other form is BAD_VALUE with a zero word."""
    corpus = R.slot_corpus(np.random.default_rng(42))
    fam, n_ok, n_bad = R.families(corpus, R.strict_slot)
    print(f"slot corpus: {len(corpus)} values, {n_ok} PRESENT, {n_bad} BAD_VALUE")
    assert fam == R.SLOT_FAMILIES and n_ok == 4 * 32 and n_bad >= 20
    pre = [(j + 1).to_bytes(32, "big") for j in range(len(corpus))]
    skv = sorted((oracle.keccak256(p), v) for p, (_, v) in zip(pre, corpus))
    stor = oracle.Trie([k for k, _ in skv], [v for _, v in skv])
    owner, other = R.address(1), R.address(2)
    t, nodes = R.state_of_leaves(oracle, {owner: _rlp_list([_rlp_int(1), _rlp_int(2), _rlp_str(stor.root()), _rlp_str(R.EMPTY_CODE)]),
                                          other: _rlp_list([_rlp_int(3), _rlp_int(4), _rlp_str(R.EMPTY_ROOT), _rlp_str(R.EMPTY_CODE)])})
    for k, _ in skv:
        for nd in stor.prove(k):
            nodes[nd] = None
    absent = (10_000).to_bytes(32, "big")
    for nd in stor.prove(oracle.keccak256(absent)):
        nodes[nd] = None
    doc = {"state": [R._hex(x) for x in nodes], "keys": [R._hex(owner + p) for p in pre] + [R._hex(owner + absent), R._hex(other)]}
    want = R.prestate_ref(oracle, doc, t.root(), strict=True)
    got = _arrays(P, doc, t.root())
    assert got["account_status"].tolist() == [R.PRESENT, R.PRESENT]
    for j, (name, v) in enumerate(corpus):
        val = R.strict_slot(v)
        st, word = int(got["slot_status"][j]), int.from_bytes(got["slot_vals"][j].tobytes(), "big")
        assert (st, word) == ((R.PRESENT, val) if val is not None else (R.BAD_VALUE, 0)), (name, v.hex(), st, hex(word))
    assert got["slot_status"][len(corpus)] == R.ABSENT and not got["slot_vals"][len(corpus)].any()
    _same(got, want, "slot corpus")
    assert got["n_failed"] == n_bad


# ---------------------------------------------------------------- code hashing
def _code_lengths(rng):
    top = suite.scale(3 * 136 + 9, 136 + 9)
    lens = list(range(top + 1)) + [int(x) for x in rng.permutation(top + 1)]
    lens += [k * 136 + r for k in suite.scale((7, 63, 180), (7,)) for r in (0, 1, 7, 8, 127, 128, 134, 135)]
    lens += suite.scale([24_576], [])  # (the emulated run has that length in test_codes)
    if len(lens) % 2 == 0:
        lens.append(137)
    return lens


@pytest.mark.parametrize("form", [0, 1])
def test_code_lengths_sweep(P, oracle, form):
    """Codes of every length 0 .. 3 * 136 + 9 in ascending and in shuffled order (the halves of a wave then differ in block count),
    long ones at every residue that matters mod 8 and mod 136, the longest a contract may be; concatenated as they come (every
    start alignment), an odd count (the last half wave has no partner).  One account per code finds it; accounts that carry the
    digest of a code with its last byte flipped or with one zero byte appended find nothing."""
    rng = np.random.default_rng(50 + form)
    lens = _code_lengths(rng)
    assert len(lens) % 2 == 1 and set(x % 8 for x in np.cumsum(lens)) == set(range(8))
    codes = [rng.bytes(n) for n in lens]
    first, dig = R.first_index(oracle, codes)
    assert len(first) >= len(codes) - 3  # (the two empty codes are equal, one-byte codes may be)
    near = []
    for c in codes:
        if c:
            near.append(oracle.keccak256(c[:-1] + bytes([c[-1] ^ 0x01])))
        near.append(oracle.keccak256(c + b"\x00"))
    owners = list(dig) + near
    doc, root = R.code_owner_doc(oracle, codes, owners)
    want = R.prestate_ref(oracle, doc, root, strict=True)
    with _code_hash_form(form):
        got = _arrays(P, doc, root)
    assert (got["account_status"] == R.PRESENT).all()
    wrong = [(i, lens[i], int(got["code_index"][i]), first[dig[i]]) for i in range(len(codes)) if got["code_index"][i] != first[dig[i]]
             and dig[i] != R.EMPTY_CODE]
    assert not wrong, f"(code, its length, code_index, expected) {wrong[:12]} ... {len(wrong)} codes"
    for i, d in enumerate(owners):
        exp = R.CODE_NONE if d == R.EMPTY_CODE else first.get(d, R.CODE_NONE)
        assert got["code_index"][i] == exp, (i, int(got["code_index"][i]), exp)
    _same(got, want, f"code lengths, form {form}")
    n_none = sum(1 for d in near if d not in first)
    assert n_none >= len(near) - 4 and got["n_missing_code"] == n_none
    assert got["n_unused_codes"] == 2  # (the two empty codes: no account names keccak256("") as a code to look up)


CODE_COUNTS = (2047, 2048, 2049, 4100)


def code_count_case(P, oracle, nc):
    """code_hash_kernel's sponge takes theta's column in one trip while the launch has at most a wave per SIMD (nc <= 2048) and in
    two beyond: both sides of the switch, all codes distinct, each owned by one account, all found."""
    rng = np.random.default_rng(nc)
    top = suite.scale(300, 100)
    codes = [rng.bytes(int(n)) + k.to_bytes(2, "big") for k, n in enumerate(rng.integers(0, top - 1, nc))]
    first, dig = R.first_index(oracle, codes)
    assert len(first) == nc
    # (the emulated run hashes every code but keeps the state around them small: every 16th code and the last nine are owned)
    own = list(range(nc)) if not suite.EMULATED or suite.FULL else sorted(set(range(0, nc, 16)) | set(range(nc - 9, nc)))
    doc, root = R.code_owner_doc(oracle, codes, [dig[k] for k in own])
    got = _arrays(P, doc, root)
    wrong = [(k, len(codes[k]), int(got["code_index"][i])) for i, k in enumerate(own) if got["code_index"][i] != k]
    assert not wrong, f"(code, its length, code_index) {wrong[:12]} ... {len(wrong)} of {nc}"
    _same(got, R.prestate_ref(oracle, doc, root, strict=True), f"{nc} codes")
    assert got["n_missing_code"] == 0 and got["n_unused_codes"] == nc - len(own) and got["n_failed"] == 0


@pytest.mark.parametrize("nc", CODE_COUNTS)
def test_code_count_switches_sponge_variant(P, oracle, nc):
    code_count_case(P, oracle, nc)


# ---------------------------------------------------------------- the digest table
def _flood(oracle, codes, rng):
    """the witness of `codes` with one account per distinct digest (a sample of max_owners where there are more) plus one account
    per sampled duplicate copy: every owner's code_index is the LOWEST index of its digest"""
    first, dig = R.first_index(oracle, codes)
    distinct, max_owners = list(first), suite.scale(4000, 40)  # (the state around the codes is what costs host and emulator time)
    if len(distinct) > max_owners:
        distinct = [distinct[i] for i in sorted(rng.choice(len(distinct), max_owners, replace=False))]
    owners = distinct + [dig[int(k)] for k in rng.integers(0, len(codes), min(len(codes), suite.scale(64, 8)))]
    doc, root = R.code_owner_doc(oracle, codes, owners)
    want = R.prestate_ref(oracle, doc, root, strict=True)
    owned = set(owners)
    assert want["n_unused_codes"] == sum(1 for d in dig if d not in owned) and want["n_missing_code"] == 0
    return doc, root, want, [first[d] for d in owners]


def _check_flood(P, doc, root, want, lowest, what):
    got = _arrays(P, doc, root)
    wrong = [(i, int(got["code_index"][i]), lowest[i]) for i in range(len(lowest)) if got["code_index"][i] != lowest[i]]
    assert not wrong, f"{what}: (account, code_index, the lowest index of its digest) {wrong[:12]} ... {len(wrong)} accounts"
    _same(got, want, what)


def test_duplicate_code_floods(P, oracle):
    """code_insert under contention: ~130 copies of each of 300 codes in shuffled order, every code identical, all distinct, and
    counts at the table's sizing boundaries, under both forms of the hash kernel; the lowest index of a digest wins and unused
    copies are counted one by one.  The emulator runs workgroups one after another (it sees a wrong order of indices, not a race):
    the concurrent case is the GPU run's."""
    rng = np.random.default_rng(77)
    nc = suite.scale(40_000, 256)
    pool = [rng.bytes(int(n)) for n in rng.integers(1, suite.scale(300, 130), 300)]
    cases = [("copies of 300 codes", [pool[int(k)] for k in rng.integers(0, 300, nc)]),
             ("one code", [pool[0]] * nc),
             ("all distinct", [rng.bytes(int(n)) + k.to_bytes(3, "big") for k, n in enumerate(rng.integers(0, suite.scale(200, 100), nc))])]
    for n in suite.scale((31, 32, 33, 64, 65), (32, 33)):  # code_table_slots: 64 slots up to 32 codes, 128 up to 64, 256 from 65
        cases.append((f"{n} distinct", [rng.bytes(20) + bytes([k]) for k in range(n)]))
        if n != 32 or not suite.EMULATED:
            cases.append((f"{n} in pairs", [b"a code that comes twice" + bytes([k // 2]) for k in range(n)]))
    for what, codes in cases:
        built = _flood(oracle, codes, rng)
        repeats = suite.scale(3, 1) if len(codes) == nc and what != "all distinct" else 1
        for form in (0, 1):
            with _code_hash_form(form):
                for r in range(repeats):  # (the table memsets and the helper stream's join are crossed again on the same ctx)
                    _check_flood(P, *built, f"{what}, form {form}, call {r}")


# ---------------------------------------------------------------- one context, many calls
def _node_set(oracle, rng, n):
    keys, vals = random_kv(rng, n, val_min=1, val_max=60)
    t = oracle.Trie(keys, vals)
    nodes = {}
    for k in keys:
        for nd in t.prove(k):
            nodes[nd] = None
    absent = [rng.bytes(32) for _ in range(8)]
    for k in absent:
        for nd in t.prove(k):
            nodes[nd] = None
    uniq = [x for x in nodes]
    uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    return t.root(), keys + absent, uniq


def _verify_set(P, oracle, ctx, root, keys, nodes):
    blob = np.frombuffer(b"".join(nodes), np.uint8).copy()
    off = np.zeros(len(nodes) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in nodes])
    r, karr = np.frombuffer(root, np.uint8).copy(), np.frombuffer(b"".join(keys), np.uint8).copy()
    got = P.mpt.verify_nodeset(r, None, karr, 32, blob, off, ctx=ctx)
    want = oracle.mpt_verify_nodeset(r, None, karr, 32, blob, off)
    assert np.array_equal(got[0], want[0]), (got[0][:16], want[0][:16])
    ok = want[0] == R.PRESENT
    assert np.array_equal(got[1][ok], want[1][ok]) and np.array_equal(got[2][ok], want[2][ok])
    return want[0]


def test_calls_share_one_context(P, oracle):
    """Documents small -> large -> small on one private context, a call with a wrong trusted root, a call the library refuses and
    node-set verifies of an unrelated larger set (whole, then damaged) in between: the node-set workspace, its epoch, the grown
    buffers and the helper stream carry nothing over -- every result is what a fresh context gives and what the reference says."""
    rng = np.random.default_rng(90)
    small = R.block_witness_doc(oracle, rng, n_accounts=20, n_contracts=suite.scale(3, 1), max_slots=5, n_touched=6, slots_per=3, n_absent=2)[:2]
    large = R.block_witness_doc(oracle, rng, n_accounts=suite.scale(1500, 50), n_contracts=suite.scale(40, 2), max_slots=suite.scale(60, 8),
                                n_touched=suite.scale(300, 12), slots_per=suite.scale(8, 3), n_absent=suite.scale(30, 4))[:2]
    small2 = R.block_witness_doc(oracle, rng, n_accounts=40, n_contracts=suite.scale(4, 2), max_slots=6, n_touched=10, slots_per=2, n_absent=3)[:2]
    set_root, set_keys, set_nodes = _node_set(oracle, rng, suite.scale(6000, 90))
    assert len(set_nodes) > max(len(d["state"]) for d, _ in (small, large, small2))
    bad_root = bytes(31) + b"\x02"
    fresh = {}
    for name, (doc, root) in (("small", small), ("large", large), ("small2", small2), ("wrong root", (large[0], bad_root))):
        c = _private_context(P)
        try:
            fresh[name] = _arrays(P, doc, root, c)
        finally:
            c.close()
        _same(fresh[name], R.prestate_ref(oracle, doc, root, strict=True), "fresh context, " + name)
    assert (fresh["wrong root"]["account_status"] == MISSING_NODE).all() and fresh["large"]["n_failed"] == 0
    ctx = _private_context(P)
    try:
        def call(name, doc, root):
            _same(_arrays(P, doc, root, ctx), fresh[name], "shared context, " + name)

        call("small", *small)
        call("large", *large)
        call("wrong root", large[0], bad_root)
        call("small", *small)
        st = _verify_set(P, oracle, ctx, set_root, set_keys, set_nodes)
        assert (st[:-8] == R.PRESENT).all() and (st[-8:] == R.ABSENT).all()
        call("small2", *small2)
        damaged = list(set_nodes)
        for j in range(0, len(damaged), max(1, len(damaged) // 9)):
            b = bytearray(damaged[j])
            b[len(b) // 2] ^= 0x40
            damaged[j] = bytes(b)
        st = _verify_set(P, oracle, ctx, set_root, set_keys, damaged[:-3])
        assert (st != R.PRESENT).any()
        call("large", *large)
        # a call the library refuses (no trusted root) leaves nothing behind
        w = P.stateless.StatelessWitness.parse_json(R.dumps(small[0]))
        try:
            o = P.stateless.PrestateOut()
            o.struct_size = C.sizeof(P.stateless.PrestateOut)
            assert ctx._lib.phant_exec_witness_prestate(ctx.handle, w._h, None, C.byref(o)) == -1
        finally:
            w.close()
        call("small", *small)
        call("wrong root", large[0], bad_root)
        call("small2", *small2)
        st = _verify_set(P, oracle, ctx, set_root, set_keys, set_nodes)
        assert (st[:-8] == R.PRESENT).all()
    finally:
        ctx.close()


def test_degenerate_documents(P, oracle):
    rng = np.random.default_rng(91)
    doc, root, accounts = R.block_witness_doc(oracle, rng, n_accounts=30, n_contracts=suite.scale(4, 2), max_slots=6, n_touched=8, slots_per=3, n_absent=2)
    codes = doc["codes"]

    def run(d, r=root):
        got = _arrays(P, d, r)
        _same(got, R.prestate_ref(oracle, d, r, strict=True), str({k: len(v) for k, v in d.items()}))
        return got

    # no keys at all: the codes are still hashed, every one of them unused
    got = run({"state": doc["state"], "codes": codes, "keys": []})
    assert len(got["account_status"]) == 0 and len(got["slot_status"]) == 0
    assert (got["n_failed"], got["n_missing_code"], got["n_unused_codes"]) == (0, 0, len(codes))
    got = run({"state": [], "codes": codes + codes, "keys": []})
    assert got["n_unused_codes"] == 2 * len(codes)
    # nothing at all
    got = run({"state": [], "keys": []})
    assert (got["n_failed"], got["n_missing_code"], got["n_unused_codes"]) == (0, 0, 0)
    got = run({"state": [], "codes": [], "keys": []})
    assert (got["n_failed"], got["n_missing_code"], got["n_unused_codes"]) == (0, 0, 0)
    # only 52-byte keys: their accounts are implied
    only52 = [k for k in doc["keys"] if len(k) == 2 + 104]
    assert only52
    got = run({"state": doc["state"], "codes": codes, "keys": only52})
    want_all = R.prestate_ref(oracle, doc, root, strict=True)
    assert len(got["account_status"]) == len(set(k[:42] for k in only52)) and len(got["slot_status"]) == len(set(only52))
    assert (got["account_status"] != MISSING_NODE).all() and sorted(got["slot_status"].tolist()) == sorted(want_all["slot_status"].tolist())
    # no nodes: nothing hashes to the root, no slot is anchored
    got = run({"state": [], "codes": codes, "keys": doc["keys"]})
    assert (got["account_status"] == MISSING_NODE).all() and (got["slot_status"] == R.MISMATCH).all()
    assert got["n_failed"] == len(got["account_status"]) + len(got["slot_status"]) and got["n_unused_codes"] == len(codes)
    assert got["n_missing_code"] == 0 and (got["code_index"] == R.CODE_NONE).all()
    # ... unless the trusted root is the empty trie's: every account is proven absent by it
    got = run({"state": [], "codes": codes, "keys": doc["keys"]}, R.EMPTY_ROOT)
    assert (got["account_status"] == R.ABSENT).all() and (got["slot_status"] == R.ABSENT).all() and got["n_failed"] == 0
    # the same keys many times, in any order
    many = [doc["keys"][int(i)] for i in rng.integers(0, len(doc["keys"]), 40 * len(doc["keys"]))]
    got = run({"state": doc["state"], "codes": codes, "keys": many})
    assert len(got["account_status"]) <= len(want_all["account_status"]) and len(got["slot_status"]) <= len(want_all["slot_status"])
    one = [k for k in doc["keys"] if len(k) == 2 + 104][0]
    got = run({"state": doc["state"], "codes": codes, "keys": [one] * 300 + [one[:42]] * 300})
    assert len(got["account_status"]) == 1 and len(got["slot_status"]) == 1
    # codes, and every account absent
    state, _, _ = R.build_tries(oracle, accounts)
    nodes, keys = {}, []
    for _ in range(12):
        a = rng.bytes(20)
        keys += [R._hex(a), R._hex(a + rng.bytes(32))]
        for nd in state.prove(oracle.keccak256(a)):
            nodes[nd] = None
    got = run({"state": [R._hex(x) for x in nodes], "codes": codes, "keys": keys})
    assert (got["account_status"] == R.ABSENT).all() and (got["slot_status"] == R.ABSENT).all()
    assert (got["n_failed"], got["n_missing_code"], got["n_unused_codes"]) == (0, 0, len(codes))
    assert (got["code_index"] == R.CODE_NONE).all()


def test_null_outputs(P, oracle):
    """The C entry point itself: each output pointer NULL ("not wanted") in turn and all of them at once leave the counts and the
    other arrays as they are; a short struct_size and a NULL root are PHANT_E_INVALID_ARG and the context works on."""
    from phant_amd import _lib as L
    from phant_amd.context import default_context
    S = P.stateless
    rng = np.random.default_rng(92)
    accounts = [{"addr": R.address(i), "nonce": i, "balance": 1 << (9 * i), "code": rng.bytes(20 + i) if i % 2 else b"",
                 "storage": {int(s): int(s) + 1 for s in rng.integers(1, 1 << 40, i % 4)}} for i in range(12)]
    doc, root = R.full_witness(oracle, accounts, rng, extra_keys=[R._hex(rng.bytes(20)), R._hex(R.address(3) + bytes(32))])
    doc["codes"] = doc["codes"][::2] + [R._hex(b"\x60\x00")]  # (missing codes and an unused one: no count is zero by accident)
    st = list(doc["state"])
    doc["state"] = st[:len(st) // 2] + st[len(st) // 2 + 1:]  # (and a node is gone)
    want = R.prestate_ref(oracle, doc, root, strict=True)
    assert want["n_failed"] and want["n_missing_code"] and want["n_unused_codes"]
    ctx, lib = default_context(), L.lib()
    w = S.StatelessWitness.parse_json(R.dumps(doc))
    try:
        i = w.info()
        na, ns = i["n_accounts"], i["n_slots"]
        shapes = {"account_status": ((na,), np.uint8), "nonces": ((na,), np.uint64), "balances": ((na, 32), np.uint8),
                  "storage_roots": ((na, 32), np.uint8), "code_hashes": ((na, 32), np.uint8), "code_index": ((na,), np.uint32),
                  "slot_status": ((ns,), np.uint8), "slot_vals": ((ns, 32), np.uint8)}
        rootbuf = C.create_string_buffer(root, 32)

        def call(leave_out=(), struct_size=None, root_arg=rootbuf):
            bufs = {k: np.full(int(np.prod(s)) * np.dtype(d).itemsize, 0xEE, np.uint8).view(d).reshape(s)
                    for k, (s, d) in shapes.items()}
            o = S.PrestateOut()
            o.struct_size = C.sizeof(S.PrestateOut) if struct_size is None else struct_size
            for k, a in bufs.items():
                setattr(o, k, None if k in leave_out else a.ctypes.data)
            o.n_failed = o.n_missing_code = o.n_unused_codes = 0xEEEE
            rc = lib.phant_exec_witness_prestate(ctx.handle, w._h, root_arg, C.byref(o))
            return rc, bufs, (int(o.n_failed), int(o.n_missing_code), int(o.n_unused_codes))

        rc, full, counts = call()
        assert rc == L.OK
        _same({**full, **dict(zip(COUNTS, counts))}, want, "all outputs")
        for leave_out in [(k,) for k in ARRAYS] + [ARRAYS, ARRAYS[:4], ARRAYS[4:]]:
            rc, bufs, cnt = call(leave_out)
            assert rc == L.OK and cnt == counts, (leave_out, rc, cnt)
            for k in ARRAYS:
                if k in leave_out:
                    assert (bufs[k].view(np.uint8) == 0xEE).all(), k  # (ours: untouched)
                else:
                    assert np.array_equal(bufs[k], full[k]), (leave_out, k)
        for kw in (dict(struct_size=C.sizeof(S.PrestateOut) - 4), dict(struct_size=0), dict(root_arg=None)):
            rc, bufs, cnt = call(**kw)
            assert rc == L.E_INVALID_ARG, (kw, rc)
            assert all((bufs[k].view(np.uint8) == 0xEE).all() for k in ARRAYS)
        assert lib.phant_exec_witness_prestate(ctx.handle, w._h, rootbuf, None) == L.E_INVALID_ARG
        assert lib.phant_exec_witness_prestate(ctx.handle, None, rootbuf, C.byref(S.PrestateOut())) == L.E_INVALID_ARG
        rc, again, cnt = call()
        assert rc == L.OK and cnt == counts and all(np.array_equal(again[k], full[k]) for k in ARRAYS)
    finally:
        w.close()
