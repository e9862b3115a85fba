"""The pre-state of an execution witness (phant_exec_witness_prestate): the HIP pipeline against the reference's genesis / post allocs
(known answers) and against the CPU reference tests/prestate_ref.py (the oracle's node-set walk twice, the leaves decoded in Python)."""
import numpy as np
import pytest

from tests import golden, suite
from tests import prestate_ref as R
from tests.witness_util import _rlp_int, _rlp_list, _rlp_str

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _run(P, doc, root):
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        return w.prestate_arrays(None, root), w.prestate(None, root)
    finally:
        w.close()


def _same(got, want):
    for k in ("account_status", "nonces", "balances", "storage_roots", "code_hashes", "code_index", "slot_status", "slot_vals"):
        assert np.array_equal(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k]), (k, got[k][:8], want[k][:8])
    for k in ("n_failed", "n_missing_code", "n_unused_codes"):
        assert got[k] == want[k], (k, got[k], want[k])


def _alloc_cases():
    fx = golden.fixtures()
    out = []
    for c in fx["cases"]:
        out.append((c["name"] + "/pre", c["pre"], c["genesis_state_root"]))
        if c.get("post") and c.get("post_state_root"):
            out.append((c["name"] + "/post", c["post"], c["post_state_root"]))
    return fx, out


def test_golden_allocs_are_known_answers(P, oracle):
    """Every genesis `pre` and `post` alloc of the reference's fixtures as a full witness (all nodes of the state trie and of every
    storage trie, shuffled; all codes; every key): every account PRESENT, the pre-state IS the alloc, and its state root is the
    fixture's."""
    fx, cases = _alloc_cases()
    cases = cases[:suite.scale(len(cases), 6)]
    rng = np.random.default_rng(5)
    n_pre = sum(1 for n, _, _ in cases if n.endswith("/pre"))
    assert n_pre == suite.scale(84, n_pre) and len(cases) == suite.scale(157, len(cases))
    for name, alloc, root_hex in cases:
        acc = golden.accounts_of(alloc, fx["codes"])
        doc, root = R.full_witness(oracle, acc, rng)
        assert root.hex() == root_hex, name
        got, pre = _run(P, doc, root)
        assert pre.ok and got["n_missing_code"] == 0, name
        assert (got["account_status"] == R.PRESENT).all(), name
        assert len(pre.accounts) == len(acc), name
        for a, g in zip(acc, pre.accounts):
            assert g.addr == a["addr"] and g.nonce == a["nonce"] and g.balance == a["balance"] and g.code == a["code"], name
            assert g.storage == {k: v for k, v in a["storage"].items() if v}, name
        assert P.state.state_root(pre.accounts).hex() == root_hex, name


@pytest.mark.parametrize("shape", ["block", "small"])
def test_block_witness_matches_the_reference(P, oracle, shape):
    rng = np.random.default_rng(11 if shape == "block" else 12)
    if shape == "block":
        kw = dict(n_accounts=suite.scale(1500, 120), n_contracts=suite.scale(40, 6), max_slots=suite.scale(60, 12),
                  n_touched=suite.scale(300, 25), slots_per=suite.scale(8, 4), n_absent=suite.scale(30, 5))
    else:
        kw = dict(n_accounts=20, n_contracts=3, max_slots=5, n_touched=6, slots_per=3, n_absent=2)
    doc, root, _ = R.block_witness_doc(oracle, rng, **kw)
    got, pre = _run(P, doc, root)
    want = R.prestate_ref(oracle, doc, root)
    _same(got, want)
    st = set(got["account_status"].tolist())
    assert R.PRESENT in st and R.ABSENT in st and pre.ok


def test_config4_scale_witness(P, oracle):
    """More than 300 000 nodes (BASELINE config 4's order): the class-list hash kernels, not the wave-per-node one."""
    rng = np.random.default_rng(4)
    n = suite.scale(150_000, 3_000)
    accounts = [{"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1 << 20)),
                 "balance": int(rng.integers(0, 1 << 62)), "code": b"", "storage": {}} for _ in range(n)]
    for c in range(suite.scale(12, 2)):
        accounts[c]["code"] = bytes([c + 1]) * (100 + 37 * c)
        accounts[c]["storage"] = {int(rng.integers(0, 1 << 62)): int(rng.integers(1, 1 << 62)) for _ in range(suite.scale(12_000, 300))}
    doc, root = R.full_witness(oracle, accounts, rng)
    if not suite.EMULATED:
        assert len(doc["state"]) > 300_000
    got, pre = _run(P, doc, root)
    want = R.prestate_ref(oracle, doc, root)
    _same(got, want)
    assert pre.ok and len(pre.accounts) == n


def _custom_state(oracle, leaves, storage_leaves=None):
    """a state trie whose leaves are the given bodies (address -> bytes) -> (doc pieces: nodes, root)"""
    kv = sorted((oracle.keccak256(a), v) for a, v in leaves.items())
    t = oracle.Trie([k for k, _ in kv], [v for _, v in kv])
    nodes = {}
    for k, _ in kv:
        for nd in t.prove(k):
            nodes[nd] = None
    return t, nodes


def test_damaged_nodes_and_a_wrong_root(P, oracle):
    rng = np.random.default_rng(21)
    doc, root, _ = R.block_witness_doc(oracle, rng, n_accounts=suite.scale(400, 60), n_contracts=5, max_slots=10,
                                       n_touched=suite.scale(60, 12), slots_per=4, n_absent=3)
    # a wrong trusted root: every account fails, every slot is not anchored
    bad_root = bytes(31) + b"\x01"
    got, _ = _run(P, doc, bad_root)
    _same(got, R.prestate_ref(oracle, doc, bad_root))
    assert (got["account_status"] == 20).all()  # PHANT_PROOF_MISSING_NODE: nothing in the set hashes to that root
    assert (got["slot_status"] == R.MISMATCH).all()
    # a damaged / a missing node on account paths
    for kind in ("flip", "drop"):
        d = dict(doc)
        st = list(doc["state"])
        for j in range(0, len(st), max(1, len(st) // 7)):
            if kind == "drop":
                st[j] = None
            else:
                b = bytearray(R._unhex(st[j]))
                b[len(b) // 2] ^= 0x10
                st[j] = R._hex(bytes(b))
        d["state"] = [x for x in st if x is not None]
        got, _ = _run(P, d, root)
        want = R.prestate_ref(oracle, d, root)
        _same(got, want)
        assert want["n_failed"] > 0
        bad_acc = np.nonzero(~np.isin(want["account_status"], [R.PRESENT, R.ABSENT]))[0]
        addrs, slots = R.keys_of(d)
        first = np.cumsum([0] + [len(s) for s in slots])
        for a in bad_acc:
            assert (got["slot_status"][first[a]:first[a + 1]] == R.MISMATCH).all()


def test_leaves_that_are_not_values(P, oracle):
    """Leaf bodies that are no account (a 9-byte nonce, a leading zero, a 33-byte balance, a 31-byte hash, a 3-item list) and slot
    values that are no minimal non-zero integer (0x00, a leading zero, 33 bytes): BAD_VALUE; a slot under a BAD_VALUE account:
    MISMATCH."""
    rng = np.random.default_rng(3)
    h32 = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    empty = R.EMPTY_ROOT
    skv = {1: b"\x00", 2: b"\x82\x00\x05", 3: b"\xa1" + b"\x07" * 33, 4: b"\x05", 5: b"\x81\x90", 6: b"\x80"}
    skeys = sorted((oracle.keccak256(s.to_bytes(32, "big")), v) for s, v in skv.items())
    stor = oracle.Trie([k for k, _ in skeys], [v for _, v in skeys])
    bodies = {
        "nonce9": _rlp_list([_rlp_str(b"\x01" * 9), _rlp_int(1), _rlp_str(empty), _rlp_str(R.EMPTY_CODE)]),
        "lead0": _rlp_list([_rlp_int(1), _rlp_str(b"\x00\x05"), _rlp_str(empty), _rlp_str(R.EMPTY_CODE)]),
        "bal33": _rlp_list([_rlp_int(1), _rlp_str(b"\x01" * 33), _rlp_str(empty), _rlp_str(R.EMPTY_CODE)]),
        "hash31": _rlp_list([_rlp_int(1), _rlp_int(2), _rlp_str(h32[:31]), _rlp_str(R.EMPTY_CODE)]),
        "three": _rlp_list([_rlp_int(1), _rlp_int(2), _rlp_str(empty)]),
        "trailing": _rlp_list([_rlp_int(1), _rlp_int(2), _rlp_str(empty), _rlp_str(R.EMPTY_CODE)]) + b"\x00",
        "good": _rlp_list([_rlp_int(7), _rlp_int(9), _rlp_str(stor.root()), _rlp_str(R.EMPTY_CODE)]),
        "oddcode": _rlp_list([_rlp_int(7), _rlp_int(9), _rlp_str(stor.root()), _rlp_str(R.EMPTY_CODE)[:-1] + b"\x00"]),
    }
    addrs = {name: bytes([i + 1]) * 20 for i, name in enumerate(bodies)}
    t, nodes = _custom_state(oracle, {addrs[n]: b for n, b in bodies.items()})
    for k, _ in skeys:
        for nd in stor.prove(k):
            nodes[nd] = None
    keys = [R._hex(addrs[n]) for n in bodies]
    keys += [R._hex(addrs["good"] + s.to_bytes(32, "big")) for s in skv]
    keys += [R._hex(addrs["nonce9"] + (4).to_bytes(32, "big"))]
    doc = {"state": [R._hex(x) for x in nodes], "keys": keys}
    got, pre = _run(P, doc, t.root())
    want = R.prestate_ref(oracle, doc, t.root())
    _same(got, want)
    st = dict(zip(bodies, got["account_status"].tolist()))
    for n in ("nonce9", "lead0", "bal33", "hash31", "three", "trailing"):
        assert st[n] == R.BAD_VALUE, (n, st[n])
    assert st["good"] == R.PRESENT and st["oddcode"] == R.PRESENT
    ss = got["slot_status"].tolist()  # (grouped by account: the slot under "nonce9" first, then those of "good")
    assert ss[0] == R.MISMATCH
    assert ss[1:] == [R.BAD_VALUE, R.BAD_VALUE, R.BAD_VALUE, R.PRESENT, R.PRESENT, R.BAD_VALUE], ss
    assert int.from_bytes(got["slot_vals"][4].tobytes(), "big") == 5 and int.from_bytes(got["slot_vals"][5].tobytes(), "big") == 0x90
    assert not pre.ok and got["n_failed"] == 6 + 4 + 1 and got["n_missing_code"] == 1


def test_codes(P, oracle):
    """A missing code (CODE_NONE, counted, the account stays PRESENT), an empty code, duplicate codes (the lowest index), unused
    codes, one code of 24 576 bytes and one of 0 bytes."""
    rng = np.random.default_rng(8)
    big = rng.integers(0, 256, 24_576, dtype=np.uint8).tobytes()
    c1 = rng.integers(0, 256, 136, dtype=np.uint8).tobytes()   # exactly one rate block
    c2 = rng.integers(0, 256, 135, dtype=np.uint8).tobytes()
    c3 = rng.integers(0, 256, 777, dtype=np.uint8).tobytes()   # missing from the witness
    accounts = [{"addr": bytes([i + 1]) * 20, "nonce": i, "balance": 10 * i, "code": c, "storage": {}}
                for i, c in enumerate([big, c1, c2, c3, b"", c1])]
    doc, root = R.full_witness(oracle, accounts, rng)
    unused = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    doc["codes"] = [R._hex(x) for x in [unused, c1, big, c2, b"", c1, big]]
    got, pre = _run(P, doc, root)
    want = R.prestate_ref(oracle, doc, root)
    _same(got, want)
    assert got["code_index"].tolist() == [2, 1, 3, R.CODE_NONE, R.CODE_NONE, 1]
    assert got["n_missing_code"] == 1 and got["n_unused_codes"] == 2  # `unused` and the empty code
    assert (got["account_status"] == R.PRESENT).all() and pre.ok
    assert pre.missing_code == [accounts[3]["addr"]]
    assert pre.accounts[0].code == big and pre.accounts[4].code == b""
    # no codes member at all
    del doc["codes"]
    got, _ = _run(P, doc, root)
    want = R.prestate_ref(oracle, doc, root)
    _same(got, want)
    assert got["n_missing_code"] == 5 and got["n_unused_codes"] == 0


def test_code_hash_forms_agree(P, oracle):
    """The lane-per-code form (PHANT_DIAG_CODE_HASH_FORM = 1) gives what the half-wave form gives."""
    from phant_amd.context import default_context
    rng = np.random.default_rng(9)
    doc, root, _ = R.block_witness_doc(oracle, rng, n_accounts=60, n_contracts=suite.scale(20, 5), max_slots=4, n_touched=30,
                                       slots_per=2, n_absent=2)
    want = R.prestate_ref(oracle, doc, root)
    ctx = default_context()
    try:
        ctx.diag_set("code_hash_form", 1)
        got, _ = _run(P, doc, root)
    finally:
        ctx.diag_set("code_hash_form", 0)
    _same(got, want)


def test_new_payload_prestate_hook(P, oracle):
    rng = np.random.default_rng(10)
    doc, root, _ = R.block_witness_doc(oracle, rng, n_accounts=50, n_contracts=4, max_slots=5, n_touched=10, slots_per=2, n_absent=2)
    pre = P.stateless.new_payload_prestate(R.dumps(doc), root)
    assert pre.ok and pre.absent
    with pytest.raises(P.stateless.PrestateError):
        P.stateless.new_payload_prestate(R.dumps(doc), bytes(32))
    with pytest.raises(ValueError):
        P.stateless.StatelessWitness.parse_json(R.dumps(doc)).prestate(None, None)
