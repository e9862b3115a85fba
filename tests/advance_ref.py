"""TEST INFRASTRUCTURE: the CPU reference of phant_exec_witness_advance's node set.  As in tests/poststate_ref.py the truth is the FULL
state: the writes are applied to the complete account list (poststate_ref.apply_writes), every trie in scope is built whole with
oracle.Trie, and the expected "state" of the next witness is, per trie,

    A = the union of Trie.prove(k) over the witness's keys of that trie          (the post-trie walks, rule 3 of the prover)
    B = all nodes of the post trie - all nodes of the pre trie, by bytes          (what the writes created, on those walks or beside)

sorted, and concatenated over the tries: the post storage tries of the accounts that exist afterwards and have a slot among the keys
(an empty one has no nodes), then the state trie."""
import numpy as np

from tests import poststate_ref as Q
from tests import prestate_ref as R


def _all_nodes(trie, keys):
    out = set()
    for k in keys:
        out.update(trie.prove(k))
    return out


def assert_positions_distinct(trie, keys):
    """no two positions of the trie hold the same bytes (the reference compares by bytes): a node reached behind two different
    chains of ancestors, or one branch that refers to the same hash twice"""
    seen = {}
    for k in keys:
        proof = trie.prove(k)
        for i, nd in enumerate(proof):
            above = tuple(proof[:i])
            assert seen.setdefault(nd, above) == above, "identical nodes at two positions: choose other inputs"
            items = R.rlp_decode_strict(nd)
            if isinstance(items, list) and len(items) == 17:
                refs = [bytes(x) for x in items[:16] if isinstance(x, (bytes, bytearray)) and len(x) == 32]
                assert len(refs) == len(set(refs)), "a branch with one child twice: choose other inputs"


def trie_nodes(post, post_keys, pre, pre_keys, witness_keys, check_distinct=False):
    """-> (sorted A | B, B - A) for one trie; post / pre: oracle.Trie or None (empty)"""
    if post is None:
        return [], set()
    if check_distinct:
        assert_positions_distinct(post, post_keys)
    a = set()
    for k in witness_keys:
        a.update(post.prove(k))
    b = _all_nodes(post, post_keys) - (_all_nodes(pre, pre_keys) if pre is not None else set())
    return sorted(a | b), b - a


def expected(oracle, info, accounts, writes):
    """-> dict(nodes: the expected sorted-per-trie concatenation, beside: how many nodes of B are on no key's walk, emptied: storage
    tries among the keys' accounts that are empty afterwards, created_with_slots: accounts the block creates with a live slot among
    the keys, after: the complete post-state)"""
    after = Q.apply_writes(accounts, writes)
    pre_state, pre_skeys, pre_storage = R.build_tries(oracle, accounts)
    post_state, post_skeys, post_storage = R.build_tries(oracle, after) if after else (None, [], {})
    pre_idx = {a["addr"]: i for i, a in enumerate(accounts)}
    post_idx = {a["addr"]: i for i, a in enumerate(after)}
    first, slots = info["slot_first"], info["slots"]
    nodes, beside, emptied, created = [], 0, 0, 0
    addrs = [bytes(a) for a in info["addresses"]]
    for k, addr in enumerate(addrs):
        js = range(int(first[k]), int(first[k + 1]))
        if not len(js) or addr not in post_idx:
            continue
        pre = pre_storage.get(pre_idx.get(addr, -1))
        post = post_storage.get(post_idx[addr])
        if post is None:
            emptied += pre is not None
            continue
        created += addr not in pre_idx
        wk = [oracle.keccak256(slots[j].tobytes()) for j in js]
        got, extra = trie_nodes(post[0], post[1], pre[0] if pre else None, pre[1] if pre else [], wk)
        nodes += got
        beside += len(extra)
    got, extra = trie_nodes(post_state, post_skeys, pre_state if accounts else None, pre_skeys, [oracle.keccak256(a) for a in addrs])
    nodes += got
    beside += len(extra)
    return {"nodes": nodes, "beside": beside, "emptied": emptied, "created_with_slots": created, "after": after}


def nodes_of(info):
    """the "state" of a witness as a list of byte strings, in its own order"""
    blob, off = info["nodes"].tobytes(), info["node_off"]
    return [blob[int(off[j]):int(off[j + 1])] for j in range(info["total_nodes"])]


def check_prestate(oracle, pre, info, after):
    """`pre`: prestate_arrays of the next witness against the post root -- every account and slot must be the post alloc's, a
    deleted (or never created) account ABSENT"""
    assert pre["n_failed"] == 0, (pre["n_failed"], pre["account_status"][:8], pre["slot_status"][:8])
    post = {a["addr"]: a for a in after}
    first, slots = info["slot_first"], info["slots"]
    for k, addr in enumerate(bytes(a) for a in info["addresses"]):
        a = post.get(addr)
        assert pre["account_status"][k] == (Q.PRESENT if a else Q.ABSENT), (k, pre["account_status"][k])
        if a:
            assert int(pre["nonces"][k]) == int(a["nonce"])
            assert int.from_bytes(pre["balances"][k].tobytes(), "big") == int(a["balance"])
            assert pre["code_hashes"][k].tobytes() == oracle.keccak256(bytes(a["code"]))
        for j in range(int(first[k]), int(first[k + 1])):
            v = int(a["storage"].get(int.from_bytes(slots[j].tobytes(), "big"), 0)) if a else 0
            assert pre["slot_status"][j] == (Q.PRESENT if v else Q.ABSENT), (k, j, pre["slot_status"][j])
            assert int.from_bytes(pre["slot_vals"][j].tobytes(), "big") == v


def arrays_equal(a: dict, b: dict):
    for key in ("state_root", "n_failed"):
        assert a[key] == b[key], key
    for key in ("storage_roots", "account_status", "slot_status"):
        assert np.array_equal(a[key], b[key]), key
