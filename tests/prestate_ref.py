"""TEST INFRASTRUCTURE: the CPU reference of phant_exec_witness_prestate, built from what oracle/oracle.py offers -- the node-set
walk twice (the accounts from the trusted root; the slots from the storage roots the account leaves prove, decoded here in Python
between the two walks) and oracle.keccak256 for the codes -- plus the builders of execution-witness documents the tests use."""
import json

import numpy as np

from tests.witness_util import _rlp_int, _rlp_list, _rlp_str

PRESENT, ABSENT, MISMATCH, BAD_VALUE = 1, 2, 22, 23
CODE_NONE = 0xFFFFFFFF
EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")
EMPTY_CODE = bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")


def _hex(b: bytes) -> str:
    return "0x" + b.hex()


def _unhex(s: str) -> bytes:
    s = s[2:] if s[:2] in ("0x", "0X") else s
    return b"" if s in ("", "0") else bytes.fromhex(s)


def keys_of(doc):
    """-> (addresses in order of first appearance, slot preimages per account in order of first appearance)"""
    addrs, index, slots, seen = [], {}, [], set()
    for k in doc["keys"]:
        b = _unhex(k)
        a = b[:20]
        if a not in index:
            index[a] = len(addrs)
            addrs.append(a)
            slots.append([])
        if len(b) == 52 and b not in seen:
            seen.add(b)
            slots[index[a]].append(b[20:])
    return addrs, slots


def _short_string(v: bytes, p: int):
    """-> (content, p behind it) of one canonical short RLP string at v[p:], or None"""
    if p >= len(v):
        return None
    b = v[p]
    if b < 0x80:
        return v[p:p + 1], p + 1
    if b > 0xB7:
        return None
    n = b - 0x80
    if n > len(v) - p - 1 or (n == 1 and v[p + 1] < 0x80):
        return None
    return v[p + 1:p + 1 + n], p + 1 + n


def decode_account(v: bytes):
    """strict rlp([nonce, balance, storageRoot, codeHash]) -> (nonce, balance, storage_root, code_hash) or None"""
    if not v:
        return None
    if 0xC0 <= v[0] <= 0xF7:
        pay, p = v[0] - 0xC0, 1
    elif v[0] == 0xF8 and len(v) >= 2 and v[1] >= 56:
        pay, p = v[1], 2
    else:
        return None
    if p + pay != len(v):
        return None
    items = []
    for _ in range(4):
        r = _short_string(v, p)
        if r is None:
            return None
        c, p = r
        items.append(c)
    if p != len(v):
        return None
    n, b, sr, ch = items
    if len(n) > 8 or (n and n[0] == 0) or len(b) > 32 or (b and b[0] == 0) or len(sr) != 32 or len(ch) != 32:
        return None
    return int.from_bytes(n, "big"), int.from_bytes(b, "big"), sr, ch


def decode_slot(v: bytes):
    r = _short_string(v, 0)
    if r is None or r[1] != len(v) or not 1 <= len(r[0]) <= 32 or r[0][0] == 0:
        return None
    return int.from_bytes(r[0], "big")


def prestate_ref(oracle, doc, state_root: bytes) -> dict:
    """The outputs of phant_exec_witness_prestate for the document `doc` (a dict) against `state_root`."""
    nodes = [_unhex(x) for x in doc["state"]]
    codes = [_unhex(x) for x in doc.get("codes", [])]
    addrs, slots = keys_of(doc)
    na = len(addrs)
    blob = np.frombuffer(b"".join(nodes), np.uint8).copy() if nodes else np.zeros(0, np.uint8)
    off = np.zeros(len(nodes) + 1, np.uint64)
    if nodes:
        off[1:] = np.cumsum([len(x) for x in nodes])
    out = {"account_status": np.zeros(na, np.uint8), "nonces": np.zeros(na, np.uint64), "balances": np.zeros((na, 32), np.uint8),
           "storage_roots": np.zeros((na, 32), np.uint8), "code_hashes": np.zeros((na, 32), np.uint8),
           "code_index": np.full(na, CODE_NONE, np.uint32)}
    failed = 0
    if na:
        keys = np.frombuffer(b"".join(oracle.keccak256(a) for a in addrs), np.uint8).copy()
        st, voff, vlen = oracle.mpt_verify_nodeset(np.frombuffer(state_root, np.uint8), None, keys, 32, blob, off)
        for i in range(na):
            s, acc = int(st[i]), None
            if s == PRESENT:
                acc = decode_account(blob[int(voff[i]):int(voff[i]) + int(vlen[i])].tobytes())
                if acc is None:
                    s = BAD_VALUE
            nonce, bal, sr, ch = acc if acc else (0, 0, EMPTY_ROOT, EMPTY_CODE)
            out["account_status"][i] = s
            out["nonces"][i] = nonce
            out["balances"][i] = np.frombuffer(bal.to_bytes(32, "big"), np.uint8)
            out["storage_roots"][i] = np.frombuffer(sr, np.uint8)
            out["code_hashes"][i] = np.frombuffer(ch, np.uint8)
            failed += s not in (PRESENT, ABSENT)
    # the slots, walked from the storage roots the first walk proved
    flat = [(a, sl) for a in range(na) for sl in slots[a]]
    ns = len(flat)
    out["slot_status"] = np.zeros(ns, np.uint8)
    out["slot_vals"] = np.zeros((ns, 32), np.uint8)
    if ns:
        ridx = np.array([a for a, _ in flat], np.uint32)
        keys = np.frombuffer(b"".join(oracle.keccak256(sl) for _, sl in flat), np.uint8).copy()
        st, voff, vlen = oracle.mpt_verify_nodeset(out["storage_roots"].reshape(-1), ridx, keys, 32, blob, off)
        for j, (a, _) in enumerate(flat):
            s, v = int(st[j]), 0
            if out["account_status"][a] not in (PRESENT, ABSENT):
                s = MISMATCH
            elif s == PRESENT:
                v = decode_slot(blob[int(voff[j]):int(voff[j]) + int(vlen[j])].tobytes())
                if v is None:
                    s, v = BAD_VALUE, 0
            out["slot_status"][j] = s
            out["slot_vals"][j] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)
            failed += s not in (PRESENT, ABSENT)
    # codes: the lowest index per digest
    first = {}
    for k, c in enumerate(codes):
        first.setdefault(oracle.keccak256(c), k)
    used, missing = set(), 0
    for i in range(na):
        ch = out["code_hashes"][i].tobytes()
        if out["account_status"][i] != PRESENT or ch == EMPTY_CODE:
            continue
        if ch in first:
            out["code_index"][i] = first[ch]
            used.add(ch)
        else:
            missing += 1
    out["n_failed"] = failed
    out["n_missing_code"] = missing
    out["n_unused_codes"] = sum(1 for c in codes if oracle.keccak256(c) not in used)
    return out


# ---------------------------------------------------------------- documents
def account_leaf(oracle, a, storage_root: bytes) -> bytes:
    return _rlp_list([_rlp_int(int(a["nonce"])), _rlp_int(int(a["balance"])), _rlp_str(storage_root),
                      _rlp_str(oracle.keccak256(bytes(a["code"])))])


def build_tries(oracle, accounts):
    """accounts: dicts addr / nonce / balance / code / storage (zero values allowed: not in the trie) ->
    (state trie, its sorted keys, {account index: (storage trie, sorted keys)})"""
    storage = {}
    for i, a in enumerate(accounts):
        kv = sorted((oracle.keccak256(int(s).to_bytes(32, "big")), _rlp_int(int(v))) for s, v in a["storage"].items() if int(v))
        if kv:
            storage[i] = (oracle.Trie([k for k, _ in kv], [v for _, v in kv]), [k for k, _ in kv])
    kv = sorted((oracle.keccak256(a["addr"]), account_leaf(oracle, a, storage[i][0].root() if i in storage else EMPTY_ROOT))
                for i, a in enumerate(accounts))
    state = oracle.Trie([k for k, _ in kv], [v for _, v in kv])
    return state, [k for k, _ in kv], storage


def full_witness(oracle, accounts, rng, extra_keys=()):
    """The execution witness of the whole alloc: every node of the state trie and of every storage trie (the union of the proofs
    of all their keys), shuffled; all codes; every address and every address ++ slot.  -> (doc, state root)"""
    state, skeys, storage = build_tries(oracle, accounts)
    nodes = {}
    for k in skeys:
        for nd in state.prove(k):
            nodes[nd] = None
    for t, ks in storage.values():
        for k in ks:
            for nd in t.prove(k):
                nodes[nd] = None
    uniq = list(nodes)
    uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    codes = list(dict.fromkeys(bytes(a["code"]) for a in accounts if a["code"]))
    keys = []
    for a in accounts:
        keys.append(_hex(a["addr"]))
        keys += [_hex(a["addr"] + int(s).to_bytes(32, "big")) for s in a["storage"]]
    keys += list(extra_keys)
    return {"state": [_hex(x) for x in uniq], "codes": [_hex(c) for c in codes], "keys": keys}, state.root()


def block_witness_doc(oracle, rng, n_accounts=1500, n_contracts=40, max_slots=60, n_touched=300, slots_per=8, n_absent=30):
    """A block-shaped execution witness (witness_util.block_witness's shapes): a state of n_accounts, the first n_contracts with
    storage and code; the proofs of n_touched accounts (a few absent) and of slots under them (a few absent, some under absent
    accounts), every node once, shuffled.  -> (doc, state root, accounts)"""
    accounts = []
    for i in range(n_accounts):
        st = {}
        code = b""
        if i < n_contracts:
            for _ in range(int(rng.integers(1, max_slots + 1))):
                st[int(rng.integers(0, 1 << 62))] = int.from_bytes(rng.integers(0, 256, int(rng.integers(1, 33)), dtype=np.uint8).tobytes(), "big") or 1
            code = rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes()
        accounts.append({"addr": rng.integers(0, 256, 20, dtype=np.uint8).tobytes(), "nonce": int(rng.integers(0, 1000)),
                         "balance": int(rng.integers(0, 1 << 62)), "code": code, "storage": st})
    state, _, storage = build_tries(oracle, accounts)
    touched = sorted(set(int(x) for x in rng.integers(0, n_contracts, min(n_contracts, n_touched)))
                     | set(int(x) for x in rng.integers(0, n_accounts, n_touched)))
    absent = [rng.integers(0, 256, 20, dtype=np.uint8).tobytes() for _ in range(n_absent)]
    nodes, keys = {}, []
    for i in touched:
        a = accounts[i]
        keys.append(_hex(a["addr"]))
        for nd in state.prove(oracle.keccak256(a["addr"])):
            nodes[nd] = None
        if i in storage:
            t = storage[i][0]
            have = list(a["storage"])
            for _ in range(slots_per):
                s = have[int(rng.integers(0, len(have)))] if rng.random() < 0.8 else int(rng.integers(0, 1 << 62))
                keys.append(_hex(a["addr"] + s.to_bytes(32, "big")))
                for nd in t.prove(oracle.keccak256(s.to_bytes(32, "big"))):
                    nodes[nd] = None
    for j, ad in enumerate(absent):
        keys.append(_hex(ad))
        if j % 3 == 0:  # a slot under an absent account
            keys.append(_hex(ad + int(rng.integers(0, 1 << 62)).to_bytes(32, "big")))
        for nd in state.prove(oracle.keccak256(ad)):
            nodes[nd] = None
    order = rng.permutation(len(keys))
    keys = [keys[i] for i in order]
    uniq = list(nodes)
    uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    codes = [a["code"] for a in accounts[:n_contracts]]
    return {"state": [_hex(x) for x in uniq], "codes": [_hex(c) for c in codes], "keys": keys}, state.root(), accounts


def dumps(doc) -> str:
    return json.dumps(doc)
