"""TEST INFRASTRUCTURE: the CPU reference of phant_exec_witness_poststate.  The truth is the FULL state, never a partial-trie
algorithm: the writes are applied to the complete account list, oracle.state_root gives the root and oracle.mptize (through
prestate_ref.build_tries) every storage root.  Plus the builder of the witness a producer would ship: the proofs of every touched
key and, for every removed key, the proofs of the nearest surviving pre-state key on each side in hashed-key order (a branch's
keys are contiguous in that order, so the surviving child of any collapse is among them)."""
import numpy as np

from tests import prestate_ref as R

PRESENT, ABSENT, MISMATCH, MISSING_NODE, MISSING_SIBLING = 1, 2, 22, 20, 24
KEEP, SET, DELETE = 0, 1, 2
EMPTY_ROOT = R.EMPTY_ROOT


def apply_writes(accounts, writes):
    """accounts: the complete pre-state (dicts addr / nonce / balance / code / storage).  writes: addr -> None (delete) |
    dict(nonce, balance, code, storage={slot: value}) (SET: the storage entries are slot WRITES, zero removes) |
    ("keep", {slot: value}).  -> the complete post-state"""
    by = {a["addr"]: a for a in accounts}
    out = []
    for a in accounts:
        w = writes.get(a["addr"], "untouched")
        if w is None:
            continue
        st = dict(a["storage"])
        b = dict(a)
        if w != "untouched":
            upd = w[1] if isinstance(w, tuple) else w["storage"]
            st.update(upd)
            if not isinstance(w, tuple):
                b.update(nonce=w["nonce"], balance=w["balance"], code=w["code"])
        b["storage"] = {s: v for s, v in st.items() if v}
        out.append(b)
    for addr, w in writes.items():
        if addr not in by and isinstance(w, dict):
            out.append({"addr": addr, "nonce": w["nonce"], "balance": w["balance"], "code": w["code"],
                        "storage": {s: v for s, v in w["storage"].items() if v}})
    return out


def _neighbours(sorted_keys, removed):
    """for every removed key the nearest key on each side that is not removed"""
    out = set()
    pos = {k: i for i, k in enumerate(sorted_keys)}
    for k in removed:
        for step in (-1, 1):
            i = pos[k] + step
            while 0 <= i < len(sorted_keys) and sorted_keys[i] in removed:
                i += step
            if 0 <= i < len(sorted_keys):
                out.add(sorted_keys[i])
    return out


def witness_doc(oracle, accounts, writes, rng, extra_slots=None, neighbours=True, tries=None):
    """-> (doc, parent root).  Keys: every written address and slot (+ extra_slots: addr -> [slot] read only), shuffled."""
    state, skeys, storage = tries or R.build_tries(oracle, accounts)
    index = {a["addr"]: i for i, a in enumerate(accounts)}
    nodes, keys = {}, []

    def add(trie, k):
        for nd in trie.prove(k):
            nodes[nd] = None

    removed_acc = set()
    for addr, w in writes.items():
        keys.append(R._hex(addr))
        hk = oracle.keccak256(addr)
        add(state, hk)
        if w is None and addr in index:
            removed_acc.add(hk)
        upd = {} if w is None else (w[1] if isinstance(w, tuple) else w["storage"])
        slots = list(upd) + list((extra_slots or {}).get(addr, []))
        i = index.get(addr)
        removed = set()
        for s in slots:
            keys.append(R._hex(addr + int(s).to_bytes(32, "big")))
            if i is not None and i in storage:
                sk = oracle.keccak256(int(s).to_bytes(32, "big"))
                add(storage[i][0], sk)
                if s in upd and not int(upd[s]) and int(accounts[i]["storage"].get(s, 0)):
                    removed.add(sk)
        if neighbours and removed:
            for k in _neighbours(storage[i][1], removed):
                add(storage[i][0], k)
    if neighbours:
        for k in _neighbours(skeys, removed_acc):
            add(state, k)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    uniq = list(nodes)
    uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    return {"state": [R._hex(x) for x in uniq], "keys": keys}, state.root()


def write_arrays(oracle, info, writes):
    """the C-ABI's input arrays in the witness's own order"""
    na, ns = info["n_accounts"], info["n_slots"]
    w = {"account_op": np.zeros(na, np.uint8), "nonces": np.zeros(na, np.uint64), "balances": np.zeros((na, 32), np.uint8),
         "code_hashes": np.zeros((na, 32), np.uint8), "slot_write": np.zeros(ns, np.uint8), "slot_vals": np.zeros((ns, 32), np.uint8)}
    first, slots = info["slot_first"], info["slots"]
    for k, addr in enumerate(bytes(a) for a in info["addresses"]):
        x = writes.get(addr, "untouched")
        if x == "untouched":
            continue
        if x is None:
            w["account_op"][k] = DELETE
            continue
        upd = x[1] if isinstance(x, tuple) else x["storage"]
        if not isinstance(x, tuple):
            w["account_op"][k] = SET
            w["nonces"][k] = x["nonce"]
            w["balances"][k] = np.frombuffer(int(x["balance"]).to_bytes(32, "big"), np.uint8)
            w["code_hashes"][k] = np.frombuffer(oracle.keccak256(bytes(x["code"])), np.uint8)
        for j in range(int(first[k]), int(first[k + 1])):
            s = int.from_bytes(slots[j].tobytes(), "big")
            if s in upd:
                w["slot_write"][j] = 1
                w["slot_vals"][j] = np.frombuffer(int(upd[s]).to_bytes(32, "big"), np.uint8)
    return w


def expected(oracle, info, accounts, writes):
    """-> dict(state_root, storage_roots, account_status, slot_status) from the full pre- and post-state"""
    after = apply_writes(accounts, writes)
    pre = {a["addr"]: a for a in accounts}
    post = {a["addr"]: a for a in after}
    _, _, storage = R.build_tries(oracle, after)
    sroot = {a["addr"]: (storage[i][0].root() if i in storage else EMPTY_ROOT) for i, a in enumerate(after)}
    na, ns = info["n_accounts"], info["n_slots"]
    out = {"state_root": oracle.state_root(after) if after else EMPTY_ROOT, "storage_roots": np.zeros((na, 32), np.uint8),
           "account_status": np.zeros(na, np.uint8), "slot_status": np.zeros(ns, np.uint8)}
    first, slots = info["slot_first"], info["slots"]
    for k, addr in enumerate(bytes(a) for a in info["addresses"]):
        out["account_status"][k] = PRESENT if addr in pre else ABSENT
        out["storage_roots"][k] = np.frombuffer(sroot.get(addr, EMPTY_ROOT), np.uint8)
        for j in range(int(first[k]), int(first[k + 1])):
            s = int.from_bytes(slots[j].tobytes(), "big")
            out["slot_status"][j] = PRESENT if addr in pre and int(pre[addr]["storage"].get(s, 0)) else ABSENT
    return out
