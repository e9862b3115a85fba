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


# ---------------------------------------------------------------- a second, independent strict reference
# Written from the RLP specification (Ethereum yellow paper, appendix B), not from the kernel: a general decoder of ONE canonical
# item into a tree (bytes | list), and the type rules of an account body / a slot value applied on that tree.  decode_account /
# decode_slot above follow account_decode_kernel's order of checks; a misreading of RLP shared by the kernel and its mirror shows
# up as a disagreement between the two references (tests/test_prestate_ref.py).
def _rlp_length(b: bytes, p: int, end: int, ll: int):
    """the big-endian length of a long form, `ll` bytes at b[p:]: minimal (no leading zero byte, >= 56) or None"""
    if p + ll > end or b[p] == 0:
        return None
    n = int.from_bytes(b[p:p + ll], "big")
    return n if n >= 56 else None


def _rlp_item(b: bytes, p: int, end: int):
    """-> (item, index behind it) of the canonical item that starts at b[p] and lies inside b[p:end], or None"""
    if p >= end:
        return None
    t = b[p]
    if t < 0x80:                                    # a single byte is its own encoding
        return b[p:p + 1], p + 1
    if t <= 0xB7 or 0xC0 <= t <= 0xF7:              # short string / short list: the length is in the prefix
        n, body = t - (0x80 if t <= 0xB7 else 0xC0), p + 1
    else:                                           # long string / long list: a length of 1 .. 8 bytes follows the prefix
        ll = t - (0xB7 if t <= 0xBF else 0xF7)
        n, body = _rlp_length(b, p + 1, end, ll), p + 1 + ll
        if n is None:
            return None
    if body + n > end:
        return None
    if t <= 0xBF:
        if t == 0x81 and b[body] < 0x80:            # must have been the single byte itself
            return None
        return b[body:body + n], body + n
    items, q = [], body
    while q < body + n:
        r = _rlp_item(b, q, body + n)
        if r is None:
            return None
        items.append(r[0])
        q = r[1]
    return items, body + n


def rlp_decode_strict(b: bytes):
    """The item `b` is the canonical RLP encoding of (bytes, or a list of items), or None: non-minimal length forms, length bytes
    with a leading zero, 0x81 in front of a byte below 0x80, an item that overruns its container and trailing bytes are rejected."""
    b = bytes(b)
    r = _rlp_item(b, 0, len(b))
    return r[0] if r is not None and r[1] == len(b) else None


def _scalar(x, max_len: int):
    return isinstance(x, bytes) and len(x) <= max_len and not (x and x[0] == 0)


def account_of_item(item):
    """a decoded tree -> (nonce, balance, storage_root, code_hash), or None where it is no account body"""
    if not isinstance(item, list) or len(item) != 4:
        return None
    n, b, sr, ch = item
    if not (_scalar(n, 8) and _scalar(b, 32) and isinstance(sr, bytes) and len(sr) == 32 and isinstance(ch, bytes) and len(ch) == 32):
        return None
    return int.from_bytes(n, "big"), int.from_bytes(b, "big"), sr, ch


def slot_of_item(item):
    """a decoded tree -> the slot's value, or None where it is no minimal non-zero integer of 1 to 32 bytes"""
    if not (isinstance(item, bytes) and _scalar(item, 32) and len(item) >= 1):
        return None
    return int.from_bytes(item, "big")


def strict_account(v: bytes):
    return account_of_item(rlp_decode_strict(v))


def strict_slot(v: bytes):
    return slot_of_item(rlp_decode_strict(v))


# ---------------------------------------------------------------- decode corpora
NONCE_EDGES = (0, 1, 0x7F, 0x80, 0xFF, 1 << 56, 1 << 63, (1 << 64) - 1)
BALANCE_EDGES = (0, 1, 0x7F, 0x80, 1 << 64, 1 << 248, 1 << 255, (1 << 256) - 1)
MUTATION_BYTES = (0x00, 0x7F, 0x80, 0x81, 0xB7, 0xB8, 0xC0, 0xF7, 0xF8, 0xF9)
# What each family of leaf_corpus can come out as, argued from the format and not from any decoder's answer:
#   seed     canonical bodies: PRESENT.
#   byte     one byte replaced: a byte of a prefix or the first byte of a scalar mostly breaks the body, a byte INSIDE the nonce,
#            the balance or the code hash (the last two bytes always are) leaves a canonical body with another value: both.
#   trunc / append / prefix   the outer list no longer spans exactly the value: BAD_VALUE.
#   item     an item that is a list, a string in its long form, or 0x81 in front of a byte below 0x80: BAD_VALUE.
#   width    a canonical list whose nonce has 9 bytes, whose balance has 33 or one of whose hashes has not 32: BAD_VALUE.
#   count    three / five items: BAD_VALUE.     short   short lists (payload < 56: no room for two 32-byte hashes): BAD_VALUE.
#   other    a single byte, a 200-byte string, a 200-byte list: BAD_VALUE.
LEAF_FAMILIES = {"seed": {True}, "byte": {True, False}, "trunc": {False}, "append": {False}, "prefix": {False}, "item": {False},
                 "width": {False}, "count": {False}, "short": {False}, "other": {False}}


def _account_items(nonce, balance, sr, ch):
    return [_rlp_int(nonce), _rlp_int(balance), _rlp_str(sr), _rlp_str(ch)]


def leaf_corpus(rng, mutate_every=3):
    """(name, body) of account-leaf bodies, deterministic in `rng`: the 64 canonical seeds at the width edges of nonce and balance
    and, of every `mutate_every`-th seed, the mutations of LEAF_FAMILIES (name = family/...).  No duplicates, no empty body."""
    rnd32 = lambda: rng.integers(0, 256, 32, dtype=np.uint8).tobytes()  # noqa: E731
    roots = (None, EMPTY_ROOT, bytes(32), b"\xff" * 32)
    hashes = (None, EMPTY_CODE, bytes(32), b"\xff" * 32, EMPTY_CODE)  # (five against four: every pair comes up)
    out, seen = [], set()

    def add(name, body):
        body = bytes(body)
        if body and body not in seen:
            seen.add(body)
            out.append((name, body))

    seeds = []
    for i, n in enumerate(NONCE_EDGES):
        for j, b in enumerate(BALANCE_EDGES):
            k = 8 * i + j
            sr, ch = roots[k % 4] or rnd32(), hashes[k % 5] or rnd32()
            seeds.append((f"n{i}b{j}", _account_items(n, b, sr, ch)))
            add(f"seed/n{i}b{j}", _rlp_list(seeds[-1][1]))
    assert min(len(b) for _, b in out) == 70 and max(len(b) for _, b in out) == 110 and all(b[0] == 0xF8 for _, b in out)
    for tag, items in seeds[::mutate_every]:
        body = _rlp_list(items)
        pay = b"".join(items)
        for k in range(1, len(body)):
            add(f"trunc/{tag}/{k}", body[:k])
        for k in (1, 2, 3):
            add(f"append/{tag}/{k}", body + bytes(rng.integers(0, 256, k, dtype=np.uint8)))
        for pos in list(range(12)) + [len(body) - 2, len(body) - 1]:
            for v in MUTATION_BYTES:
                add(f"byte/{tag}/{pos}={v:02x}", body[:pos] + bytes([v]) + body[pos + 1:])
        add(f"prefix/{tag}/len-1", bytes([0xF8, len(pay) - 1]) + pay)
        add(f"prefix/{tag}/len+1", bytes([0xF8, len(pay) + 1]) + pay)
        add(f"prefix/{tag}/f7", bytes([0xF7]) + body[1:])
        add(f"prefix/{tag}/f9", bytes([0xF9]) + body[1:])
        add(f"prefix/{tag}/f8-55", bytes([0xF8, 55]) + pay)
        add(f"prefix/{tag}/f8-55-cut", bytes([0xF8, 55]) + pay[:55])
        add(f"prefix/{tag}/f8-4", bytes([0xF8, 4]) + pay[:4])
        add(f"prefix/{tag}/f9-00", bytes([0xF9, 0x00, len(pay)]) + pay)
        add(f"prefix/{tag}/short-form", bytes([0xC0 + min(len(pay), 55)]) + pay)
        for k in range(4):
            content = rlp_decode_strict(items[k])
            own = content[:1] if content and content[0] < 0x80 else b"\x05"
            for what, repl in (("list", _rlp_list([items[k]])), ("empty-list", b"\xc0"),
                               ("long-form-32", bytes([0xB8, 0x20]) + b"\x01" + (content + bytes(31))[:31]),
                               ("long-form-own", bytes([0xB8, len(content)]) + content), ("81-00", b"\x81\x00"),
                               ("81-7f", b"\x81\x7f"), ("81-own", b"\x81" + own)):
                add(f"item/{tag}/{k}/{what}", _rlp_list(items[:k] + [repl] + items[k + 1:]))
        for what, k, repl in (("nonce-9", 0, b"\x01" + bytes(8)), ("nonce-9-ff", 0, b"\xff" * 9), ("balance-33", 1, b"\x01" + bytes(32)),
                              ("balance-33-ff", 1, b"\xff" * 33), ("root-31", 2, b"\x77" * 31), ("root-33", 2, b"\x77" * 33),
                              ("root-0", 2, b""), ("hash-31", 3, b"\x77" * 31), ("hash-33", 3, b"\x77" * 33), ("hash-1", 3, b"\x77")):
            add(f"width/{tag}/{what}", _rlp_list(items[:k] + [_rlp_str(repl)] + items[k + 1:]))
        add(f"count/{tag}/3", _rlp_list(items[:3]))
        add(f"count/{tag}/3b", _rlp_list(items[1:]))
        add(f"count/{tag}/5", _rlp_list(items + [b"\x80"]))
        add(f"count/{tag}/5b", _rlp_list(items + [items[0]]))
    # the short-list branch of the decoder (0xc0 .. 0xf7): no valid body is that short
    add("short/c0", b"\xc0")
    add("short/c4", bytes.fromhex("c401020304"))
    add("short/c4-80", bytes.fromhex("c480808080"))
    add("short/four-short-items", _rlp_list([_rlp_int(5), _rlp_int(1 << 70), _rlp_str(b"\x11" * 20), _rlp_str(b"\x22" * 20)]))
    add("short/f7", _rlp_list([_rlp_int(1), _rlp_int(2), _rlp_str(b"\x33" * 32), _rlp_str(b"\x44" * 19)]))
    assert out[-1][1][0] == 0xF7
    add("short/c5-overrun", bytes.fromhex("c501020304"))
    add("other/05", b"\x05")
    add("other/string-200", _rlp_str(bytes(rng.integers(0, 256, 198, dtype=np.uint8))))
    add("other/list-200", _rlp_list([_rlp_int(1), _rlp_str(bytes(rng.integers(1, 256, 129, dtype=np.uint8))), _rlp_str(EMPTY_ROOT),
                                     _rlp_str(EMPTY_CODE)]))
    assert len(out[-1][1]) == 200 and len(out[-2][1]) == 200
    return out


SLOT_FAMILIES = {"valid": {True}, "noncanonical": {False}, "lead0": {False}, "empty": {False}, "wide": {False}, "long": {False},
                 "list": {False}, "trailing": {False}, "cut": {False}}


def slot_corpus(rng):
    """(name, value bytes) of storage-leaf values: every width 1 .. 32 led by 0x01, 0x7f, 0x80, 0xff (valid) and the forms that are
    no rlp(minimal non-zero integer of at most 32 bytes)."""
    out, seen = [], set()

    def add(name, v):
        v = bytes(v)
        assert v and v not in seen, name
        seen.add(v)
        out.append((name, v))

    for w in range(1, 33):
        for lead in (0x01, 0x7F, 0x80, 0xFF):
            add(f"valid/{w}/{lead:02x}", _rlp_str(bytes([lead]) + bytes(rng.integers(0, 256, w - 1, dtype=np.uint8))))
    for x in (0x02, 0x05, 0x7E):
        add(f"noncanonical/81-{x:02x}", bytes([0x81, x]))
    add("noncanonical/b8-01", bytes.fromhex("b80190"))
    add("noncanonical/b8-20", bytes([0xB8, 0x20]) + b"\x07" * 32)
    add("noncanonical/b9-0020", bytes([0xB9, 0x00, 0x20]) + b"\x07" * 32)
    add("lead0/00", b"\x00")
    add("lead0/81-00", b"\x81\x00")
    add("lead0/82", bytes.fromhex("820005"))
    add("lead0/a0", b"\xa0\x00" + b"\x09" * 31)
    add("empty/80", b"\x80")
    add("wide/33", b"\xa1" + b"\x07" * 33)
    add("wide/55", b"\xb7" + b"\x07" * 55)
    add("long/56", _rlp_str(b"\x07" * 56))
    add("long/120", _rlp_str(b"\x07" * 120))
    add("list/c0", b"\xc0")
    add("list/c1", b"\xc1\x05")
    add("list/c2", bytes.fromhex("c28190"))
    add("list/of-32", _rlp_list([_rlp_str(b"\x07" * 32)]))
    add("trailing/05-00", b"\x05\x00")
    add("trailing/81", bytes.fromhex("819000"))
    add("trailing/a0", b"\xa0" + b"\x07" * 32 + b"\x01")
    add("cut/82", bytes.fromhex("8290"))
    add("cut/a0", b"\xa0" + b"\x07" * 31)
    add("cut/b8", b"\xb8")
    return out


def families(corpus, decode):
    """-> ({family: set of outcomes (True = decodes)}, how many decode, how many do not) of a corpus under `decode`"""
    fam, n_ok = {}, 0
    for name, body in corpus:
        ok = decode(body) is not None
        fam.setdefault(name.split("/")[0], set()).add(ok)
        n_ok += ok
    return fam, n_ok, len(corpus) - n_ok


def state_of_leaves(oracle, leaves):
    """a state trie whose leaf bodies are given as {address: bytes} -> (trie, {node: None} of every node on a path to a leaf)"""
    kv = sorted((oracle.keccak256(a), v) for a, v in leaves.items())
    assert len(set(k for k, _ in kv)) == len(kv)
    t = oracle.Trie([k for k, _ in kv], [v for _, v in kv])
    nodes = {}
    for k, _ in kv:
        for nd in t.prove(k):
            nodes[nd] = None
    return t, nodes


def address(i: int) -> bytes:
    return b"\xad" + i.to_bytes(19, "big")


def code_owner_doc(oracle, codes, digests, rng=None):
    """A witness whose codes are `codes` (as given, in order) and whose accounts -- one per entry of `digests`, address(i) -- carry
    that entry as codeHash.  -> (doc, state root)"""
    leaves = {address(i): _rlp_list(_account_items(i + 1, 1000 + i, EMPTY_ROOT, d)) for i, d in enumerate(digests)}
    t, nodes = state_of_leaves(oracle, leaves)
    uniq = list(nodes)
    if rng is not None:
        uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    return {"state": [_hex(x) for x in uniq], "codes": [_hex(c) for c in codes],
            "keys": [_hex(address(i)) for i in range(len(digests))]}, t.root()


def first_index(oracle, codes):
    """-> ({digest: the lowest index of a code with that digest}, [the digest of each code])"""
    first, dig = {}, []
    for k, c in enumerate(codes):
        d = oracle.keccak256(c)
        dig.append(d)
        first.setdefault(d, k)
    return first, dig


def prestate_ref(oracle, doc, state_root: bytes, strict: bool = False) -> dict:
    """The outputs of phant_exec_witness_prestate for the document `doc` (a dict) against `state_root`.  strict: the leaves are
    decoded by the general decoder (strict_account / strict_slot) and not by the kernel's mirror."""
    dec_account, dec_slot = (strict_account, strict_slot) if strict else (decode_account, decode_slot)
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
                acc = dec_account(blob[int(voff[i]):int(voff[i]) + int(vlen[i])].tobytes())
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
                v = dec_slot(blob[int(voff[j]):int(voff[j]) + int(vlen[j])].tobytes())
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
