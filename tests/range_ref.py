"""The definition of phant_mpt_verify_ranges (include/phant_gpu.h) in plain Python: tests/test_range_ref.py holds it against answers
that owe nothing to it, the GPU and the emulated tests hold the library against it.

    verify(root, origin, leaves, has_proof, table) -> (status, has_more, computed_root, bad_leaf)

leaves: [(key32, value)], table: {keccak256(node): node} (table_of(nodes)).  bad_leaf is the index inside `leaves` (NO_LEAF: none);
verify_call() adds the ranges' offsets as the library does.  Hashing goes through oracle.keccak256; everything else is restated here:
canonical RLP as phant_amd/csrc/rlp.h decodes it, a node is a list of 17 or of 2 items, the hex-prefix rules."""
from oracle import oracle

VALID, EMPTY_VALUE, VALUE_TOO_LONG, BAD_ORDER, BELOW_ORIGIN, ROOT_MISMATCH = 1, 32, 33, 34, 35, 36
BAD_NODE, MISSING_NODE = 18, 20
NO_LEAF = 0xFFFFFFFF
MAX_VALUE = 560
EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")
ZERO = bytes(32)


class Mismatch(Exception):
    pass


class WalkError(Exception):
    def __init__(self, status):
        self.status = status


def nibbles(key):
    return tuple(x for b in key for x in (b >> 4, b & 15))


def table_of(nodes):
    return {oracle.keccak256(bytes(n)): bytes(n) for n in nodes}


# ---------------------------------------------------------------- RLP
def rlp_str(s):
    if len(s) == 1 and s[0] < 0x80:
        return bytes(s)
    return _hdr(0x80, len(s)) + bytes(s)


def rlp_list(payload):
    return _hdr(0xC0, len(payload)) + payload


def _hdr(base, n):
    if n <= 55:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def hex_prefix(nibs, leaf):
    flag = (2 if leaf else 0) + (len(nibs) & 1)
    nibs = ([flag, 0] if len(nibs) % 2 == 0 else [flag]) + list(nibs)
    return bytes(nibs[i] << 4 | nibs[i + 1] for i in range(0, len(nibs), 2))


def rlp_item(b, at, avail):
    """one canonical item at b[at:at + avail] -> (payload offset, payload length, total, is_list) or None"""
    if avail == 0:
        return None
    x = b[at]
    if x < 0x80:
        return at, 1, 1, False
    if x <= 0xB7 or 0xC0 <= x <= 0xF7:
        is_list = x >= 0xC0
        n = x - (0xC0 if is_list else 0x80)
        if 1 + n > avail or (not is_list and n == 1 and b[at + 1] < 0x80):
            return None
        return at + 1, n, 1 + n, is_list
    is_list = x >= 0xF8
    ll = x - (0xF7 if is_list else 0xB7)
    if 1 + ll > avail or b[at + 1] == 0:
        return None
    n = int.from_bytes(b[at + 1:at + 1 + ll], "big")
    if n <= 55 or n > avail - 1 - ll:
        return None
    return at + 1 + ll, n, 1 + ll + n, is_list


def _ref_kind(it):
    pay, n, total, is_list = it
    if is_list:
        return "embed" if total < 32 else "bad"
    return "empty" if n == 0 else "hash" if n == 32 else "bad"


def decode_node(b):
    """-> ("branch", [16 references]) / ("leaf", path nibbles, value) / ("ext", path nibbles, reference) or None.  A reference is
    b"" (empty), 32 bytes (a hash) or the whole encoding of an embedded node (a list shorter than 32 bytes)."""
    outer = rlp_item(b, 0, len(b))
    if outer is None or outer[2] != len(b) or not outer[3]:
        return None
    items, off = [], 0
    while off < outer[1]:
        if len(items) == 17:
            return None
        it = rlp_item(b, outer[0] + off, outer[1] - off)
        if it is None:
            return None
        items.append(it)
        off += it[2]

    def ref(it):
        k = _ref_kind(it)
        return b"" if k == "empty" else b[it[0]:it[0] + 32] if k == "hash" else b[it[0] - (it[2] - it[1]):it[0] + it[1]]

    if len(items) == 17:
        if any(_ref_kind(it) == "bad" for it in items[:16]) or items[16][3]:
            return None
        return ("branch", [ref(it) for it in items[:16]], b[items[16][0]:items[16][0] + items[16][1]])
    if len(items) != 2:
        return None
    pay, n, _, is_list = items[0]
    if is_list or n == 0 or n > 33:
        return None
    flag = b[pay] >> 4
    if flag > 3 or (not flag & 1 and b[pay] & 15):
        return None
    path = nibbles(b[pay:pay + n])[1 if flag & 1 else 2:]
    if flag & 2:
        if items[1][3]:
            return None
        return ("leaf", path, b[items[1][0]:items[1][0] + items[1][1]])
    if not path or _ref_kind(items[1]) in ("bad", "empty"):
        return None
    return ("ext", path, ref(items[1]))


# ---------------------------------------------------------------- the walks
def slots_of(nib, right):
    """the slots of a branch a walker emits where its key has nibble nib: those below it (the origin's walker), those above it (the last
    key's)"""
    return range(nib + 1, 16) if right else range(nib)


def diverging(path, mine, right):
    """a leaf / an extension with `path` where the walker's key has the nibbles `mine`: the walker's to emit?  The origin's walker emits
    what is smaller, the last key's what is greater; the other lies in the range"""
    return (path > mine) == right


def walk(root, key, table, right):
    """What the path of `key` leaves to its left (right: to its right) -> [(path, kind, payload)] in path order; kind "leaf" (payload:
    the value), "ref" (a reference of unknown type), "branch" (a reference known to be a branch)."""
    key, out, pos = nibbles(key), [], 0
    if root == EMPTY_ROOT:
        return out
    ref, front, back = root, [], []
    while True:
        if len(ref) == 32:
            if ref not in table:
                raise WalkError(MISSING_NODE)
            node = table[ref]
        else:
            node = ref
        n = decode_node(node)
        if n is None:
            raise WalkError(BAD_NODE)
        if n[0] == "branch":
            if pos >= 64 or n[2]:
                raise WalkError(BAD_NODE)
            here = [(key[:pos] + (s,), "ref", n[1][s]) for s in slots_of(key[pos], right) if n[1][s]]
            if right:
                back = here + back
            else:
                front += here
            ref = n[1][key[pos]]
            pos += 1
            if not ref:
                break
            continue
        path = n[1]
        if pos + len(path) > 64 or (n[0] == "leaf" and pos + len(path) != 64):
            raise WalkError(BAD_NODE)
        mine = key[pos:pos + len(path)]
        if path == mine:
            if n[0] == "leaf":
                break
            pos += len(path)
            ref = n[2]
            continue
        if diverging(path, mine, right):
            item = (key[:pos] + path, "leaf" if n[0] == "leaf" else "branch", n[2])
            if right:
                back = [item] + back
            else:
                front.append(item)
        break
    return back if right else front


# ---------------------------------------------------------------- the build
def _ref_of(node, force=False):
    return node if len(node) < 32 and not force else oracle.keccak256(node)


def _ref_item(ref):
    return b"\xa0" + ref if len(ref) == 32 else ref


def _node(items, d):
    """the encoding of the node over `items`, which share their first d nibbles (never a lone reference that has no nibble left)"""
    if len(items) == 1:
        path, kind, payload = items[0]
        rest = path[d:]
        if kind == "leaf":
            if len(payload) > MAX_VALUE:
                raise Mismatch
            return rlp_list(rlp_str(hex_prefix(rest, True)) + rlp_str(payload))
        if kind != "branch":
            raise Mismatch  # a reference of unknown type under nibbles of its own: never looked up
        return rlp_list(rlp_str(hex_prefix(rest, False)) + _ref_item(payload))
    lcp = d
    while all(len(p) > lcp for p, _, _ in items) and len({p[lcp] for p, _, _ in items}) == 1:
        lcp += 1
    if any(len(p) <= lcp for p, _, _ in items):
        raise Mismatch  # one path inside another
    slots = [b"\x80"] * 17
    for s in range(16):
        sub = [it for it in items if it[0][lcp] == s]
        if sub:
            slots[s] = _ref_item(_child(sub, lcp + 1))
    branch = rlp_list(b"".join(slots))
    if lcp == d:
        return branch
    return rlp_list(rlp_str(hex_prefix(items[0][0][d:lcp], False)) + _ref_item(_ref_of(branch)))


def _child(items, d):
    """the reference that fills a branch's slot at depth d - 1"""
    if len(items) == 1 and items[0][1] != "leaf" and len(items[0][0]) == d:
        return items[0][2]  # the reference as it is
    return _ref_of(_node(items, d))


def build_root(items):
    """the root of the trie over a strictly ordered, prefix-free item list (Mismatch: it is not one, or cannot be built)"""
    if not items:
        return EMPTY_ROOT
    for a, b in zip(items, items[1:]):
        m = min(len(a[0]), len(b[0]))
        if a[0][:m] >= b[0][:m]:
            raise Mismatch
    return oracle.keccak256(_node(items, 0))  # (a root is always hashed)


# ---------------------------------------------------------------- the definition
def leaf_rules(origin, leaves, has_proof):
    """-> (status, index) of the least leaf that breaks a rule, or (0, NO_LEAF)"""
    for j, (k, v) in enumerate(leaves):
        if len(v) == 0:
            return EMPTY_VALUE, j
        if len(v) > MAX_VALUE:
            return VALUE_TOO_LONG, j
        if j and k <= leaves[j - 1][0]:
            return BAD_ORDER, j
        if j == 0 and has_proof and k < origin:
            return BELOW_ORIGIN, j
    return 0, NO_LEAF


def verify(root, origin, leaves, has_proof, table):
    st, j = leaf_rules(origin, leaves, has_proof)
    if st:
        return st, 0, ZERO, j
    items, more = [], False
    try:
        if has_proof:
            items += walk(root, origin, table, False)
        items += [(nibbles(k), "leaf", bytes(v)) for k, v in leaves]
        if has_proof and leaves:
            right = walk(root, leaves[-1][0], table, True)
            more = bool(right)
            items += right
    except WalkError as e:
        return e.status, 0, ZERO, NO_LEAF
    try:
        got = build_root(items)
    except Mismatch:
        return ROOT_MISMATCH, 0, ZERO, NO_LEAF
    if got != root:
        return ROOT_MISMATCH, 0, ZERO, NO_LEAF
    return VALID, int(more), got, NO_LEAF


def verify_call(ranges, nodes):
    """ranges: [(root, origin, leaves, has_proof)] over one node set -> the call's outputs as lists, bad_leaf counted over the call"""
    table, first, out = table_of(nodes), 0, []
    for root, origin, leaves, has_proof in ranges:
        st, more, got, j = verify(bytes(root), bytes(origin or ZERO), [(bytes(k), bytes(v)) for k, v in leaves], bool(has_proof), table)
        out.append((st, more, got, NO_LEAF if j == NO_LEAF else first + j))
        first += len(leaves)
    return out
