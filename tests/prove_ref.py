"""TEST INFRASTRUCTURE: what phant_mpt_prove_nodeset must emit, from the oracle's prover (oracle.Trie.prove) and the rule of
DESIGN.md section 7d for PHANT_PROVE_MAY_REMOVE, written from the key set alone: no code of the library is mirrored here."""
import numpy as np

from tests.prestate_ref import rlp_decode_strict

PRESENT, ABSENT = 1, 2
VALUE = 16  # the seventeenth position of a branch


def nibbles(key: bytes):
    return tuple(x for b in key for x in (b >> 4, b & 15))


def absent_queries(keys, rng, many=20):
    """Keys that are NOT in `keys`, one family per way a walk can end early: a nibble changed at every depth (an empty branch slot, a
    leaf that diverges, an extension that diverges in its first / any middle / last nibble -- whichever node covers that depth),
    a key shorter and a key longer than a stored one, the empty key.  Small tries get every key at every depth."""
    have = set(keys)
    out = []
    pick = list(keys) if len(keys) <= many else [keys[int(i)] for i in rng.choice(len(keys), many, replace=False)]
    for k in pick:
        nn = 2 * len(k)
        depths = range(nn) if len(keys) <= many else sorted({0, nn - 1, *[int(x) for x in rng.integers(0, nn, 5)]})
        for d in depths:
            b = bytearray(k)
            b[d >> 1] ^= (0x10 if d % 2 == 0 else 0x01) * int(rng.integers(1, 16))
            out.append(bytes(b))
        out.append(k[:-1])
        out.append(k + b"\x00")
        out.append(k + bytes(rng.integers(0, 256, 3, dtype=np.uint8)))
    out.append(b"")
    return [q for q in dict.fromkeys(out) if q not in have]


def query_list(keys, rng, many=20):
    """every present key and every kind of absent key, each twice, the whole list shuffled"""
    q = list(keys) + absent_queries(keys, rng, many)
    q = q + q
    return [q[int(i)] for i in rng.permutation(len(q))]


def oracle_union(trie, queries):
    """the set of node byte strings oracle.Trie.prove returns over `queries`"""
    out = set()
    for q in queries:
        out.update(trie.prove(q))
    return out


def statuses(keys, queries):
    have = set(keys)
    return np.array([PRESENT if q in have else ABSENT for q in queries], np.uint8)


def _hp_path_len(hp: bytes) -> int:
    return 2 * (len(hp) - 1) + (1 if hp[0] & 0x10 else 0)


def _branch_at(oracle, proof, depth):
    """the decoded 17-item node that sits at nibble depth `depth` on the proof's path (every node above a hashed branch is hashed,
    so the proof lists them all), or None"""
    pos = 0
    for node in proof:
        items = rlp_decode_strict(node)
        if len(items) == 17:
            if pos == depth:
                return items
            pos += 1
        else:
            pos += _hp_path_len(items[0])
        if pos > depth:
            return None
    return None


def sibling_nodes(oracle, trie, keys, queries, flags):
    """DESIGN.md section 7d, from the key set: a branch is a nibble prefix P under which the stored keys continue in two or more
    positions (next nibble, or VALUE for the key that ends there).  It is MARKED if some query starts with P.  Every flagged query
    that is a stored key marks its position in every branch on its path.  A marked branch with exactly one occupied position
    outside that mask, that position holding a 32-byte reference, adds the node the reference names.  -> set of node bytes."""
    kn = [nibbles(k) for k in keys]
    have = {k: i for i, k in enumerate(keys)}
    prefixes = {}
    for i, n in enumerate(kn):
        for d in range(len(n) + 1):
            prefixes.setdefault(n[:d], []).append(i)
    branches = {}
    for P, members in prefixes.items():
        occ = {}
        for i in members:
            occ.setdefault(VALUE if len(kn[i]) == len(P) else kn[i][len(P)], []).append(i)
        if len(occ) >= 2:
            branches[P] = occ
    marked, mask = set(), {}
    for q, f in zip(queries, flags):
        qn = nibbles(q)
        for d in range(len(qn) + 1):
            if qn[:d] in branches:
                marked.add(qn[:d])
                if (f & 1) and q in have:
                    mask.setdefault(qn[:d], set()).add(VALUE if len(qn) == d else qn[d])
    out = set()
    for P in marked:
        rest = [s for s in branches[P] if s not in mask.get(P, ())]
        if len(rest) != 1 or rest[0] == VALUE or not mask.get(P):
            continue
        k = keys[branches[P][rest[0]][0]]
        proof = trie.prove(k)
        br = _branch_at(oracle, proof, len(P))
        if br is None:
            continue  # the branch itself is embedded: so is everything under it
        ref = br[rest[0]]
        if not (isinstance(ref, bytes) and len(ref) == 32):
            continue
        hit = [n for n in proof if oracle.keccak256(n) == ref]
        assert len(hit) == 1
        out.add(hit[0])
    return out
