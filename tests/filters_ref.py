"""A plain-Python definition of every output of phant_block_log_filters and phant_log_filters_bloom, written from the rules of
include/phant_gpu.h (eth_getLogs' semantics): set membership on `bytes` for the exact call, the oracle's Keccak-256 for the bits of the
bloom call.  No device, no library.  tests/test_filters_ref.py holds it against tests/receipts_seg_ref.py's blooms;
tests/test_gpu_log_filters.py and tests/test_gpu_bloom_filters.py hold the device against it."""
import functools

import numpy as np

from oracle import oracle as O

MATCH_OUTPUTS = ("filter_first", "match_log", "filter_count")


class Filter:
    """addresses: 20-byte strings (none: any address); topics: up to four lists of 32-byte strings, list p the values topic p may take
    (an empty list: anything, or no topic at all); lo, hi: the blocks [lo, hi), None = from the first / to the last"""

    def __init__(self, addresses=(), topics=(), lo=None, hi=None):
        self.addresses = [bytes(a) for a in addresses]
        self.topics = ([[bytes(t) for t in ts] for ts in topics] + [[], [], [], []])[:4]
        self.lo, self.hi = lo, hi
        self.address_set, self.topic_sets = set(self.addresses), [set(ts) for ts in self.topics]
        assert all(len(a) == 20 for a in self.addresses) and all(len(t) == 32 for ts in self.topics for t in ts) and len(list(topics)) <= 4


def pack(filters):
    """-> (the arrays of phant_log_filters (never empty; block_lo and block_hi None: `ranges` makes them), n_filters, n_addr, n_topic)"""
    addr = [a for f in filters for a in f.addresses]
    topic = [t for f in filters for ts in f.topics for t in ts]
    a = {"addr_first": np.cumsum([0] + [len(f.addresses) for f in filters]).astype(np.uint32),
         "addr": np.frombuffer(b"".join(addr) or bytes(20), np.uint8).copy(),
         "topic_first": np.cumsum([0] + [len(ts) for f in filters for ts in f.topics]).astype(np.uint32),
         "topic": np.frombuffer(b"".join(topic) or bytes(32), np.uint8).copy(), "block_lo": None, "block_hi": None}
    return a, len(filters), len(addr), len(topic)


def ranges(filters, n):
    """-> (block_lo, block_hi) with every None filled in for a call over n blocks (or blooms)"""
    return (np.asarray([0 if f.lo is None else f.lo for f in filters] or [0], np.uint32),
            np.asarray([n if f.hi is None else f.hi for f in filters] or [0], np.uint32))


def log_matches(f, block, address, topics, n_blocks):
    lo, hi = 0 if f.lo is None else f.lo, n_blocks if f.hi is None else f.hi
    if not lo <= block < hi:
        return False
    if f.addresses and bytes(address) not in f.address_set:
        return False
    for p, ts in enumerate(f.topic_sets):
        if ts and (len(topics) <= p or bytes(topics[p]) not in ts):
            return False
    return True


def rows_logs(rows):
    """the rows of the logs as phant_block_receipt_segments answers them -> [(block, address, [topics])] in log order, n_blocks"""
    block_first, log_first, topic_first = (np.asarray(rows[k]).astype(np.int64).tolist() for k in ("block_first", "log_first", "topic_first"))
    address, topics = np.asarray(rows["address"], np.uint8).tobytes(), np.asarray(rows["topics"], np.uint8).tobytes()
    nb, out = len(block_first) - 1, []
    for b in range(nb):
        for l in range(log_first[block_first[b]], log_first[block_first[b + 1]]):
            out.append((b, address[20 * l:20 * l + 20], [topics[32 * t:32 * t + 32] for t in range(topic_first[l], topic_first[l + 1])]))
    return out, nb


def expected_matches(rows, filters):
    """-> ({output: bytes}, n_matches): match_log ordered by filter, then by log"""
    logs, nb = rows_logs(rows)
    first, match = [0], []
    for f in filters:
        match += [l for l, (b, a, ts) in enumerate(logs) if log_matches(f, b, a, ts, nb)]
        first.append(len(match))
    return {"filter_first": np.asarray(first, "<u4").tobytes(), "match_log": np.asarray(match, "<u4").tobytes(),
            "filter_count": np.diff(np.asarray(first, np.int64)).astype("<u4").tobytes()}, len(match)


# ------------------------------------------------------------------------------------------------------------- blooms
@functools.lru_cache(maxsize=None)
def bloom_values(entry):
    """the three 11-bit values of an address or a topic: the low 11 bits of the big-endian 16-bit words at bytes 0, 2, 4 of its Keccak-256"""
    h = O.keccak256(entry)
    return [int.from_bytes(h[2 * i:2 * i + 2], "big") & 0x7FF for i in range(3)]


def bloom_bits(entry):
    """-> [(byte of the 256, mask inside it)] x 3: value v is bit 7 - (2047 - v) % 8 of byte (2047 - v) // 8"""
    return [((2047 - v) // 8, 1 << (7 - (2047 - v) % 8)) for v in bloom_values(bytes(entry))]


def bloom_of(entries):
    """the 256 bytes with the bits of every entry set"""
    out = bytearray(256)
    for e in entries:
        for byte, mask in bloom_bits(e):
            out[byte] |= mask
    return bytes(out)


def in_bloom(bloom, entry):
    return all(bloom[byte] & mask for byte, mask in bloom_bits(entry))


def bloom_may(f, b, bloom, n_blooms):
    lo, hi = 0 if f.lo is None else f.lo, n_blooms if f.hi is None else f.hi
    if not lo <= b < hi:
        return False
    return all(not s or any(in_bloom(bloom, e) for e in s) for s in [f.addresses] + f.topics)


def expected_may(blooms, filters):
    """blooms: a list of 256-byte strings -> (may as bytes of little-endian 64-bit words, may_count as bytes)"""
    n, words = len(blooms), (len(blooms) + 63) // 64
    may = np.zeros((len(filters), words), np.uint64)
    for i, f in enumerate(filters):
        for b, bloom in enumerate(blooms):
            if bloom_may(f, b, bloom, n):
                may[i, b // 64] |= np.uint64(1 << (b % 64))
    count = np.asarray([sum(bin(int(w)).count("1") for w in row) for row in may], "<u4")
    return may.astype("<u8").tobytes(), count.tobytes()
