"""A plain-Python definition of every output of phant_block_requests, written from the rules of include/phant_gpu.h (EIP-7685, EIP-6110)
with hashlib.sha256: the deposit requests rebuilt from the rows of the logs, each block's requests and its requests_hash, the flags.  No
device, no library.  tests/test_requests_ref.py holds it against known values; tests/test_gpu_requests.py holds the device against it."""
import hashlib

import numpy as np

DEPOSIT_TOPIC = bytes.fromhex("649bbc62d0e31342afea4e5cd82d4049e7e1ee912fc0889aa790803be39038c5")
EMPTY_HASH = bytes.fromhex("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")
LAYOUT, ORDER, HASH = 1, 2, 4
EVENT_BYTES, ROW_BYTES = 576, 192
OFFSETS, SIZES = (160, 256, 320, 384, 512), (48, 32, 8, 96, 8)
OUTPUTS = ("deposit_log", "deposit", "deposit_first", "requests_hash", "block_flags")
WIDTH = {"deposit_log": 4, "deposit": 192, "deposit_first": 4, "requests_hash": 32, "block_flags": 4}
PER_DEPOSIT = ("deposit_log", "deposit")


def sha256(b):
    return hashlib.sha256(bytes(b)).digest()


def requests_hash(requests):
    """[(type, data)] in the order they are committed in -> the header's requests_hash; a request without data is left out"""
    return sha256(b"".join(sha256(bytes([t]) + bytes(d)) for t, d in requests if len(d)))


def abi_bytes(values):
    """the ABI encoding of a tuple of dynamic `bytes` values, generically: a head of offsets, then each value as its length word and its
    bytes padded to a multiple of 32"""
    head, tail = b"", b""
    for v in values:
        head += (32 * len(values) + len(tail)).to_bytes(32, "big")
        tail += len(v).to_bytes(32, "big") + bytes(v) + bytes(-len(v) % 32)
    return head + tail


def deposit_event(pubkey, credentials, amount, signature, index):
    """the data of a DepositEvent log: 48, 32, 8, 96 and 8 bytes"""
    return abi_bytes([pubkey, credentials, amount, signature, index])


def is_candidate(address, topics, contract):
    return bytes(address) == bytes(contract) and len(topics) >= 1 and bytes(topics[0]) == DEPOSIT_TOPIC


def well_formed(receipts, rc_bytes, data_at, data_len):
    if data_len != EVENT_BYTES or data_at + EVENT_BYTES > rc_bytes:
        return False
    d = bytes(receipts[data_at:data_at + EVENT_BYTES])
    word = lambda at: int.from_bytes(d[at:at + 32], "big")  # noqa: E731
    return all(word(32 * k) == OFFSETS[k] for k in range(5)) and all(word(OFFSETS[k]) == SIZES[k] for k in range(5))


def deposit_row(d):
    """the event's data -> the 192 bytes of its request: pubkey, credentials, amount, signature, index as they stand"""
    return bytes(d[192:240] + d[288:320] + d[352:360] + d[416:512] + d[544:552])


def expected(a, contract, other=None, active=None, exp_hash=None, rc_bytes=None):
    """a: the rows of the logs as phant_block_receipt_segments answers them -- receipts (bytes), block_first, log_first, address (n_logs x 20
    bytes), topic_first, topics (n_topics x 32 bytes), data_at, data_len.  other: per block a list of (type, data), the caller's rows.
    active: per block, or None.  exp_hash: per block 32 bytes, or None.  -> ({output: bytes}, n_deposits, first_bad_block)"""
    receipts = bytes(np.asarray(a["receipts"], np.uint8).tobytes())
    rc_bytes = len(receipts) if rc_bytes is None else rc_bytes
    block_first, log_first, topic_first = (np.asarray(a[k]).tolist() for k in ("block_first", "log_first", "topic_first"))
    address, topics = bytes(np.asarray(a["address"], np.uint8).tobytes()), bytes(np.asarray(a["topics"], np.uint8).tobytes())
    data_at, data_len = np.asarray(a["data_at"]).tolist(), np.asarray(a["data_len"]).tolist()
    nb = len(block_first) - 1
    other = other or [[] for _ in range(nb)]
    rows, logs, deposit_first, hashes, flags = [], [], [0], [], []
    for b in range(nb):
        on = active is None or bool(active[b])
        f, mine = 0, []
        for l in range(log_first[block_first[b]], log_first[block_first[b + 1]]) if on else ():
            ts = [topics[32 * t:32 * t + 32] for t in range(topic_first[l], topic_first[l + 1])]
            if not is_candidate(address[20 * l:20 * l + 20], ts, contract):
                continue
            if well_formed(receipts, rc_bytes, data_at[l], data_len[l]):
                mine.append(deposit_row(receipts[data_at[l]:data_at[l] + EVENT_BYTES]))
                logs.append(l)
            else:
                f |= LAYOUT
        rows += mine
        deposit_first.append(len(rows))
        if not on:
            hashes.append(bytes(32)), flags.append(0)
            continue
        types = [t for t, _ in other[b]]
        if any(t == 0 or (k > 0 and t <= types[k - 1]) for k, t in enumerate(types)):
            f |= ORDER
        h = requests_hash(([(0, b"".join(mine))] if mine else []) + [(t, d) for t, d in other[b]])
        if exp_hash is not None and bytes(exp_hash[b]) != h:
            f |= HASH
        hashes.append(h), flags.append(f)
    out = {"deposit_log": np.asarray(logs, "<u4").tobytes(), "deposit": b"".join(rows), "deposit_first": np.asarray(deposit_first, "<u4").tobytes(),
           "requests_hash": b"".join(hashes), "block_flags": np.asarray(flags, "<u4").tobytes()}
    return out, len(rows), next((b for b, f in enumerate(flags) if f), nb)


def pack_other(other, nb):
    """per block a list of (type, data) -> req_block_first, req_type, req_bytes, req_off as the call takes them (never empty arrays)"""
    other = other or [[] for _ in range(nb)]
    rows = [r for b in other for r in b]
    return {"req_block_first": np.cumsum([0] + [len(b) for b in other]).astype(np.uint32), "req_type": np.asarray([t for t, _ in rows] or [0], np.uint8),
            "req_bytes": np.frombuffer(b"".join(bytes(d) for _, d in rows) or b"\x00", np.uint8).copy(),
            "req_off": np.cumsum([0] + [len(d) for _, d in rows]).astype(np.uint64)}, len(rows)
