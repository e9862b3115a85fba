"""A plain-Python reference for a block's receipts: what phant_block_receipts must answer for ANY block.  Written from the Yellow
Paper's RLP rules (appendix B), EIP-658 (the status field), EIP-2718 (the type byte in front of a typed receipt) and
src/types/receipt.zig (the field order :13-35, the bloom :37-63, Log :66-70) -- not from the kernels.  Hashing goes through the
oracle's keccak256, roots through its index_root_rlp.

A receipt here is a tuple (tx_type, succeeded, cumulative_gas_used, logs), a log a tuple (address, topics, data)."""
from oracle import oracle as O


# ---------------------------------------------------------------------------------------------------------------- RLP
def _be(v):
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def rlp_str(b):
    b = bytes(b)
    if len(b) == 1 and b[0] < 0x80:
        return b
    if len(b) < 56:
        return bytes([0x80 + len(b)]) + b
    ll = _be(len(b))
    return bytes([0xb7 + len(ll)]) + ll + b


def rlp_list(encoded_items):
    p = b"".join(encoded_items)
    if len(p) < 56:
        return bytes([0xc0 + len(p)]) + p
    ll = _be(len(p))
    return bytes([0xf7 + len(ll)]) + ll + p


def rlp_int(v):
    return rlp_str(_be(v))  # (0 is the empty string)


def rlp_decode(b):
    """One item that must span all of b -> bytes, or a list of decoded items.  Strict: canonical lengths only."""
    item, end = _decode_at(bytes(b), 0)
    if end != len(b):
        raise ValueError("trailing bytes")
    return item


def _decode_at(b, at):
    t = b[at]
    if t < 0x80:
        return b[at:at + 1], at + 1
    if t < 0xb8:
        n, body = t - 0x80, at + 1
        if n == 1 and b[body] < 0x80:
            raise ValueError("single byte below 0x80 with a header")
    elif t < 0xc0:
        ll = t - 0xb7
        n, body = int.from_bytes(b[at + 1:at + 1 + ll], "big"), at + 1 + ll
        if n < 56 or b[at + 1] == 0:
            raise ValueError("non-canonical long string")
    elif t < 0xf8:
        n, body = t - 0xc0, at + 1
    else:
        ll = t - 0xf7
        n, body = int.from_bytes(b[at + 1:at + 1 + ll], "big"), at + 1 + ll
        if n < 56 or b[at + 1] == 0:
            raise ValueError("non-canonical long list")
    if body + n > len(b):
        raise ValueError("item runs past the end")
    if t < 0xc0:
        return b[body:body + n], body + n
    items, p = [], body
    while p < body + n:
        it, p = _decode_at(b, p)
        items.append(it)
    if p != body + n:
        raise ValueError("list payload overrun")
    return items, body + n


# -------------------------------------------------------------------------------------------------------------- bloom
def bloom_of(logs):
    """receipt.zig:37-63: for every address and topic, the three bits 0x7ff - (big-endian u16 at hash[2i] & 0x7ff), i = 0..2,
    counted from the most significant bit of byte 0.  A log's data does not enter."""
    bloom = bytearray(256)
    for address, topics, _data in logs:
        for item in (address, *topics):
            h = O.keccak256(bytes(item))
            for i in range(3):
                bit_index = 0x7ff - (int.from_bytes(h[2 * i:2 * i + 2], "big") & 0x7ff)
                bloom[bit_index // 8] |= 1 << (7 - bit_index % 8)
    return bytes(bloom)


def block_bloom(receipts):
    out = bytearray(256)
    for r in receipts:
        for k, v in enumerate(bloom_of(r[3])):
            out[k] |= v
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ receipts
def encode(receipt, bloom=None):
    """bloom: the receipt's 256 bytes where the caller already has them (they are not checked); None computes them from the logs"""
    tx_type, ok, gas, logs = receipt
    body = rlp_list([rlp_int(1 if ok else 0), rlp_int(gas), rlp_str(bloom_of(logs) if bloom is None else bloom),
                     rlp_list([rlp_list([rlp_str(a), rlp_list([rlp_str(t) for t in ts]), rlp_str(d)]) for a, ts, d in logs])])
    return (bytes([tx_type]) if tx_type else b"") + body


def decode(b):
    """-> (tx_type, succeeded, cumulative_gas_used, logs); the bloom inside must be the logs' bloom."""
    b = bytes(b)
    tx_type = 0
    if b[0] < 0x80:
        tx_type, b = b[0], b[1:]
    status, gas, bloom, logs = rlp_decode(b)
    if status not in (b"\x01", b"") or (gas[:1] == b"\x00") or len(bloom) != 256:
        raise ValueError("not a receipt")
    out = []
    for address, topics, data in logs:
        if len(address) != 20 or any(len(t) != 32 for t in topics):
            raise ValueError("not a log")
        out.append((address, list(topics), data))
    if bloom != bloom_of(out):
        raise ValueError("the bloom is not the logs' bloom")
    return (tx_type, status == b"\x01", int.from_bytes(gas, "big"), out)


def receipts_root(receipts):
    return O.index_root_rlp([encode(r) for r in receipts])
