"""TEST REFERENCE: what phant_block_access_lists answers (include/phant_gpu.h), in plain Python -- its own RLP walk over every span,
dicts for the joins with the witness's tables, `min` for the "same" indices.  It never calls into the library.  A span is the payload
of an access list: [[address20, [key32, ...]], ...] without the outer list header."""
import numpy as np

NONE = 0xFFFFFFFF
MALFORMED, DUPLICATES = 1, 2
# the outputs in the order of phant_access_out: (name, numpy dtype, elements per row, the count its rows follow, rows beyond that count)
OUTPUTS = (("tuple_first", "u4", 1, "n", 1), ("al_flags", "u4", 1, "n", 0), ("warm_addresses", "u4", 1, "n", 0), ("warm_keys", "u4", 1, "n", 0),
           ("address", "u1", 20, "n_tuples", 0), ("key_first", "u4", 1, "n_tuples", 1), ("account_row", "u4", 1, "n_tuples", 0),
           ("tuple_same", "u4", 1, "n_tuples", 0), ("key", "u1", 32, "n_keys", 0), ("slot_row", "u4", 1, "n_keys", 0), ("key_same", "u4", 1, "n_keys", 0))
TOTALS = ("n_tuples", "n_keys", "n_missing_accounts", "n_missing_slots", "first_malformed")


# ------------------------------------------------------------------------------------------------------------ RLP, both ways
def rlp_header(base, payload_len):
    if payload_len <= 55:
        return bytes([base + payload_len])
    be = payload_len.to_bytes((payload_len.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def rlp_str(b):
    b = bytes(b)
    return b if len(b) == 1 and b[0] < 0x80 else rlp_header(0x80, len(b)) + b


def rlp_list(payload):
    return rlp_header(0xC0, len(payload)) + bytes(payload)


def encode(entries):
    """[(address, [key, ...]), ...] -> the list's payload (what al_off / al_len span)"""
    return b"".join(rlp_list(rlp_str(a) + rlp_list(b"".join(rlp_str(k) for k in keys))) for a, keys in entries)


def item(b, pos, end):
    """one canonical RLP item at b[pos:end] -> (payload begin, payload end, is a list), or None"""
    if pos >= end:
        return None
    c = b[pos]
    if c < 0x80:
        return pos, pos + 1, False
    if c <= 0xB7 or 0xC0 <= c <= 0xF7:
        is_list = c >= 0xC0
        ln = c - (0xC0 if is_list else 0x80)
        if pos + 1 + ln > end or (not is_list and ln == 1 and b[pos + 1] < 0x80):
            return None
        return pos + 1, pos + 1 + ln, is_list
    is_list = c >= 0xF8
    ll = c - (0xF7 if is_list else 0xB7)
    if pos + 1 + ll > end or b[pos + 1] == 0:
        return None
    ln = int.from_bytes(b[pos + 1:pos + 1 + ll], "big")
    if ln <= 55 or pos + 1 + ll + ln > end:
        return None
    return pos + 1 + ll, pos + 1 + ll + ln, is_list


def walk(span):
    """the span's entries [(address, [key, ...]), ...], or None when it is no well-formed access-list payload"""
    span = bytes(span)
    out, pos, end = [], 0, len(span)
    while pos < end:
        t = item(span, pos, end)
        if t is None or not t[2]:
            return None
        a = item(span, t[0], t[1])
        if a is None or a[2] or a[1] - a[0] != 20:
            return None
        ks = item(span, a[1], t[1])
        if ks is None or not ks[2] or ks[1] != t[1]:
            return None
        keys, kp = [], ks[0]
        while kp < ks[1]:
            k = item(span, kp, ks[1])
            if k is None or k[2] or k[1] - k[0] != 32:
                return None
            keys.append(span[k[0]:k[1]])
            kp = k[1]
        out.append((span[a[0]:a[1]], keys))
        pos = t[1]
    return out


# ------------------------------------------------------------------------------------------------------------ the definition
def define(spans, addresses=(), slot_first=None, slots=()):
    """-> ({output: list}, {total: int}); addresses / slot_first / slots: the witness's tables (none: nothing is joined)"""
    addresses, slots = [bytes(a) for a in addresses], [bytes(s) for s in slots]
    row_of, slot_of = {}, {}
    for j, a in enumerate(addresses):
        row_of.setdefault(a, []).append(j)
        for s in range(slot_first[j], slot_first[j + 1]):
            slot_of.setdefault((j, slots[s]), []).append(s)
    o = {name: [] for name, _, _, _, _ in OUTPUTS}
    o["tuple_first"].append(0)
    o["key_first"].append(0)
    missing_accounts = missing_slots = 0
    malformed = []
    for i, span in enumerate(spans):
        entries = walk(span)
        flags = warm_a = warm_k = 0
        if entries is None:
            flags = MALFORMED
            malformed.append(i)
        else:
            tuples_of, keys_of = {}, {}
            for a, keys in entries:
                e = len(o["address"])
                tuples_of.setdefault(a, []).append(e)
                same = min(tuples_of[a])
                row = min(row_of[a]) if a in row_of else NONE
                o["address"].append(a), o["account_row"].append(row), o["tuple_same"].append(same)
                if same == e:
                    warm_a += 1
                    missing_accounts += row == NONE
                else:
                    flags |= DUPLICATES
                for key in keys:
                    k = len(o["key"])
                    keys_of.setdefault((a, key), []).append(k)
                    ksame = min(keys_of[a, key])
                    srow = min(slot_of[row, key]) if (row, key) in slot_of else NONE
                    o["key"].append(key), o["slot_row"].append(srow), o["key_same"].append(ksame)
                    if ksame == k:
                        warm_k += 1
                        missing_slots += srow == NONE
                    else:
                        flags |= DUPLICATES
                o["key_first"].append(len(o["key"]))
        o["tuple_first"].append(len(o["address"]))
        o["al_flags"].append(flags), o["warm_addresses"].append(warm_a), o["warm_keys"].append(warm_k)
    totals = {"n_tuples": len(o["address"]), "n_keys": len(o["key"]), "n_missing_accounts": missing_accounts, "n_missing_slots": missing_slots,
              "first_malformed": min(malformed) if malformed else len(spans)}
    return o, totals


def expected(spans, addresses=(), slot_first=None, slots=()):
    """the definition's answer as the bytes the call's buffers must hold -> ({output: bytes}, totals)"""
    o, totals = define(spans, addresses, slot_first, slots)
    exp = {}
    for name, dt, k, _, _ in OUTPUTS:
        exp[name] = b"".join(o[name]) if k > 1 else np.asarray(o[name], dt).tobytes()
    return exp, totals


def inputs(spans, addresses=(), slot_first=None, slots=(), gap=b"\xf8\x00junk"):
    """the call's input arrays: the spans inside a blob with `gap` in front of, between and behind them (an empty span: 0, 0)"""
    blob, off, ln = bytearray(gap), [], []
    for s in spans:
        off.append(len(blob) if len(s) else 0), ln.append(len(s))
        blob += bytes(s) + gap
    na = len(addresses)
    return {"txs": np.frombuffer(bytes(blob), np.uint8).copy(), "al_off": np.asarray(off, np.uint64), "al_len": np.asarray(ln, np.uint32),
            "addresses": np.frombuffer(b"".join(bytes(a) for a in addresses), np.uint8).copy() if na else None,
            "slot_first": np.asarray(slot_first, np.uint32) if na else None,
            "slots": np.frombuffer(b"".join(bytes(s) for s in slots), np.uint8).copy() if len(slots) else None}
