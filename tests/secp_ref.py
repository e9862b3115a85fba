"""TEST INFRASTRUCTURE: the reference the secp256k1 kernels are checked against, in Python integers.

Written from SEC 1 (v2) section 4.1.6 "Public Key Recovery Operation" and section 4.1.3 (signing), the curve parameters of SEC 2
section 2.4.1, and src/signer/signer.zig:40-188 for the transaction side; Keccak comes from the oracle.  It defines an answer --
a status, and for OK a public key -- for EVERY tuple (z, r, s, recid), genuine signature or not, with the checks in the order
include/phant_gpu.h states them, and for every byte string offered as a transaction."""
import hashlib
import hmac

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
OK, BAD_RANGE, HIGH_S, BAD_RECID, NOT_ON_CURVE, INFINITY, BAD_TX, BAD_V = range(8)
LOW_S = 1


# ------------------------------------------------------------------------------------------------- the group (None = infinity)
def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def mul(k, pt):
    k %= N
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def lift_x(x, odd):
    """the curve point with this x (< P) and this parity of y, or None"""
    rhs = (x ** 3 + 7) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return (x, y if (y & 1) == odd else P - y)


# ------------------------------------------------------------------------------------------------------------ recovery
def recover(z, r, s, recid, flags=0):
    """-> (status, public key point or None)"""
    if recid > 3:
        return BAD_RECID, None
    if r == 0 or r >= N or s == 0 or s >= N:
        return BAD_RANGE, None
    if (flags & LOW_S) and s > N // 2:
        return HIGH_S, None
    x = r + (N if recid & 2 else 0)
    if x >= P:
        return BAD_RECID, None
    R = lift_x(x, recid & 1)
    if R is None:
        return NOT_ON_CURVE, None
    ri = pow(r, -1, N)
    q = add(mul(-z * ri % N, G), mul(s * ri % N, R))
    if q is None:
        return INFINITY, None
    return OK, q


def pubkey_bytes(q):
    return q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


def address(oracle, q):
    return oracle.keccak256(pubkey_bytes(q))[12:]


def recover_batch(oracle, tuples, flags=0):
    """[(z, r, s, recid)] -> (status bytes, 64-byte keys, 20-byte addresses); a failed item's outputs are zero"""
    st, pk, ad = bytearray(), [], []
    for z, r, s, recid in tuples:
        code, q = recover(z, r, s, recid, flags)
        st.append(code)
        pk.append(pubkey_bytes(q) if code == OK else bytes(64))
        ad.append(address(oracle, q) if code == OK else bytes(20))
    return bytes(st), pk, ad


# ------------------------------------------------------------------------------------------- signing (for test inputs only)
def _nonce(d, z):
    """RFC 6979 section 3.2 with HMAC-SHA256: deterministic, and any k in [1, n) gives a valid signature"""
    x, h = d.to_bytes(32, "big"), (z % N).to_bytes(32, "big")
    v, k = b"\x01" * 32, b"\x00" * 32
    k = hmac.new(k, v + b"\x00" + x + h, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    k = hmac.new(k, v + b"\x01" + x + h, hashlib.sha256).digest()
    v = hmac.new(k, v, hashlib.sha256).digest()
    while True:
        v = hmac.new(k, v, hashlib.sha256).digest()
        t = int.from_bytes(v, "big")
        if 1 <= t < N:
            return t
        k = hmac.new(k, v + b"\x00", hashlib.sha256).digest()
        v = hmac.new(k, v, hashlib.sha256).digest()


def sign(d, z, low_s=True):
    """-> (r, s, recid) of private key d over the 256-bit digest z (SEC 1 section 4.1.3)"""
    k = _nonce(d, z)
    while True:
        R = mul(k, G)
        r = R[0] % N
        s = pow(k, -1, N) * (z + r * d) % N
        if r and s:
            break
        k = k % (N - 1) + 1
    recid = (R[1] & 1) | (2 if R[0] >= N else 0)
    if low_s and s > N // 2:
        s, recid = N - s, recid ^ 1
    return r, s, recid


def high_s_twin(r, s, recid):
    """the other signature of the same key over the same digest"""
    return r, N - s, recid ^ 1


# -------------------------------------------------------------------------------------------------------------- RLP
def rlp_bytes(b):
    if len(b) == 1 and b[0] < 0x80:
        return bytes(b)
    return _hdr(0x80, len(b)) + bytes(b)


def rlp_int(v):
    return rlp_bytes(v.to_bytes((v.bit_length() + 7) // 8, "big"))


def rlp_list(items):
    body = b"".join(items)
    return _hdr(0xC0, len(body)) + body


def _hdr(base, n):
    if n <= 55:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def rlp_item(b, pos, end):
    """one canonical item of b[pos:end) -> (is_list, payload start, payload end, item end), or None"""
    if pos >= end:
        return None
    p = b[pos]
    if p < 0x80:
        return False, pos, pos + 1, pos + 1
    if p <= 0xB7 or 0xC0 <= p <= 0xF7:
        is_list = p >= 0xC0
        n = p - (0xC0 if is_list else 0x80)
        if pos + 1 + n > end:
            return None
        if not is_list and n == 1 and b[pos + 1] < 0x80:
            return None
        return is_list, pos + 1, pos + 1 + n, pos + 1 + n
    is_list = p >= 0xF8
    ll = p - (0xF7 if is_list else 0xB7)
    if pos + 1 + ll > end or b[pos + 1] == 0:
        return None
    n = int.from_bytes(b[pos + 1:pos + 1 + ll], "big")
    if n <= 55 or n > end - pos - 1 - ll:
        return None
    return is_list, pos + 1 + ll, pos + 1 + ll + n, pos + 1 + ll + n


def _items(b, start, end):
    out, pos = [], start
    while pos < end:
        it = rlp_item(b, pos, end)
        if it is None:
            return None
        out.append((it[0], pos, it[1], it[2], it[3]))  # (is_list, item start, payload start, payload end, item end)
        pos = it[3]
    return out


def _uint(b, it, width):
    return not it[0] and it[3] - it[2] <= width and (it[3] == it[2] or b[it[2]] != 0)


def _access_list(b, it):
    if not it[0]:
        return False
    entries = _items(b, it[2], it[3])
    if entries is None:
        return False
    for e in entries:
        if not e[0]:
            return False
        parts = _items(b, e[2], e[3])
        if parts is None or len(parts) != 2 or parts[0][0] or parts[0][3] - parts[0][2] != 20 or not parts[1][0]:
            return False
        keys = _items(b, parts[1][2], parts[1][3])
        if keys is None or any(k[0] or k[3] - k[2] != 32 for k in keys):
            return False
    return True


# field widths in bytes, in order; "to", "data" and "al" (access list) are special
_LAYOUT = {0: [8, 32, 8, "to", 32, "data"],
           1: [8, 8, 32, 8, "to", 32, "data", "al"],
           2: [8, 8, 32, 32, 8, "to", 32, "data", "al"]}


def tx_signing_parts(tx, chain_id):
    """raw transaction -> (OK, preimage, r, s, recid) or (BAD_TX | BAD_V, None, 0, 0, 0)"""
    bad = (BAD_TX, None, 0, 0, 0)
    tx = bytes(tx)
    if not tx:
        return bad
    typ, start = 0, 0
    if tx[0] < 0x80:
        typ, start = tx[0], 1
        if typ not in (1, 2):
            return bad
    top = rlp_item(tx, start, len(tx))
    if top is None or not top[0] or top[3] != len(tx):
        return bad
    its = _items(tx, top[1], top[2])
    layout = _LAYOUT[typ]
    if its is None or len(its) != len(layout) + 3:
        return bad
    for it, kind in zip(its, layout):
        if kind == "to":
            if it[0] or it[3] - it[2] not in (0, 20):
                return bad
        elif kind == "data":
            if it[0]:
                return bad
        elif kind == "al":
            if not _access_list(tx, it):
                return bad
        elif not _uint(tx, it, kind):
            return bad
    v_it, r_it, s_it = its[-3:]
    if not (_uint(tx, v_it, 32) and _uint(tx, r_it, 32) and _uint(tx, s_it, 32)):
        return bad
    v, r, s = (int.from_bytes(tx[i[2]:i[3]], "big") for i in (v_it, r_it, s_it))
    tail = b""
    if typ == 0:
        if v in (27, 28):
            recid = v - 27
        elif v in (35 + 2 * chain_id, 36 + 2 * chain_id):
            recid = v - 35 - 2 * chain_id
            tail = rlp_int(chain_id) + b"\x80\x80"
        else:
            return BAD_V, None, 0, 0, 0
    else:
        if v > 1:
            return BAD_V, None, 0, 0, 0
        recid = v
    body = tx[top[1]:v_it[1]] + tail
    pre = (bytes([typ]) if typ else b"") + _hdr(0xC0, len(body)) + body
    return OK, pre, r, s, recid


def tx_sender(oracle, tx, chain_id):
    """-> (status, 20-byte address; zero unless OK)"""
    st, pre, r, s, recid = tx_signing_parts(tx, chain_id)
    if st != OK:
        return st, bytes(20)
    st, q = recover(int.from_bytes(oracle.keccak256(pre), "big"), r, s, recid, LOW_S)
    return st, (address(oracle, q) if st == OK else bytes(20))


def make_tx(oracle, d, typ, chain_id, nonce=0, gas_price=10**9, gas=21000, to=b"\x11" * 20, value=1, data=b"", access_list=(),
            eip155=True, max_priority=2, high_s=False, v_override=None):
    """a signed raw transaction of private key d (typ 0: legacy, 1, 2)"""
    al = rlp_list([rlp_list([rlp_bytes(a), rlp_list([rlp_bytes(k) for k in keys])]) for a, keys in access_list])
    if typ == 0:
        fields = [rlp_int(nonce), rlp_int(gas_price), rlp_int(gas), rlp_bytes(to), rlp_int(value), rlp_bytes(data)]
        pre = rlp_list(fields + ([rlp_int(chain_id), b"\x80", b"\x80"] if eip155 else []))
    elif typ == 1:
        fields = [rlp_int(chain_id), rlp_int(nonce), rlp_int(gas_price), rlp_int(gas), rlp_bytes(to), rlp_int(value), rlp_bytes(data), al]
        pre = b"\x01" + rlp_list(fields)
    else:
        fields = [rlp_int(chain_id), rlp_int(nonce), rlp_int(max_priority), rlp_int(gas_price), rlp_int(gas), rlp_bytes(to), rlp_int(value),
                  rlp_bytes(data), al]
        pre = b"\x02" + rlp_list(fields)
    r, s, recid = sign(d, int.from_bytes(oracle.keccak256(pre), "big"))
    if high_s:
        r, s, recid = high_s_twin(r, s, recid)
    v = recid if typ else (recid + (35 + 2 * chain_id if eip155 else 27))
    if v_override is not None:
        v = v_override
    raw = rlp_list(fields + [rlp_int(v), rlp_int(r), rlp_int(s)])
    return (bytes([typ]) if typ else b"") + raw


# ------------------------------------------------------------------------------------------------------- known answers
def load_vectors():
    """tests/golden/sender_vectors.json (tests/golden/make_sender_vectors.py) with every transaction as bytes under "tx" """
    import base64
    import json
    import os
    import zlib
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sender_vectors.json")) as f:
        doc = json.load(f)
    for group in (doc["mainnet"], doc["fixtures"]):
        for t in group:
            t["tx"] = bytes.fromhex(t["tx"]) if "tx" in t else zlib.decompress(base64.b64decode(t.pop("tx_zlib_b64")))
    return doc
