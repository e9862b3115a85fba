"""TEST INFRASTRUCTURE: the definition of phant_block_transactions in Python integers.

Written from src/types/transaction.zig:152-273 (the fields of the three types, `chainIdFromSignature`), src/blockchain/blockchain.zig:237-260
(`checkTransaction`), :262-274 (the upfront cost), :345-381 (`validateTransaction`, `calculateIntrinsicCost`, `initCodeCost`),
src/blockchain/params.zig:7-19 and src/signer/signer.zig:40-188, on top of tests/secp_ref.py (the strict decode `tx_signing_parts`, the
recovery).  It defines every output of include/phant_gpu.h's phant_txs_out for EVERY byte string offered as a transaction."""
import numpy as np

from tests import secp_ref as S

# src/blockchain/params.zig
TX_BASE_COST, TX_DATA_ZERO, TX_DATA_NON_ZERO, TX_CREATE_COST, AL_ADDRESS_COST, AL_KEY_COST = 21000, 4, 16, 32000, 2400, 1900
INIT_CODE_WORD_COST, MAX_CODE_SIZE = 2, 0x6000

# flags, in the order include/phant_gpu.h states them
UNDECODABLE, BAD_V, SIGNATURE, CHAIN_ID, PRIORITY_ABOVE_MAX, FEE_BELOW_BASE, GAS_ABOVE_BLOCK, INTRINSIC_GAS, NONCE_MAX, INITCODE_SIZE, COST_OVERFLOW, IS_CREATE = \
    (1 << k for k in range(12))
ERROR_BITS = IS_CREATE - 1
M256 = (1 << 256) - 1

# the outputs: (name, numpy dtype, elements per transaction), in the order of phant_txs_out
OUTPUTS = (("tx_hash", "u1", 32), ("sig_hash", "u1", 32), ("sender", "u1", 20), ("sig_status", "u1", 1), ("sig", "u1", 65), ("type", "u1", 1),
           ("chain_id", "u8", 1), ("nonce", "u8", 1), ("gas_limit", "u8", 1), ("gas_price", "u1", 32), ("priority_fee", "u1", 32),
           ("value", "u1", 32), ("to", "u1", 20), ("data_off", "u8", 1), ("data_len", "u4", 1), ("al_off", "u8", 1), ("al_len", "u4", 1),
           ("al_addresses", "u4", 1), ("al_keys", "u4", 1), ("intrinsic_gas", "u8", 1), ("effective_gas_price", "u1", 32),
           ("upfront_cost", "u1", 32), ("flags", "u4", 1))
_NAMES = {0: ["nonce", "gas_price", "gas_limit", "to", "value", "data"],
          1: ["chain_id", "nonce", "gas_price", "gas_limit", "to", "value", "data", "al"],
          2: ["chain_id", "nonce", "priority_fee", "gas_price", "gas_limit", "to", "value", "data", "al"]}


# ---- the recovery of tests/secp_ref.py in Jacobian coordinates: the same checks in the same order, ~10 x faster (the hostile-byte tests
# recover thousands of altered transactions); tests/test_tx_ref.py holds it against secp_ref.recover
def _jdbl(p):
    if p is None or p[1] == 0:
        return None
    x, y, z = p
    yy = y * y % S.P
    s, m = 4 * x * yy % S.P, 3 * x * x % S.P
    x2 = (m * m - 2 * s) % S.P
    return x2, (m * (s - x2) - 8 * yy * yy) % S.P, 2 * y * z % S.P


def _jadd(p, q):
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1, z1), (x2, y2, z2) = p, q
    z1z1, z2z2 = z1 * z1 % S.P, z2 * z2 % S.P
    u1, u2, s1, s2 = x1 * z2z2 % S.P, x2 * z1z1 % S.P, y1 * z2 * z2z2 % S.P, y2 * z1 * z1z1 % S.P
    if u1 == u2:
        return _jdbl(p) if s1 == s2 else None
    h, r = (u2 - u1) % S.P, (s2 - s1) % S.P
    h2 = h * h % S.P
    h3, v = h * h2 % S.P, u1 * h2 % S.P
    x3 = (r * r - h3 - 2 * v) % S.P
    return x3, (r * (v - x3) - s1 * h3) % S.P, h * z1 * z2 % S.P


def _jmul(k, pt):
    k %= S.N
    table = [None, (pt[0], pt[1], 1)]
    for _ in range(14):
        table.append(_jadd(table[-1], table[1]))
    acc = None
    for shift in range(252, -1, -4):
        for _ in range(4):
            acc = _jdbl(acc)
        acc = _jadd(acc, table[(k >> shift) & 15])
    return acc


def fast_recover(z, r, s, recid, flags=0):
    """tests/secp_ref.recover, value for value"""
    if recid > 3:
        return S.BAD_RECID, None
    if r == 0 or r >= S.N or s == 0 or s >= S.N:
        return S.BAD_RANGE, None
    if (flags & S.LOW_S) and s > S.N // 2:
        return S.HIGH_S, None
    x = r + (S.N if recid & 2 else 0)
    if x >= S.P:
        return S.BAD_RECID, None
    R = S.lift_x(x, recid & 1)
    if R is None:
        return S.NOT_ON_CURVE, None
    ri = pow(r, -1, S.N)
    q = _jadd(_jmul(-z * ri % S.N, S.G), _jmul(s * ri % S.N, R))
    if q is None or q[2] == 0:
        return S.INFINITY, None
    zi = pow(q[2], -1, S.P)
    return S.OK, (q[0] * zi * zi % S.P, q[1] * zi * zi * zi % S.P)


def decode(tx, chain_id):
    """raw transaction -> (status of tests/secp_ref.tx_signing_parts, fields or None, (preimage, r, s, recid)).  fields: integers, `to`
    (bytes, empty for a creation), the calldata's and the access list's payload spans inside tx, the list's counts"""
    tx = bytes(tx)
    st, pre, r, s, recid = S.tx_signing_parts(tx, chain_id)
    if st == S.BAD_TX:
        return st, None, None
    typ, start = (tx[0], 1) if tx[0] < 0x80 else (0, 0)
    top = S.rlp_item(tx, start, len(tx))
    its = S._items(tx, top[1], top[2])
    f = {"type": typ, "al": (0, 0), "al_addresses": 0, "al_keys": 0}
    for name, it in zip(_NAMES[typ], its):
        if name in ("to",):
            f[name] = tx[it[2]:it[3]]
        elif name == "data":
            f[name] = (it[2], it[3] - it[2])
        elif name == "al":
            f[name] = (it[2], it[3] - it[2])
            tuples = S._items(tx, it[2], it[3])
            f["al_addresses"] = len(tuples)
            f["al_keys"] = sum(len(S._items(tx, k[2], k[3])) for t in tuples for k in [S._items(tx, t[2], t[3])[1]])
        else:
            f[name] = int.from_bytes(tx[it[2]:it[3]], "big")
    f["v"] = int.from_bytes(tx[its[-3][2]:its[-3][3]], "big")
    if typ == 0:  # transaction.zig:195-202 chainIdFromSignature (for a v the signer accepts; any other v: 0)
        f["chain_id"] = (f["v"] - 35) >> 1 if st == S.OK and f["v"] not in (27, 28) else 0
    if typ != 2:
        f["priority_fee"] = f["gas_price"]
    return st, f, (pre, r, s, recid)


def intrinsic_gas(data, create, al_addresses, al_keys):
    """blockchain.zig:355-381"""
    zeros = data.count(0)
    cost = TX_BASE_COST + TX_DATA_ZERO * zeros + TX_DATA_NON_ZERO * (len(data) - zeros) + AL_ADDRESS_COST * al_addresses + AL_KEY_COST * al_keys
    if create:
        cost += TX_CREATE_COST + INIT_CODE_WORD_COST * ((len(data) + 31) // 32)
    return cost


def analyse(oracle, tx, chain_id, base_fee=None, block_gas_limit=None, recover=True, at=0):
    """-> {output name: integer or bytes} for the transaction that lies at offset `at` of the call's blob"""
    tx = bytes(tx)
    o = {name: (bytes(k) if dt == "u1" and k > 1 else 0) for name, dt, k in OUTPUTS}
    o["tx_hash"] = oracle.keccak256(tx)
    st, f, sig = decode(tx, chain_id)
    o["sig_status"] = st
    if f is None:
        o["flags"] = UNDECODABLE
        return o
    flags = 0
    if st == S.OK:
        pre, r, s, recid = sig
        o["sig_hash"] = oracle.keccak256(pre)
        o["sig"] = r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([recid])
        if recover:
            code, q = fast_recover(int.from_bytes(o["sig_hash"], "big"), r, s, recid, S.LOW_S)
            o["sig_status"] = code
            if code == S.OK:
                o["sender"] = S.address(oracle, q)
            else:
                flags |= SIGNATURE
    else:
        flags |= BAD_V
    if not recover:
        o["sig_status"] = 0
    create = len(f["to"]) == 0
    data = tx[f["data"][0]:f["data"][0] + f["data"][1]]
    o.update(type=f["type"], chain_id=f["chain_id"], nonce=f["nonce"], gas_limit=f["gas_limit"], gas_price=f["gas_price"].to_bytes(32, "big"),
             priority_fee=f["priority_fee"].to_bytes(32, "big"), value=f["value"].to_bytes(32, "big"), to=f["to"].rjust(20, b"\0"),
             data_off=at + f["data"][0], data_len=f["data"][1], al_off=at + f["al"][0] if f["type"] else 0, al_len=f["al"][1],
             al_addresses=f["al_addresses"], al_keys=f["al_keys"])
    o["intrinsic_gas"] = intrinsic_gas(data, create, f["al_addresses"], f["al_keys"])
    if f["type"] and f["chain_id"] != chain_id:
        flags |= CHAIN_ID
    if base_fee is not None:  # blockchain.zig:243-258
        if f["type"] == 2 and f["gas_price"] < f["priority_fee"]:
            flags |= PRIORITY_ABOVE_MAX
        if f["gas_price"] < base_fee:
            flags |= FEE_BELOW_BASE
        if not flags & (PRIORITY_ABOVE_MAX | FEE_BELOW_BASE):
            eff = min(f["priority_fee"], f["gas_price"] - base_fee) + base_fee if f["type"] == 2 else f["gas_price"]
            o["effective_gas_price"] = eff.to_bytes(32, "big")
    if block_gas_limit is not None and f["gas_limit"] > block_gas_limit:
        flags |= GAS_ABOVE_BLOCK
    if o["intrinsic_gas"] > f["gas_limit"]:  # blockchain.zig:345-353
        flags |= INTRINSIC_GAS
    if f["nonce"] == (1 << 64) - 1:  # EIP-2681 (the reference's constant (2 << 64) - 1 is beyond every u64)
        flags |= NONCE_MAX
    if create and len(data) > 2 * MAX_CODE_SIZE:
        flags |= INITCODE_SIZE
    cost = f["gas_limit"] * f["gas_price"] + f["value"]  # blockchain.zig:268-274
    if cost > M256:
        flags |= COST_OVERFLOW
    else:
        o["upfront_cost"] = cost.to_bytes(32, "big")
    o["flags"] = flags | (IS_CREATE if create else 0)
    return o


_rows = {}  # what analyse answered for a transaction at offset 0 (test batches repeat their transactions)


def expected(oracle, txs, chain_id, base_fee=None, block_gas_limit=None, recover=True):
    """-> ({output name: bytes of the whole array}, first_bad)"""
    rows, at = [], 0
    for t in txs:
        key = (bytes(t), chain_id, base_fee, block_gas_limit, recover)
        if key not in _rows:
            _rows[key] = analyse(oracle, t, chain_id, base_fee, block_gas_limit, recover, 0)
        row = dict(_rows[key])
        if not row["flags"] & UNDECODABLE:
            row["data_off"] += at
            row["al_off"] += at if row["type"] else 0
        rows.append(row)
        at += len(t)
    out = {}
    for name, dt, k in OUTPUTS:
        if dt == "u1" and k > 1:
            out[name] = b"".join(r[name] for r in rows)
        else:
            out[name] = np.asarray([r[name] for r in rows], dtype="<" + dt).tobytes()
    bad = [i for i, r in enumerate(rows) if r["flags"] & ERROR_BITS]
    return out, (bad[0] if bad else len(rows))


def load_vectors():
    """tests/golden/tx_vectors.json.gz (tests/golden/make_tx_vectors.py): entry k describes transaction k of
    tests/secp_ref.load_vectors()["fixtures"]; "data" as bytes, the integers as integers"""
    import base64
    import gzip
    import json
    import os
    import zlib
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx_vectors.json.gz")) as f:
        doc = json.load(f)
    for t in doc["fixtures"]:
        t["data"] = bytes.fromhex(t["data"]) if "data" in t else zlib.decompress(base64.b64decode(t.pop("data_zlib_b64")))
        for k in ("nonce", "gasPrice", "gasLimit", "value", "v", "r", "s"):
            t[k] = int(t[k] or "0", 16)
        t["to"], t["sender"] = bytes.fromhex(t["to"]), bytes.fromhex(t["sender"].rjust(40, "0"))
    return doc
