"""TEST INFRASTRUCTURE: the definition of phant_block_transactions_ex in Python integers.

Types 0 - 2 are tests/tx_ref.py's.  Types 3 and 4 are not in the reference (its transaction.zig stops at FeeMarketTx); they are
written here from the EIPs, which include/phant_gpu.h restates: EIP-4844 (the blob transaction, its 14 items, the blob term of the
upfront cost, fake_exponential), EIP-7702 (the set-code transaction, its authorization tuples, what an authority signs, 25000 gas a
tuple), EIP-7623 (the calldata floor) and EIP-2 (low s).  It has its own strict decode for both types and defines every output of
phant_txs_ex_out for EVERY byte string offered as a transaction."""
import numpy as np

from tests import secp_ref as S
from tests import tx_ref as T

LONDON, CANCUN, PRAGUE = 0, 1, 2
NO_TO, BLOB_NONE, BLOB_VERSION, BLOB_FEE_BELOW_BASE, AUTH_NONE, FLOOR_GAS = (1 << k for k in range(12, 18))
ERROR_BITS = 0x7FF | 0x7F000
AUTH_CHAIN_ID, AUTH_NONCE_MAX = 8, 9  # auth_status, beside tests/secp_ref.py's OK .. BAD_V
GAS_PER_BLOB, PER_AUTH_BASE_COST, FLOOR_COST_PER_TOKEN, TOKENS_PER_NONZERO = 131072, 25000, 10, 4
M64, M256 = (1 << 64) - 1, (1 << 256) - 1

# the new outputs: (name, numpy dtype, elements per row), in the order of phant_txs_ex_out: a row per transaction (auth_first: n + 1) ...
TX_OUTPUTS = (("max_fee_per_blob_gas", "u1", 32), ("blob_off", "u8", 1), ("blobs", "u4", 1), ("auth_first", "u4", 1), ("floor_gas", "u8", 1))
# ... and a row per authorization tuple
AUTH_OUTPUTS = (("auth_chain_id", "u1", 32), ("auth_address", "u1", 20), ("auth_nonce", "u8", 1), ("auth_hash", "u1", 32), ("auth_sig", "u1", 65),
                ("authority", "u1", 20), ("auth_status", "u1", 1))
_NAMES = {3: ["chain_id", "nonce", "priority_fee", "gas_price", "gas_limit", "to", "value", "data", "al", "blob_fee", "hashes"],
          4: ["chain_id", "nonce", "priority_fee", "gas_price", "gas_limit", "to", "value", "data", "al", "auths"]}
_WIDTH = {"chain_id": 8, "nonce": 8, "priority_fee": 32, "gas_price": 32, "gas_limit": 8, "value": 32, "blob_fee": 32}


# ------------------------------------------------------------------------------------------------------ the strict decode
def _int(tx, it):
    return int.from_bytes(tx[it[2]:it[3]], "big")


def _tuples(tx, it):
    """the authorization list -> [(chain_id, address, nonce, y_parity, r, s)], or None"""
    if not it[0]:
        return None
    entries = S._items(tx, it[2], it[3])
    if entries is None:
        return None
    out = []
    for e in entries:
        parts = S._items(tx, e[2], e[3]) if e[0] else None
        if parts is None or len(parts) != 6:
            return None
        c, a, n, y, r, s = parts
        if not (S._uint(tx, c, 32) and not a[0] and a[3] - a[2] == 20 and S._uint(tx, n, 8) and S._uint(tx, y, 1) and S._uint(tx, r, 32)
                and S._uint(tx, s, 32)):
            return None
        out.append((_int(tx, c), tx[a[2]:a[3]], _int(tx, n), _int(tx, y), _int(tx, r), _int(tx, s)))
    return out


def decode(tx, chain_id, fork):
    """raw transaction -> (status, fields or None, (preimage, r, s, recid)) as tests/tx_ref.decode, whose answer it is for every byte
    string that does not begin with 0x03 or 0x04.  fields of those two also have "blob_fee", "hashes" (span of the list's payload),
    "blobs" (the hashes themselves) and "auths" (the tuples)"""
    tx = bytes(tx)
    if not tx or tx[0] not in (3, 4):
        return T.decode(tx, chain_id)
    bad = (S.BAD_TX, None, None)
    typ = tx[0]
    if typ > 2 + fork:
        return bad
    top = S.rlp_item(tx, 1, len(tx))
    if top is None or not top[0] or top[3] != len(tx):
        return bad
    its = S._items(tx, top[1], top[2])
    names = _NAMES[typ]
    if its is None or len(its) != len(names) + 3:
        return bad
    f = {"type": typ, "blob_fee": 0, "hashes": (0, 0), "blobs": [], "auths": []}
    for name, it in zip(names, its):
        if name in _WIDTH:
            if not S._uint(tx, it, _WIDTH[name]):
                return bad
            f[name] = _int(tx, it)
        elif name == "to":
            if it[0] or it[3] - it[2] not in (0, 20):
                return bad
            f[name] = tx[it[2]:it[3]]
        elif name == "data":
            if it[0]:
                return bad
            f[name] = (it[2], it[3] - it[2])
        elif name == "al":
            if not S._access_list(tx, it):
                return bad
            f[name] = (it[2], it[3] - it[2])
            tuples = S._items(tx, it[2], it[3])
            f["al_addresses"] = len(tuples)
            f["al_keys"] = sum(len(S._items(tx, k[2], k[3])) for t in tuples for k in [S._items(tx, t[2], t[3])[1]])
        elif name == "hashes":
            hs = S._items(tx, it[2], it[3]) if it[0] else None
            if hs is None or any(h[0] or h[3] - h[2] != 32 for h in hs):
                return bad
            f["hashes"], f["blobs"] = (it[2], it[3] - it[2]), [tx[h[2]:h[3]] for h in hs]
        else:
            f["auths"] = _tuples(tx, it)
            if f["auths"] is None:
                return bad
    v_it, r_it, s_it = its[-3:]
    if not (S._uint(tx, v_it, 32) and S._uint(tx, r_it, 32) and S._uint(tx, s_it, 32)):
        return bad
    f["v"] = _int(tx, v_it)
    if f["v"] > 1:
        return S.BAD_V, f, None
    body = tx[top[1]:v_it[1]]
    return S.OK, f, (bytes([typ]) + S._hdr(0xC0, len(body)) + body, _int(tx, r_it), _int(tx, s_it), f["v"])


def authorization_message(chain_id, address, nonce):
    """what an authority signs the Keccak-256 of (EIP-7702: MAGIC = 0x05)"""
    return b"\x05" + S.rlp_list([S.rlp_int(chain_id), S.rlp_bytes(address), S.rlp_int(nonce)])


def floor_gas(data):
    zeros = data.count(0)
    return T.TX_BASE_COST + FLOOR_COST_PER_TOKEN * (zeros + TOKENS_PER_NONZERO * (len(data) - zeros))


def blob_base_fee(excess_blob_gas, fork=PRAGUE):
    """EIP-4844 fake_exponential(MIN_BASE_FEE_PER_BLOB_GAS = 1, excess_blob_gas, BLOB_BASE_FEE_UPDATE_FRACTION); EIP-7691's fraction for
    Prague"""
    denominator = {CANCUN: 3338477, PRAGUE: 5007716}[fork]
    i, output, accum = 1, 0, denominator
    while accum > 0:
        output += accum
        accum = accum * excess_blob_gas // (denominator * i)
        i += 1
    return output // denominator


# ---------------------------------------------------------------------------------------------------------- one transaction
def _zero_row():
    o = {name: (bytes(k) if dt == "u1" and k > 1 else 0) for name, dt, k in T.OUTPUTS + TX_OUTPUTS if name != "auth_first"}
    return o


_tuples_seen = {}  # what analyse_tuple answered (the hostile corpus leaves most tuples as they were)


def analyse_tuple(oracle, t, chain_id, recover=True):
    """one authorization tuple -> {output name: integer or bytes}"""
    key = (t, chain_id, recover)
    if key not in _tuples_seen:
        _tuples_seen[key] = _analyse_tuple(oracle, t, chain_id, recover)
    return _tuples_seen[key]


def _analyse_tuple(oracle, t, chain_id, recover):
    c, a, n, y, r, s = t
    o = {"auth_chain_id": c.to_bytes(32, "big"), "auth_address": a, "auth_nonce": n, "auth_hash": oracle.keccak256(authorization_message(c, a, n)),
         "auth_sig": r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([y]), "authority": bytes(20), "auth_status": 0}
    if not recover:
        return o
    if c not in (0, chain_id):
        o["auth_status"] = AUTH_CHAIN_ID
    elif n == M64:
        o["auth_status"] = AUTH_NONCE_MAX
    elif y > 1:
        o["auth_status"] = S.BAD_V
    else:
        code, q = T.fast_recover(int.from_bytes(o["auth_hash"], "big"), r, s, y, S.LOW_S)
        o["auth_status"] = code
        if code == S.OK:
            o["authority"] = S.address(oracle, q)
    return o


def analyse(oracle, tx, chain_id, fork, base_fee=None, block_gas_limit=None, blob_fee_base=None, recover=True):
    """-> ({output name: integer or bytes} for the transaction at offset 0 of the call's blob, [its authorization tuples' rows])"""
    tx = bytes(tx)
    if not tx or tx[0] not in (3, 4):
        o = _zero_row()
        o.update(T.analyse(oracle, tx, chain_id, base_fee, block_gas_limit, recover, 0))
        if fork >= PRAGUE and not o["flags"] & T.UNDECODABLE:
            o["floor_gas"] = floor_gas(tx[o["data_off"]:o["data_off"] + o["data_len"]])
            if o["gas_limit"] < o["floor_gas"]:
                o["flags"] |= FLOOR_GAS
        return o, []
    o = _zero_row()
    o["tx_hash"] = oracle.keccak256(tx)
    st, f, sig = decode(tx, chain_id, fork)
    o["sig_status"] = st
    if f is None:
        o["flags"] = T.UNDECODABLE
        return o, []
    flags = 0
    if st == S.OK:
        pre, r, s, recid = sig
        o["sig_hash"] = oracle.keccak256(pre)
        o["sig"] = r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([recid])
        if recover:
            code, q = T.fast_recover(int.from_bytes(o["sig_hash"], "big"), r, s, recid, S.LOW_S)
            o["sig_status"] = code
            if code == S.OK:
                o["sender"] = S.address(oracle, q)
            else:
                flags |= T.SIGNATURE
    else:
        flags |= T.BAD_V
    if not recover:
        o["sig_status"] = 0
    typ, create = f["type"], len(f["to"]) == 0
    data = tx[f["data"][0]:f["data"][0] + f["data"][1]]
    blobs, tuples = f["blobs"], f["auths"]
    o.update(type=typ, chain_id=f["chain_id"], nonce=f["nonce"], gas_limit=f["gas_limit"], gas_price=f["gas_price"].to_bytes(32, "big"),
             priority_fee=f["priority_fee"].to_bytes(32, "big"), value=f["value"].to_bytes(32, "big"), to=f["to"].rjust(20, b"\0"),
             data_off=f["data"][0], data_len=f["data"][1], al_off=f["al"][0], al_len=f["al"][1], al_addresses=f["al_addresses"], al_keys=f["al_keys"],
             max_fee_per_blob_gas=f["blob_fee"].to_bytes(32, "big"), blob_off=f["hashes"][0] if typ == 3 else 0, blobs=len(blobs))
    o["intrinsic_gas"] = T.intrinsic_gas(data, create, f["al_addresses"], f["al_keys"]) + PER_AUTH_BASE_COST * len(tuples)
    if f["chain_id"] != chain_id:
        flags |= T.CHAIN_ID
    if base_fee is not None:
        if f["gas_price"] < f["priority_fee"]:
            flags |= T.PRIORITY_ABOVE_MAX
        if f["gas_price"] < base_fee:
            flags |= T.FEE_BELOW_BASE
        if not flags & (T.PRIORITY_ABOVE_MAX | T.FEE_BELOW_BASE):
            o["effective_gas_price"] = (min(f["priority_fee"], f["gas_price"] - base_fee) + base_fee).to_bytes(32, "big")
    if block_gas_limit is not None and f["gas_limit"] > block_gas_limit:
        flags |= T.GAS_ABOVE_BLOCK
    if o["intrinsic_gas"] > f["gas_limit"]:
        flags |= T.INTRINSIC_GAS
    if f["nonce"] == M64:
        flags |= T.NONCE_MAX
    if create and len(data) > 2 * T.MAX_CODE_SIZE:
        flags |= T.INITCODE_SIZE
    cost = f["gas_limit"] * f["gas_price"] + f["value"] + len(blobs) * GAS_PER_BLOB * f["blob_fee"]
    if cost > M256:
        flags |= T.COST_OVERFLOW
    else:
        o["upfront_cost"] = cost.to_bytes(32, "big")
    if create:
        flags |= NO_TO | T.IS_CREATE
    if typ == 3:
        if not blobs:
            flags |= BLOB_NONE
        if any(h[0] != 1 for h in blobs):
            flags |= BLOB_VERSION
        if blob_fee_base is not None and f["blob_fee"] < blob_fee_base:
            flags |= BLOB_FEE_BELOW_BASE
    if typ == 4 and not tuples:
        flags |= AUTH_NONE
    if fork >= PRAGUE:
        o["floor_gas"] = floor_gas(data)
        if f["gas_limit"] < o["floor_gas"]:
            flags |= FLOOR_GAS
    o["flags"] = flags
    return o, [analyse_tuple(oracle, t, chain_id, recover) for t in tuples]


_rows = {}  # what analyse answered (test batches repeat their transactions)


def expected(oracle, txs, chain_id, fork, base_fee=None, block_gas_limit=None, blob_fee_base=None, recover=True):
    """-> ({output name: bytes of the whole array}, first_bad, n_auth, blob_gas_used): the outputs of phant_txs_out, the per-transaction
    ones of phant_txs_ex_out and the per-authorization ones"""
    rows, auths, first, at = [], [], [0], 0
    for t in txs:
        key = (bytes(t), chain_id, fork, base_fee, block_gas_limit, blob_fee_base, recover)
        if key not in _rows:
            _rows[key] = analyse(oracle, t, chain_id, fork, base_fee, block_gas_limit, blob_fee_base, recover)
        row, mine = dict(_rows[key][0]), _rows[key][1]
        if not row["flags"] & T.UNDECODABLE:
            row["data_off"] += at
            row["al_off"] += at if row["type"] else 0
            row["blob_off"] += at if row["type"] == 3 else 0
        rows.append(row)
        auths += mine
        first.append(len(auths))
        at += len(t)
    out = {}
    for group, names in ((rows, [x for x in T.OUTPUTS + TX_OUTPUTS if x[0] != "auth_first"]), (auths, AUTH_OUTPUTS)):
        for name, dt, k in names:
            if dt == "u1" and k > 1:
                out[name] = b"".join(r[name] for r in group)
            else:
                out[name] = np.asarray([r[name] for r in group], dtype="<" + dt).tobytes()
    out["auth_first"] = np.asarray(first, "<u4").tobytes()
    bad = [i for i, r in enumerate(rows) if r["flags"] & ERROR_BITS]
    return out, (bad[0] if bad else len(rows)), len(auths), GAS_PER_BLOB * sum(r["blobs"] for r in rows)


# ------------------------------------------------------------------------------------------------------------ test inputs
def _access_list(entries):
    return S.rlp_list([S.rlp_list([S.rlp_bytes(a), S.rlp_list([S.rlp_bytes(k) for k in keys])]) for a, keys in entries])


def versioned(k, version=1):
    """a versioned hash"""
    return bytes([version]) + bytes([0x30 + k % 200]) * 31


def raw_tuple(chain_id, address, nonce, y_parity, r, s):
    return S.rlp_list([S.rlp_int(chain_id), S.rlp_bytes(address), S.rlp_int(nonce), S.rlp_int(y_parity), S.rlp_int(r), S.rlp_int(s)])


def make_authorization(oracle, d, chain_id, address=b"\x77" * 20, nonce=0, high_s=False, y_parity=None, r=None):
    """an authorization tuple (its RLP) signed by private key d; y_parity / r override what the signature gave"""
    z = int.from_bytes(oracle.keccak256(authorization_message(chain_id, address, nonce)), "big")
    r0, s, recid = S.sign(d, z)
    if high_s:
        r0, s, recid = S.high_s_twin(r0, s, recid)
    return raw_tuple(chain_id, address, nonce, recid if y_parity is None else y_parity, r0 if r is None else r, s)


def fields(typ, chain_id=1, nonce=0, max_fee=10**9, max_priority=2, gas=10**6, to=b"\x11" * 20, value=1, data=b"", al=b"\xc0", blob_fee=5,
           hashes=None, auths=None):
    """the items in front of the signature: hashes = a list of 32-byte strings or the list's whole encoding; auths = a list of encoded
    tuples or the list's whole encoding; al = the access list's whole encoding"""
    items = [S.rlp_int(chain_id), S.rlp_int(nonce), S.rlp_int(max_priority), S.rlp_int(max_fee), S.rlp_int(gas), S.rlp_bytes(to), S.rlp_int(value),
             S.rlp_bytes(data), al]
    if typ == 3:
        hashes = [versioned(0)] if hashes is None else hashes
        items += [S.rlp_int(blob_fee), hashes if isinstance(hashes, bytes) else S.rlp_list([S.rlp_bytes(h) for h in hashes])]
    else:
        assert typ == 4
        auths = [raw_tuple(chain_id, b"\x77" * 20, 0, 0, 1, 1)] if auths is None else auths
        items += [auths if isinstance(auths, bytes) else S.rlp_list(auths)]
    return items


def raw_tx(typ, v=0, r=None, s=None, **kw):
    """an UNSIGNED raw transaction of type 3 or 4 (r, s as given, by default a signature nobody made)"""
    r = int.from_bytes(bytes(range(0x81, 0xA1)), "big") if r is None else r
    s = int.from_bytes(bytes(range(0x21, 0x41)), "big") if s is None else s
    return bytes([typ]) + S.rlp_list(fields(typ, **kw) + [S.rlp_int(v), S.rlp_int(r), S.rlp_int(s)])


def make_tx(oracle, d, typ, chain_id, high_s=False, access_list=(), **kw):
    """a signed raw transaction of private key d: types 0 - 2 are tests/secp_ref.make_tx's, 3 and 4 take the keywords of `fields`"""
    if typ < 3:
        return S.make_tx(oracle, d, typ, chain_id, high_s=high_s, access_list=access_list, **kw)
    items = fields(typ, chain_id=chain_id, al=_access_list(access_list), **kw)
    r, s, recid = S.sign(d, int.from_bytes(oracle.keccak256(bytes([typ]) + S.rlp_list(items)), "big"))
    if high_s:
        r, s, recid = S.high_s_twin(r, s, recid)
    return bytes([typ]) + S.rlp_list(items + [S.rlp_int(recid), S.rlp_int(r), S.rlp_int(s)])
