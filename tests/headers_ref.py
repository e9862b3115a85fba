"""A plain-Python reference for block headers: what phant_header_chain must answer for ANY chain.  Written from
src/types/block.zig:15-69 (the fields and the fork-aware encoding), src/blockchain/blockchain.zig:100-145 (`validateBlockHeader`,
`checkGasLimit`) and the Yellow Paper's RLP rules, with Python integers -- not from the kernels.  Hashing goes through the oracle's
keccak256.

A header here is a dict of the reference's field names: the hashes, fee_recipient, logs_bloom, extra_data, prev_randao and nonce
are bytes, the rest integers; base_fee_per_gas, withdrawals_root, blob_gas_used / excess_blob_gas, parent_beacon_root and
request_hash are None where the header's fork has no such field."""
import gzip
import json
import os

from oracle import oracle as O
from tests.receipts_ref import rlp_decode, rlp_int, rlp_list, rlp_str

FIELDS = ["parent_hash", "uncle_hash", "fee_recipient", "state_root", "transactions_root", "receipts_root", "logs_bloom", "difficulty",
          "block_number", "gas_limit", "gas_used", "timestamp", "extra_data", "prev_randao", "nonce", "base_fee_per_gas",
          "withdrawals_root", "blob_gas_used", "excess_blob_gas", "parent_beacon_root", "request_hash"]
INTS = {"difficulty": 8, "block_number": 8, "gas_limit": 8, "gas_used": 8, "timestamp": 8, "base_fee_per_gas": 32, "blob_gas_used": 8,
        "excess_blob_gas": 8}  # their widths in bytes
WIDTH = {"parent_hash": 32, "uncle_hash": 32, "fee_recipient": 20, "state_root": 32, "transactions_root": 32, "receipts_root": 32,
         "logs_bloom": 256, "prev_randao": 32, "nonce": 8, "withdrawals_root": 32, "parent_beacon_root": 32, "request_hash": 32}
FIELD_COUNTS = (15, 16, 17, 19, 20, 21)
EMPTY_UNCLE_HASH = bytes([29, 204, 77, 232, 222, 199, 93, 122, 171, 133, 181, 103, 182, 204, 212, 26, 211, 18, 69, 27, 148, 138, 116, 19, 240,
                          161, 66, 253, 64, 212, 147, 71])  # block.zig:13

# bit k = the k-th check of validateBlockHeader, in its order; the names are the reference's errors
ERRORS = ["GasLimitTooHigh", "GasLimitTooLow", "GasLimitLessThanMinimum", "GasLimitExceeded", "InvalidBaseFee", "InvalidTimestamp",
          "InvalidBlockNumber", "ExtraDataTooLong", "InvalidDifficulty", "InvalidNonce", "InvalidUnclesHash", "InvalidParentHash",
          "ExpectedHashMismatch"]
BIT = {name: 1 << k for k, name in enumerate(ERRORS)}


def n_fields(h):
    """block.zig:51-68: which of the later fields are set decides how many items are encoded"""
    if h.get("request_hash") is not None:
        n = 21
    elif h.get("parent_beacon_root") is not None:
        n = 20
    elif h.get("blob_gas_used") is not None:
        n = 19
    elif h.get("withdrawals_root") is not None:
        n = 17
    elif h.get("base_fee_per_gas") is not None:
        n = 16
    else:
        n = 15
    if any(h.get(f) is None for f in FIELDS[:n]):
        raise ValueError("a field in front of the last one is missing")
    return n


def encode(h):
    items = []
    for f in FIELDS[:n_fields(h)]:
        items.append(rlp_int(h[f]) if f in INTS else rlp_str(h[f]))
    return rlp_list(items)


def hash(h):  # noqa: A001
    return O.keccak256(encode(h))


def decode(raw):
    """strict: canonical RLP, one of the six field counts, exact widths, minimal integers that fit their field"""
    items = rlp_decode(raw)
    if not isinstance(items, list) or len(items) not in FIELD_COUNTS or any(isinstance(it, list) for it in items):
        raise ValueError("not a header")
    h = {f: None for f in FIELDS}
    for f, it in zip(FIELDS, items):
        if f in INTS:
            if len(it) > INTS[f] or it[:1] == b"\x00":
                raise ValueError("integer " + f)
            h[f] = int.from_bytes(it, "big")
        else:
            if f in WIDTH and len(it) != WIDTH[f]:
                raise ValueError("width of " + f)
            h[f] = bytes(it)
    return h


def decode_block(raw):
    """the header of a whole block encoding [header, transactions, uncles, (withdrawals)]: its raw bytes"""
    raw = bytes(raw)
    items = rlp_decode(raw)
    if not isinstance(items, list) or len(items) not in (3, 4) or not all(isinstance(it, list) for it in items):
        raise ValueError("not a block")
    at = 1 if raw[0] < 0xf8 else 1 + raw[0] - 0xf7
    end = at + (1 + raw[at] - 0xc0 if raw[at] < 0xf8 else 1 + raw[at] - 0xf7 + int.from_bytes(raw[at + 1:at + 1 + raw[at] - 0xf7], "big"))
    return raw[at:end]


def expected_base_fee(p):
    """blockchain.zig:105-117 -> the integer, or None where the reference would divide by zero"""
    t = p["gas_limit"] // 2
    fee, used = p["base_fee_per_gas"], p["gas_used"]
    if used == t:
        return fee
    if t == 0:
        return None
    if used > t:
        return fee + max(fee * (used - t) // t // 8, 1)
    return fee - fee * (t - used) // t // 8


def validate(p, c, parent_hash=None):
    """bits 0 .. 11 of c against its parent p (parent_hash: hash(p) where the caller has it)"""
    f = 0
    md = p["gas_limit"] // 1024
    if c["gas_limit"] >= p["gas_limit"] + md:
        f |= BIT["GasLimitTooHigh"]
    if c["gas_limit"] <= p["gas_limit"] - md:
        f |= BIT["GasLimitTooLow"]
    if c["gas_limit"] < 5000:
        f |= BIT["GasLimitLessThanMinimum"]
    if c["gas_used"] > c["gas_limit"]:
        f |= BIT["GasLimitExceeded"]
    has, phas = c.get("base_fee_per_gas") is not None, p.get("base_fee_per_gas") is not None
    if has != phas:
        f |= BIT["InvalidBaseFee"]  # (the reference unwraps a null)
    elif has:
        e = expected_base_fee(p)
        if e is None or e != c["base_fee_per_gas"]:  # (a 32-byte field never holds a value beyond 2^256 - 1)
            f |= BIT["InvalidBaseFee"]
    if c["timestamp"] <= p["timestamp"]:
        f |= BIT["InvalidTimestamp"]
    if c["block_number"] != p["block_number"] + 1:
        f |= BIT["InvalidBlockNumber"]
    if len(c["extra_data"]) > 32:
        f |= BIT["ExtraDataTooLong"]
    if c["difficulty"] != 0:
        f |= BIT["InvalidDifficulty"]
    if c["nonce"] != bytes(8):
        f |= BIT["InvalidNonce"]
    if c["uncle_hash"] != EMPTY_UNCLE_HASH:
        f |= BIT["InvalidUnclesHash"]
    if c["parent_hash"] != (hash(p) if parent_hash is None else parent_hash):
        f |= BIT["InvalidParentHash"]
    return f


def validate_chain(headers, seg_first=None, expected_hashes=None):
    """-> (hashes, flags, first_bad) as phant_header_chain answers them"""
    n = len(headers)
    hashes = [hash(h) for h in headers]
    anchors = set(seg_first[:-1]) if seg_first is not None else {0}
    flags = []
    for i, h in enumerate(headers):
        f = 0 if i in anchors else validate(headers[i - 1], h, hashes[i - 1])
        if expected_hashes is not None and bytes(expected_hashes[i]) != hashes[i]:
            f |= BIT["ExpectedHashMismatch"]
        flags.append(f)
    return hashes, flags, next((i for i, f in enumerate(flags) if f), n)


def first_error(flags):
    """the error validateBlockHeader returns: the lowest set bit's, or None"""
    return None if not flags else ERRORS[(flags & -flags).bit_length() - 1]


# ------------------------------------------------------------------------------------------------------------ golden
_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_JSON = {"parentHash": "parent_hash", "uncleHash": "uncle_hash", "coinbase": "fee_recipient", "stateRoot": "state_root",
         "transactionsTrie": "transactions_root", "receiptTrie": "receipts_root", "bloom": "logs_bloom", "difficulty": "difficulty",
         "number": "block_number", "gasLimit": "gas_limit", "gasUsed": "gas_used", "timestamp": "timestamp", "extraData": "extra_data",
         "mixHash": "prev_randao", "nonce": "nonce", "baseFeePerGas": "base_fee_per_gas", "withdrawalsRoot": "withdrawals_root",
         "blobGasUsed": "blob_gas_used", "excessBlobGas": "excess_blob_gas", "parentBeaconBlockRoot": "parent_beacon_root",
         "requestsHash": "request_hash"}


def from_json(j):
    """a header as the fixtures spell it (hex without 0x; a zero bloom as "") -> the dict above"""
    h = {f: None for f in FIELDS}
    for k, f in _JSON.items():
        if k not in j:
            continue
        if f in INTS:
            h[f] = int(j[k] or "0", 16)
        elif f == "logs_bloom":
            h[f] = bytes.fromhex(j[k]) if j[k] else bytes(256)
        else:
            h[f] = bytes.fromhex(j[k])
    return h


_vectors = None


def load_vectors():
    """tests/golden/header_vectors.json.gz -> [chain], a chain = [(header, hash, raw encoding, raw block encoding)]"""
    global _vectors
    if _vectors is None:
        with gzip.open(os.path.join(_G, "header_vectors.json.gz"), "rb") as f:
            doc = json.load(f)
        _vectors = [[(from_json(j), bytes.fromhex(j["hash"]), bytes.fromhex(j["raw"]), bytes.fromhex(j["block"])) for j in c["headers"]]
                    for c in doc["cases"]]
    return _vectors


def mainnet_genesis():
    """tests/golden/header_public_kats.json -> (header, hash, encoded bytes)"""
    with open(os.path.join(_G, "header_public_kats.json")) as f:
        j = json.load(f)["mainnet_genesis"]
    return from_json(j), bytes.fromhex(j["hash"]), j["encoded_bytes"]
