"""tests/headers_ref.py pinned by everything the reference knows about headers: the 171 fixture headers (fields, hash, raw
encoding) of 84 chains, the public mainnet genesis header, and a hand-written table of what every single-field change of one
fixture pair must flag -- so that the restatement the GPU tests compare with is not pinned by itself.  CPU only."""
import pytest

from tests import headers_ref as H
from tests import receipts_ref as R


def _all():
    return [x for chain in H.load_vectors() for x in chain]


def test_vector_counts():
    v = H.load_vectors()
    assert len(v) == 84 and sum(len(c) for c in v) == 171 and sum(len(c) - 1 for c in v) == 87 and max(len(c) for c in v) == 12
    assert all(H.n_fields(h) == 17 for h, _, _, _ in _all())
    assert sorted({h["extra_data"] for h, _, _, _ in _all()}) == [b"", b"\x00"]


def test_hashes_and_encodings_of_every_fixture_header():
    for h, want_hash, raw, block in _all():
        assert H.encode(h) == raw
        assert H.hash(h) == want_hash
        assert H.decode(raw) == h
        assert H.decode_block(block) == raw


def test_the_encoding_sits_at_byte_three_of_genesis_rlp():
    h, _, raw, block = H.load_vectors()[0][0]
    assert block[0] == 0xf9 and block[3:3 + len(raw)] == raw


def test_mainnet_genesis():
    h, want, size = H.mainnet_genesis()
    enc = H.encode(h)
    assert H.n_fields(h) == 15 and len(enc) == size == 535 and H.hash(h) == want
    assert H.decode(enc) == h
    assert h["uncle_hash"] == H.EMPTY_UNCLE_HASH == H.O.keccak256(b"\xc0") and h["transactions_root"] == H.O.keccak256(b"\x80")


def test_every_fixture_chain_validates():
    for chain in H.load_vectors():
        headers = [h for h, _, _, _ in chain]
        hashes, flags, first_bad = H.validate_chain(headers, expected_hashes=[x[1] for x in chain])
        assert hashes == [x[1] for x in chain] and flags == [0] * len(chain) and first_bad == len(chain)
        for p, c in zip(headers, headers[1:]):
            assert H.validate(p, c) == 0


def _flip(b, k=0):
    return b[:k] + bytes([b[k] ^ 1]) + b[k + 1:]


# The first fixture pair: parent gas_limit 10^10 (so the limit may move by less than 9 765 625 and the target is 5 * 10^9), gas_used 0,
# timestamp 0, number 0, base fee 7; child gas_limit 10^10, gas_used 45 846, timestamp 1 000, number 1, base fee 7, extra data 0x00.
G, MD = 10 ** 10, 9765625
CHILD = [  # (field, new value or a function of the old one, the errors it must raise)
    ("parent_hash", _flip, {"InvalidParentHash"}),
    ("uncle_hash", _flip, {"InvalidUnclesHash"}),
    ("fee_recipient", _flip, set()),
    ("state_root", _flip, set()),
    ("transactions_root", _flip, set()),
    ("receipts_root", _flip, set()),
    ("logs_bloom", lambda b: _flip(b, 255), set()),
    ("prev_randao", _flip, set()),
    ("withdrawals_root", _flip, set()),
    ("difficulty", 1, {"InvalidDifficulty"}),
    ("block_number", 2, {"InvalidBlockNumber"}),
    ("block_number", 0, {"InvalidBlockNumber"}),
    ("gas_limit", G + MD, {"GasLimitTooHigh"}),
    ("gas_limit", G + MD - 1, set()),
    ("gas_limit", G - MD, {"GasLimitTooLow"}),
    ("gas_limit", G - MD + 1, set()),
    ("gas_limit", 4999, {"GasLimitTooLow", "GasLimitLessThanMinimum", "GasLimitExceeded"}),
    ("gas_limit", 45845, {"GasLimitTooLow", "GasLimitExceeded"}),
    ("gas_used", G + 1, {"GasLimitExceeded"}),
    ("gas_used", G, set()),
    ("timestamp", 0, {"InvalidTimestamp"}),
    ("timestamp", 1, set()),
    ("extra_data", bytes(33), {"ExtraDataTooLong"}),
    ("extra_data", bytes(32), set()),
    ("nonce", lambda b: _flip(b, 7), {"InvalidNonce"}),
    ("base_fee_per_gas", 8, {"InvalidBaseFee"}),
    ("base_fee_per_gas", 6, {"InvalidBaseFee"}),
]
PARENT = [  # every change of the parent changes its hash, which the child's parent_hash then misses
    ("gas_used", G // 2, {"InvalidParentHash"}),                               # at the target: the fee stays 7
    ("gas_used", G, {"InvalidBaseFee", "InvalidParentHash"}),                 # above: 7 * 5e9 / 5e9 / 8 = 0 -> max(0, 1): 8
    ("base_fee_per_gas", 800, {"InvalidBaseFee", "InvalidParentHash"}),       # below: 800 - 800 / 8 = 700
    ("timestamp", 1000, {"InvalidTimestamp", "InvalidParentHash"}),
    ("block_number", 1, {"InvalidBlockNumber", "InvalidParentHash"}),
    ("gas_limit", 2 * G, {"GasLimitTooLow", "InvalidParentHash"}),            # 10^10 <= 2 * 10^10 - 19 531 250; target 10^10, fee 7
    ("state_root", _flip, {"InvalidParentHash"}),
]


def _mutated(h, field, value):
    out = dict(h)
    out[field] = value(h[field]) if callable(value) else value
    return out


@pytest.mark.parametrize("who,table", [("child", CHILD), ("parent", PARENT)])
def test_single_field_mutations_of_one_pair(who, table):
    chain = H.load_vectors()[0]
    p, c = chain[0][0], chain[1][0]
    assert (p["gas_limit"], p["gas_used"], p["timestamp"], p["block_number"], p["base_fee_per_gas"]) == (G, 0, 0, 0, 7)
    assert (c["gas_limit"], c["gas_used"], c["timestamp"], c["block_number"], c["base_fee_per_gas"], c["extra_data"]) == (G, 45846, 1000, 1, 7, b"\x00")
    assert H.validate(p, c) == 0
    for field, value, errors in table:
        flags = H.validate(_mutated(p, field, value), c) if who == "parent" else H.validate(p, _mutated(c, field, value))
        assert flags == sum(H.BIT[e] for e in errors), (who, field, value if not callable(value) else "flip", flags)
        want_first = min(errors, key=H.ERRORS.index) if errors else None
        assert H.first_error(flags) == want_first


def test_expected_base_fee_by_hand():
    p = dict(gas_limit=30_000_000, gas_used=30_000_000, base_fee_per_gas=1_000_000_000)
    assert H.expected_base_fee(p) == 1_125_000_000                      # a full block: + 12.5 %
    assert H.expected_base_fee(dict(p, gas_used=0)) == 875_000_000      # an empty one: - 12.5 %
    assert H.expected_base_fee(dict(p, gas_used=15_000_000)) == 1_000_000_000
    assert H.expected_base_fee(dict(p, gas_used=15_000_001, base_fee_per_gas=7)) == 8   # the floor of one
    assert H.expected_base_fee(dict(p, gas_limit=1, gas_used=0)) == 1_000_000_000       # t = 0 and nothing used
    assert H.expected_base_fee(dict(p, gas_limit=1, gas_used=1)) is None                # the reference divides by zero


def test_strict_decoding():
    h, _, raw, _ = H.load_vectors()[0][1]
    eighteen = R.rlp_list([R.rlp_str(x) for x in R.rlp_decode(raw)] + [b"\x80"])
    for bad in (raw + b"\x00", raw[:-1], eighteen):
        with pytest.raises((ValueError, IndexError)):
            H.decode(bad)
    long_ts = dict(h, timestamp=1 << 64)  # nine bytes
    with pytest.raises(ValueError):
        H.decode(H.encode(long_ts))
    for k in H.FIELD_COUNTS:
        full = dict(h, blob_gas_used=1, excess_blob_gas=2, parent_beacon_root=bytes(32), request_hash=bytes(range(32)))
        cut = {f: (v if i < k else None) for i, (f, v) in enumerate((f, full[f]) for f in H.FIELDS)}
        assert H.n_fields(cut) == k and H.decode(H.encode(cut)) == cut
