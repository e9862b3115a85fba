"""tests/receipts_ref.py pinned against everything on record that is NOT itself: the receipts tests/golden.py derives from the
fixtures' headers (byte for byte), the oracle's logs bloom, go-ethereum's published bloom vector, and its own decoder.

No public known answer for a receipt WITH logs is available to this suite: the reference's fixtures carry only blocks whose
bloom is zero, and tests/golden/public_kats.json holds a bloom, not a receipt.  For receipts with logs the reference encoder is
pinned by construction (RLP's rules over the reference's field order), by decode(encode(x)) == x, and by the two pieces above."""
import numpy as np

from tests import golden
from tests import receipts_ref as R


def _random_receipt(rng, max_logs=4):
    logs = []
    for _ in range(int(rng.integers(0, max_logs + 1))):
        dlen = int(rng.choice([0, 1, 1, 2, 31, 32, 55, 56, 57, 255, 256, 300]))
        data = rng.integers(0, 256, dlen, dtype=np.uint8).tobytes()
        logs.append((rng.integers(0, 256, 20, dtype=np.uint8).tobytes(),
                     [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(int(rng.integers(0, 6)))], data))
    gas = int(rng.choice([0, 1, 0x7f, 0x80, 21000, 1 << 32, (1 << 64) - 1]))
    return (int(rng.choice([0, 1, 2, 3, 0x7f])), bool(rng.integers(0, 2)), gas, logs)


def test_encodings_equal_the_fixture_receipts_of_golden():
    seen = 0
    for c in golden.fixtures()["cases"]:
        for b in c["blocks"]:
            cand = golden.one_transaction_receipts(b)
            if cand is None:
                continue
            tx = bytes.fromhex(b["tx_values"][0])
            tx_type = tx[0] if tx[0] < 0x80 else 0
            assert [R.encode((tx_type, ok, b["gas_used"], [])) for ok in (True, False)] == cand
            seen += 1
    assert seen == 66
    for prefix, status, gas in ((b"", b"\x01", 21000), (b"\x02", b"\x80", 0x1234567), (b"\x01", b"\x01", 1), (b"\x7f", b"\x80", 0x80)):
        want = golden._receipt(prefix, status, gas)
        assert R.encode((prefix[0] if prefix else 0, status == b"\x01", gas, [])) == want
        assert R.decode(want) == (prefix[0] if prefix else 0, status == b"\x01", gas, [])


def test_bloom_equals_the_oracle_and_the_public_vector(oracle):
    rng = np.random.default_rng(5)
    receipts = [_random_receipt(rng, 6) for _ in range(40)]
    want = oracle.logs_bloom([[x for a, ts, _ in r[3] for x in (a, *ts)] for r in receipts])
    assert [R.bloom_of(r[3]) for r in receipts] == [w.tobytes() for w in want]
    assert R.block_bloom(receipts) == np.bitwise_or.reduce(want, axis=0).tobytes()
    assert R.bloom_of([]) == bytes(256) and R.block_bloom([]) == bytes(256)
    # data does not enter the bloom
    a, ts, _ = receipts[0][3][0] if receipts[0][3] else (b"\x11" * 20, [], b"")
    assert R.bloom_of([(a, ts, b"x" * 40)]) == R.bloom_of([(a, ts, b"")])
    # go-ethereum's TestBloomExtensively (tests/golden/public_kats.json): 100 items of one receipt
    k = golden.public_kats()["bloom_extensively"]
    bloom = R.bloom_of([((k["item_format"] % i).encode(), [], b"") for i in range(k["count"])])
    assert oracle.keccak256(bloom).hex() == k["keccak256_of_bloom"]


def test_decode_inverts_encode_and_rlp_boundaries():
    rng = np.random.default_rng(6)
    for _ in range(200):
        r = _random_receipt(rng)
        assert R.decode(R.encode(r)) == r
    # RLP's length rules at their boundaries
    assert R.rlp_str(b"") == b"\x80" and R.rlp_str(b"\x7f") == b"\x7f" and R.rlp_str(b"\x80") == b"\x81\x80"
    assert R.rlp_str(bytes(55))[:1] == b"\xb7" and R.rlp_str(bytes(56))[:2] == b"\xb8\x38"
    assert R.rlp_str(bytes(256))[:3] == b"\xb9\x01\x00" and R.rlp_str(bytes(65536))[:4] == b"\xba\x01\x00\x00"
    assert R.rlp_list([]) == b"\xc0" and R.rlp_list([bytes(55)])[:1] == b"\xf7" and R.rlp_list([bytes(56)])[:2] == b"\xf8\x38"
    assert R.rlp_int(0) == b"\x80" and R.rlp_int(0x80) == b"\x81\x80" and R.rlp_int(1 << 64) == b"\x89\x01" + bytes(8)
    for v in (b"", b"\x00", b"\x7f", b"\x80", bytes(55), bytes(56), bytes(70000)):
        assert R.rlp_decode(R.rlp_str(v)) == v
    # a log of 600 bytes of data and nine topics, typed
    big = (3, True, 1 << 63, [(b"\xaa" * 20, [bytes([i]) * 32 for i in range(9)], bytes(range(256)) * 2 + b"\x01" * 88)])
    assert R.decode(R.encode(big)) == big
