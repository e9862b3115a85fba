"""The two strict leaf references of tests/prestate_ref.py against each other, on the CPU alone: decode_account / decode_slot mirror
the decode kernels' order of checks, rlp_decode_strict + account_of_item / slot_of_item are a general canonical RLP decoder written
from the specification with the type rules applied on the decoded tree.  A disagreement on the corpora the GPU tests launch
(tests/test_gpu_prestate_more.py) is seen here, before any device is involved."""
import numpy as np

from tests import prestate_ref as R
from tests.witness_util import _rlp_int, _rlp_list, _rlp_str


def test_the_general_decoder_on_the_specification_s_own_examples():
    d = R.rlp_decode_strict
    assert d(b"\x83dog") == b"dog" and d(bytes.fromhex("c88363617483646f67")) == [b"cat", b"dog"]
    assert d(b"\x80") == b"" and d(b"\xc0") == [] and d(b"\x00") == b"\x00" and d(b"\x0f") == b"\x0f" and d(b"\x82\x04\x00") == b"\x04\x00"
    assert d(bytes.fromhex("c7c0c1c0c3c0c1c0")) == [[], [[]], [[], [[]]]]
    lorem = b"Lorem ipsum dolor sit amet, consectetur adipisicing elit"
    assert d(b"\xb8\x38" + lorem) == lorem
    for n in (55, 56, 255, 256, 1024, 70_000):
        s = bytes(range(256)) * (n // 256 + 1)
        assert d(_rlp_str(s[:n])) == s[:n] and d(_rlp_list([_rlp_str(s[:n]), b"\x01"])) == [s[:n], b"\x01"]
    bad = ["", "8100", "817f", "b800", "b837" + "07" * 55, "b90038" + "07" * 56, "b8", "b838" + "07" * 55, "83646f", "83646f6700",
           "c883636174", "c28363", "f800", "f837" + "01" * 55, "f90038" + "01" * 56, "f838" + "01" * 55, "c0c0", "c181", "bf", "ff",
           "b90100" + "07" * 255, "c3820005"[:6]]
    for h in bad:
        assert d(bytes.fromhex(h)) is None, h
    assert d(bytes.fromhex("8180")) == b"\x80" and d(bytes.fromhex("c3820005")) == [b"\x00\x05"]


def test_the_two_strict_references_agree():
    """Both pairs give the same answer on every body of the account corpus (at the size the GPU run uses and at the emulated one),
    on every value of the slot corpus, and on random canonical encodings; the conditions the GPU test asserts on the corpus hold."""
    for every, least in ((3, 2000), (32, 300)):
        corpus = R.leaf_corpus(np.random.default_rng(41), every)
        assert len(set(b for _, b in corpus)) == len(corpus) >= least and all(b for _, b in corpus)
        for name, body in corpus:
            assert R.decode_account(body) == R.strict_account(body), (name, body.hex())
        fam, ok, bad = R.families(corpus, R.strict_account)
        print(f"account corpus (every {every}. seed mutated): {len(corpus)} bodies, {ok} PRESENT, {bad} BAD_VALUE, lengths "
              f"{min(len(b) for _, b in corpus)} .. {max(len(b) for _, b in corpus)}")
        assert 4 * ok >= len(corpus) and 4 * bad >= len(corpus) and fam == R.LEAF_FAMILIES, fam
    # the width edges decode to their values
    seeds = {n: b for n, b in R.leaf_corpus(np.random.default_rng(41), 64) if n.startswith("seed/")}
    assert len(seeds) == 64
    for i, nonce in enumerate(R.NONCE_EDGES):
        for j, bal in enumerate(R.BALANCE_EDGES):
            got = R.strict_account(seeds[f"seed/n{i}b{j}"])
            assert got is not None and got[:2] == (nonce, bal), (i, j)
    slots = R.slot_corpus(np.random.default_rng(42))
    for name, v in slots:
        assert R.decode_slot(v) == R.strict_slot(v), (name, v.hex())
    fam, ok, bad = R.families(slots, R.strict_slot)
    print(f"slot corpus: {len(slots)} values, {ok} PRESENT, {bad} BAD_VALUE")
    assert fam == R.SLOT_FAMILIES and ok == 128 and bad >= 20
    rng = np.random.default_rng(43)
    for _ in range(2000):
        nonce = int.from_bytes(rng.bytes(int(rng.integers(0, 9))), "big")
        bal = int.from_bytes(rng.bytes(int(rng.integers(0, 33))), "big")
        sr, ch = rng.bytes(32), rng.bytes(32)
        body = _rlp_list([_rlp_int(nonce), _rlp_int(bal), _rlp_str(sr), _rlp_str(ch)])
        assert R.strict_account(body) == R.decode_account(body) == (nonce, bal, sr, ch)
        v = int.from_bytes(rng.bytes(int(rng.integers(1, 33))), "big") or 1
        assert R.strict_slot(_rlp_int(v)) == R.decode_slot(_rlp_int(v)) == v
        junk = rng.bytes(int(rng.integers(1, 120)))
        assert R.strict_account(junk) == R.decode_account(junk) and R.strict_slot(junk) == R.decode_slot(junk)
