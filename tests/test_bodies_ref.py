"""tests/bodies_ref.py, the definition of phant_block_bodies and of its splitter, held against known answers that owe nothing to this
code: the 87 blocks of the reference's fixtures (tests/golden/fixture_roots.json.gz) as ONE segment under each block's own base fee
and gas limit, with the roots their headers state (tests/golden/header_vectors.json.gz), at the fork the fixtures were made for
(Shanghai: the call's LONDON; under PRAGUE's calldata floor some of them would be short of gas).  CPU only."""
import numpy as np
import pytest

from tests import bodies_ref as B
from tests import golden
from tests import headers_ref as H
from tests import tx_ref as T
from tests import tx_ref_forks as F


@pytest.fixture(scope="module")
def segment():
    """-> (fixture blocks, their headers, their raw block encodings), case by case in file order"""
    blocks, headers, raws = [], [], []
    for case, chain in zip(golden.fixtures()["cases"], H.load_vectors()):
        assert len(chain) == len(case["blocks"]) + 1
        for blk, (h, _, _, raw) in zip(case["blocks"], chain[1:]):
            blocks.append(blk), headers.append(h), raws.append(raw)
    assert len(blocks) == 87
    return blocks, headers, raws


def _values(blk, key):
    return [bytes.fromhex(v) for v in blk[key]]


def test_the_fixture_segment_has_its_headers_roots_and_no_error_bit(oracle, segment):
    blocks, headers, _ = segment
    txs = [_values(b, "tx_values") for b in blocks]
    wds = [_values(b, "withdrawal_values") for b in blocks]
    assert sum(map(len, txs)) == 70 and {176, 400} <= {len(w) for w in wds}  # (both lists cross the key order's turn at 0x80)
    exp, first_bad_block, first_bad, n_auth, blob_gas = B.expected(
        oracle, txs, 1, F.LONDON, base_fee=[h["base_fee_per_gas"] for h in headers], gas_limit=[h["gas_limit"] for h in headers], recover=False,
        block_wds=wds, exp_txs_root=[h["transactions_root"] for h in headers], exp_wd_root=[h["withdrawals_root"] for h in headers])
    assert exp["transactions_root"] == b"".join(h["transactions_root"] for h in headers)
    assert exp["withdrawals_root"] == b"".join(h["withdrawals_root"] for h in headers)
    assert exp["transactions_root"] == b"".join(bytes.fromhex(b["transactions_trie"]) for b in blocks)
    flags = np.frombuffer(exp["flags"], "<u4")
    assert not (flags & F.ERROR_BITS).any() and (flags == 0).sum() == 44 and (flags == T.IS_CREATE).sum() == 26
    assert (first_bad_block, first_bad, n_auth, blob_gas) == (87, 70, 0, 0) and not np.frombuffer(exp["block_flags"], "<u4").any()
    assert np.frombuffer(exp["block_first_bad"], "<u4").tolist() == [len(t) for t in txs]
    assert np.frombuffer(exp["tx_block"], "<u4").tolist() == [b for b, t in enumerate(txs) for _ in t]


def test_splitting_the_raw_fixture_blocks_gives_the_fixtures_values(segment):
    blocks, _, raws = segment
    status, txs, wds = B.split_all(raws)
    assert status == [B.SPLIT_OK] * 87
    assert txs == [_values(b, "tx_values") for b in blocks] and wds == [_values(b, "withdrawal_values") for b in blocks]


def test_the_splitters_verdicts():
    from tests import secp_ref as S
    legacy, typed = S.rlp_list([S.rlp_int(1)]), b"\x02" + S.rlp_list([S.rlp_int(2)])
    w = [B.withdrawal(0), B.withdrawal(1)]
    ok = B.make_block([legacy, typed], w)
    assert B.split(ok) == (B.SPLIT_OK, [legacy, typed], w) and B.split(ok + b"\x00")[0] == B.SPLIT_BAD_RLP
    assert B.split(B.make_block([legacy]))[1:] == ([legacy], [])
    body = S.rlp_list([S.rlp_list([S.rlp_bytes(typed)]), b"\xc0"])
    assert B.split(body, bodies_only=True) == (B.SPLIT_OK, [typed], []) and B.split(body)[0] == B.SPLIT_BAD_RLP
    assert B.split(B.make_block([legacy], uncles=S.rlp_list([b"\xc0"])))[0] == B.SPLIT_UNCLES
    assert B.split(S.rlp_list([b"\xc0", S.rlp_list([b"\x80"]), b"\xc0"]))[0] == B.SPLIT_BAD_TX       # the empty string
    assert B.split(S.rlp_list([b"\xc0", S.rlp_list([b"\x81\x80"]), b"\xc0"]))[0] == B.SPLIT_BAD_TX   # a first byte above 0x7f
    assert B.split(S.rlp_list([b"\xc0", S.rlp_list([b"\x81\x05"]), b"\xc0"]))[0] == B.SPLIT_BAD_RLP  # not canonical
    assert B.split(S.rlp_list([b"\xc0", S.rlp_list([b"\x05"]), b"\xc0"])) == (B.SPLIT_OK, [b"\x05"], [])
    assert B.split(S.rlp_list([b"\xc0", b"\xc0", b"\xc0", S.rlp_list([b"\x05"])]))[0] == B.SPLIT_BAD_WITHDRAWAL
    assert B.split(S.rlp_list([b"\xc0", b"\xc0", b"\xc0", b"\xc0", b"\xc0"]))[0] == B.SPLIT_BAD_RLP
    assert B.split(S.rlp_list([b"\xc0", b"\x80", b"\xc0"]))[0] == B.SPLIT_BAD_RLP and B.split(b"")[0] == B.SPLIT_BAD_RLP
