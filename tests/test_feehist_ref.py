"""tests/feehist_ref.py -- the definition of phant_block_fee_history in Python integers -- against an answer derived by hand, its
division-free threshold test against floor division, and the base-fee rule phant_amd.types.block.fee_history applies to the segment's
last header against generated header chains that tests/headers_ref.py passes.  No GPU is involved."""
import random

import numpy as np
import pytest

from tests import feehist_ref as R
from tests import headers_ref as H

# one block: prices 5, 1, 3 at base fee 0 with gas 10, 20, 70 -> order rows 1, 2, 0; sums 20, 90, 100
KNOWN = {0: 1, 2000: 1, 2001: 1, 2100: 3, 9000: 3, 9100: 5, 10000: 5}


def test_the_known_answer():
    order, rewards, G = R.block_rewards([5, 1, 3], [10, 20, 70], list(KNOWN))
    assert order == [1, 2, 0] and G == 100 and rewards == list(KNOWN.values())
    out, first_bad = R.expected([0, 3], [5, 1, 3], [10, 20, 70], list(KNOWN))
    assert first_bad == 1 and out["order"] == np.asarray([1, 2, 0], "<u4").tobytes() and out["block_flags"] == bytes(4)
    assert [int.from_bytes(out["reward"][32 * k:32 * k + 32], "big") for k in range(len(KNOWN))] == list(KNOWN.values())
    assert [int.from_bytes(out["tip"][32 * k:32 * k + 32], "big") for k in range(3)] == [5, 1, 3]


def test_tips_below_the_base_fee_ties_and_an_empty_block():
    out, first_bad = R.expected([0, 0, 4, 6], [7, 9, 7, 3, 1, 1], [1, 1, 1, 1, 5, 5], [0, 5000, 10000], base_fee=[9, 4, 1])
    assert first_bad == 1 and np.frombuffer(out["block_flags"], "<u4").tolist() == [0, 1, 0]
    assert np.frombuffer(out["order"], "<u4").tolist() == [3, 0, 2, 1, 4, 5]  # (row 3 is below the base fee: tip 0; rows 0 and 2 tie)
    assert [int.from_bytes(out["reward"][32 * k:32 * k + 32], "big") for k in range(9)] == [0, 0, 0, 0, 3, 5, 0, 0, 0]
    assert np.frombuffer(out["block_gas_used"], "<u8").tolist() == [0, 4, 10]


def test_the_division_free_threshold_test_is_floor():
    rng = random.Random(7)
    top = (1 << 96) - 1
    edge = [0, 1, 2, 9999, 10000, 10001, top - 1, top]
    for p in (0, 1, 4999, 5000, 9999, 10000):
        pairs = [(g, s) for g in edge for s in edge] + [(rng.randrange(top + 1), rng.randrange(top + 1)) for _ in range(2000)]
        # ... and sums right at the threshold of a random G
        for _ in range(500):
            g = rng.randrange(top + 1)
            t = g * p // 10000
            pairs += [(g, max(t - 1, 0)), (g, t), (g, min(t + 1, top))]
        for g, s in pairs:
            assert R.reaches(s, g, p) == (s >= g * p // 10000), (g, s, p)
            assert 10000 * (s + 1) < 1 << 128 and g * p < 1 << 128


def test_the_next_base_fee_follows_generated_chains():
    """over chains that the header rules pass without a base-fee flag, the rule fee_history applies to header i is header i + 1's field"""
    pytest.importorskip("torch")  # (phant_amd imports it)
    from phant_amd.types.block import next_base_fee
    from tests.test_gpu_headers import chain
    rng = np.random.default_rng(11)
    seen = set()
    for nf in (16, 17, 21):
        headers = chain(rng, 40, nf)
        _, flags, _ = H.validate_chain(headers)
        assert not any(f & H.BIT["InvalidBaseFee"] for f in flags)
        for p, c in zip(headers, headers[1:]):
            assert next_base_fee(p["base_fee_per_gas"], p["gas_used"], p["gas_limit"]) == c["base_fee_per_gas"]
            assert R.next_base_fee(p["base_fee_per_gas"], p["gas_used"], p["gas_limit"]) == c["base_fee_per_gas"]
            seen.add((p["gas_used"] > p["gas_limit"] // 2) - (p["gas_used"] < p["gas_limit"] // 2))
    assert seen >= {-1, 1}
    assert next_base_fee(100, 15, 30) == 100 and next_base_fee(100, 30, 30) == 112 and next_base_fee(100, 0, 30) == 88 and next_base_fee(1, 16, 30) == 2
    assert R.next_excess_blob_gas(10, 5, 20) == 0 and R.next_excess_blob_gas(100, 50, 20) == 130
