"""Fee history over chain segments a second time on the CPU: the test bodies of tests/test_gpu_fee_history.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/fee_history.hip.h compiled for the host (tests/emu.py) -- and the launch counts DESIGN.md section 7u
states.  The refused arguments run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_fee_history import (  # noqa: E402,F401
    P, test_the_known_answer, test_blocks_that_straddle_the_waves_and_the_tiles, test_ties_and_tips_that_differ_in_one_limb, test_rows_below_the_base_fee,
    test_gas_of_zero_and_sums_beyond_64_bits, test_thresholds_that_a_sum_meets_exactly, test_subsets_of_the_outputs_and_odd_addresses, test_refused_arguments,
    test_too_many_rewards_is_unsupported, test_the_cap_on_a_blocks_rows, test_rows_from_the_real_calls_and_packed_by_hand,
    test_reward_percentiles_on_host_arrays_and_device_tensors, test_fee_history_of_a_segment)


def test_launch_counts(P):
    """The launches depend on neither n_blocks, n nor n_percentiles: the same rows in 1, 2, 64 and 300 blocks with 1 and 100 percentiles
    launch the same kernels -- tips, ranks, the scan's tiles and aggregates, the selection: 5 --, the device form one more (its check);
    a segment without a row launches the same."""
    import ctypes
    from phant_amd.context import default_context
    from tests import feehist_ref as R
    from tests import test_gpu_fee_history as T
    ctx = default_context()

    def counter():
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        return out[0]

    rows = [((7 * k) % 13, 21000 + k) for k in range(300)]

    def launches(n_blocks, n_pct, dev, rows=rows):
        first = [0] + sorted((k * len(rows)) // n_blocks for k in range(1, n_blocks)) + [len(rows)]
        a, ints = T.pack([rows[first[b]:first[b + 1]] for b in range(n_blocks)])
        pct = [(97 * k) % 10001 for k in range(n_pct)]
        before = counter()
        rc, got, _ = T.RawFH(a, dev=dev).call(ctx, pct, want=("reward",))
        assert rc == 0 and got["reward"] == R.expected(ints[0], ints[1], ints[2], pct)[0]["reward"]
        return counter() - before

    for n_blocks in (1, 2, 64, 300):
        for n_pct in (1, 100):
            assert [launches(n_blocks, n_pct, dev) for dev in (False, True)] == [5, 6], (n_blocks, n_pct)
    assert [launches(3, 2, dev, rows=[]) for dev in (False, True)] == [5, 6]
