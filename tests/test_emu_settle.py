"""A block of plain transfers settled a second time on the CPU: the test bodies of tests/test_gpu_settle.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/settle.hip.h and its kernels compiled for the host over the lockstep-wavefront shim (tests/emu.py) --
at the reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md section 7n states."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_settle import (  # noqa: E402,F401
    P, test_event_counts_around_a_tile, test_a_segment_across_three_tiles, test_no_transactions_and_no_withdrawals,
    test_table_sizes_around_a_key_byte, test_coincidences, test_a_balance_that_an_earlier_credit_covers, test_values_near_the_ends,
    test_gas_limit_at_the_boundary, test_classes, test_random_blocks_at_each_fork, test_subsets_of_the_outputs,
    test_a_call_beyond_the_pinned_stage, test_both_scans_beyond_one_chunk_of_aggregates, test_refused_arguments, test_the_fixtures_through_run_transfer_block, test_a_synthetic_block_end_to_end)


def test_launch_counts(P):
    """classify, three launches per byte of the sort key (the pre-state's row indices 0 .. n_accounts: one byte up to 255 rows, two up
    to 65 535), the two levels of the scan and the finish: 7 launches with a table of up to 255 rows and 10 beyond, the device form one
    more (its rows' check).  Neither the number of transactions nor how senders, recipients and the coinbase coincide changes that; a
    block of withdrawals alone takes the same path; a call without any event is the finish kernel alone."""
    import ctypes
    import numpy as np
    from phant_amd.context import default_context
    from tests import settle_ref as R
    from tests import test_gpu_settle as G
    ctx = default_context()
    rng = np.random.default_rng(3)

    def launches(n, na, arrangement, dev, n_wd=2):
        accounts = G.make_accounts(na, rng)
        ok = G.senders_of(accounts)
        txs = G.make_block(n, accounts, "one" if arrangement == "one" else "distinct", rng)
        if arrangement == "coinbase":  # everybody pays the coinbase, which also sends
            txs = [dict(t, to_row=ok[0]) for t in txs]
        raw = G.Raw(P, dev, 7, txs, accounts, [(ok[0], 5)] * n_wd)
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        before = out[0]
        rc, _, _ = raw.call(ctx, R.PRAGUE, G.BGL, ok[0])
        assert rc == 0
        ctx._lib.hipemu_counters(out)
        return out[0] - before

    for arrangement in ("distinct", "one", "coinbase"):
        assert [launches(n, na, arrangement, dev) for n, na in ((1, 200), (90, 255), (300, 30)) for dev in (False, True)] == [7, 8] * 3, arrangement
        assert [launches(n, na, arrangement, dev) for n, na in ((1, 256), (90, 257), (300, 2049)) for dev in (False, True)] == [10, 11] * 3, arrangement
    assert [launches(0, na, "one", dev) for na in (255, 256) for dev in (False, True)] == [7, 8, 10, 11]
    assert [launches(0, 200, "one", dev, n_wd=0) for dev in (False, True)] == [1, 1]
