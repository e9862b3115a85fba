"""A block's transactions against the pre-state a second time on the CPU: the test bodies of tests/test_gpu_txstate.py (imported,
unchanged) against libphant_emu.so -- phant_amd/csrc/txstate.hip.h and its kernels compiled for the host over the lockstep-wavefront
shim (tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md section 7k states."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_txstate import (  # noqa: E402,F401
    P, test_sizes_and_sender_arrangements, test_join, test_sums, test_rules, test_random_blocks_at_each_fork, test_subsets_of_the_outputs,
    test_a_call_beyond_the_pinned_stage, test_one_sequence_across_a_chunk_of_aggregates, test_refused_arguments, test_end_to_end_over_the_fixtures)


def test_launch_counts(P):
    """The small path (up to 256 transactions against up to 2 048 pre-state rows) is ONE launch.  The general path: the table, the rows,
    three launches per byte of the sort key (the pre-state's row indices: one byte up to 255 rows, two up to 65 535), the two levels of
    the scan and the rules -- 8 launches with a table of up to 255 rows and 11 beyond.  The device form one more (its arguments' check).
    Within a path neither the number of transactions nor how they spread over the senders changes that; a call without transactions is
    the table and the rows alone."""
    import ctypes
    import numpy as np
    from phant_amd.context import default_context
    from tests import test_gpu_txstate as G
    from tests import txstate_ref as R
    ctx = default_context()
    rng = np.random.default_rng(3)

    def launches(n, na, arrangement, dev, fork=R.PRAGUE):
        accounts = G.make_accounts(na, rng)
        txs = G.make_block(n, accounts, arrangement, rng)
        raw = G.Raw(P, dev, txs, accounts, probes=[G.addr(1)], auth_first=[0] * n + [1], auths=[(G.addr(2), 0)])
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        before = out[0]
        rc, _, _, _ = raw.call(ctx, fork)
        assert rc == 0
        ctx._lib.hipemu_counters(out)
        return out[0] - before

    for arrangement in ("distinct", "one", "interleaved"):
        assert [launches(n, na, arrangement, dev) for n, na in ((1, 200), (70, 300), (256, 2048)) for dev in (False, True)] == [1, 2] * 3, arrangement
        assert [launches(n, 200, arrangement, dev) for n in (257, 400) for dev in (False, True)] == [8, 9] * 2, arrangement
        assert [launches(n, na, arrangement, dev, R.LONDON) for n, na in ((257, 300), (1, 2049), (400, 2049)) for dev in (False, True)] == [11, 12] * 3, arrangement
    assert [launches(0, 200, "one", dev) for dev in (False, True)] == [2, 3]
