"""A block's transactions a second time on the CPU: the test bodies of tests/test_gpu_transactions.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/transactions.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs.  The refused-argument cases run here before they ever run on
a GPU: a lying offset that got past the check would be a fault there, not a failed assertion."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_transactions import (  # noqa: E402,F401
    P, pool, test_batch_sizes_in_both_forms, test_subsets_of_outputs, test_one_context_small_large_small, test_a_call_beyond_the_pinned_stage,
    test_block_seams_of_both_sponges, test_list_header_seams, test_hostile_bytes, test_access_lists, test_rule_boundaries,
    test_fixture_and_mainnet_senders, test_genuine_signatures_and_their_high_s_twins, test_refused_arguments, test_the_python_result)


def test_launch_counts(P, pool):
    """what DESIGN.md section 7i states: decode, hash, recover, rules -- four launches whatever the size; PHANT_TXS_NO_RECOVERY leaves the
    sender path unlaunched (three); the device form adds its check of the offsets"""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_transactions as G
    ctx = default_context()
    lib = ctx._lib

    def launches(n, dev, recover):
        raw = G.Raw(P, [pool[i % 5] for i in range(n)], dev=dev)
        out = (ctypes.c_ulonglong * 3)()
        lib.hipemu_counters(out)
        before = out[0]
        rc, _, fb = raw.call(ctx, recover=recover, want=("tx_hash", "flags"))
        assert rc == 0 and fb == n
        lib.hipemu_counters(out)
        return out[0] - before

    launches(1, False, True)  # (a context's first recovery also computes its table of G's multiples)
    assert [launches(n, dev, rec) for n in (3, 70) for dev in (False, True) for rec in (True, False)] == [4, 3, 5, 4] * 2
