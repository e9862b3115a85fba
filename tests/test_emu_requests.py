"""Execution requests of chain segments a second time on the CPU: the test bodies of tests/test_gpu_requests.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/requests.hip.h and sha256.hip.h compiled for the host (tests/emu.py) -- and the launch counts DESIGN.md
section 7s states.  The refused arguments and the malformed candidates run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_requests import (  # noqa: E402,F401
    P, test_blocks_without_logs_without_deposits_and_with_them, test_logs_that_are_no_candidates_are_ignored, test_malformed_candidates_each_alone_and_all_in_one_call,
    test_deposits_on_wave_edges_and_blocks_on_log_edges, test_many_small_blocks, test_one_block_with_seventy_deposits, test_callers_requests_order_and_the_active_mask,
    test_each_flag_alone_and_an_expected_hash_wrong_in_its_last_byte, test_subsets_of_the_outputs_unaligned_byte_arrays_and_short_caps, test_refused_arguments,
    test_validate_requests_on_a_prague_segment)


def test_launch_counts(P):
    """The launches depend on neither n_blocks nor n_logs: the same logs in 1, 2, 64 and 300 blocks launch the same kernels -- classify, one
    scan (a single tile at this size), gather, the inner hashes, the outer hash and verdict: 5 --, the device form one more (its check); a
    call without a single log launches the same five."""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_requests as T
    ctx = default_context()

    def counter():
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        return out[0]

    logs = [T.dlog(k) if k % 5 == 0 else T.other_log(k) for k in range(70)]

    def launches(n_blocks, dev, logs=logs):
        first = [0] + sorted((k * len(logs)) // n_blocks for k in range(1, n_blocks)) + [len(logs)]
        raw = T.RawReq(T.rows_by_hand([[logs[first[b]:first[b + 1]]] for b in range(n_blocks)]), dev=dev)
        before = counter()
        rc, _, sc = raw.call(ctx, other=[[(1, b"\x01")]] + [[] for _ in range(n_blocks - 1)])
        assert rc == 0 and sc == (sum(1 for k in range(len(logs)) if k % 5 == 0), n_blocks)
        return counter() - before

    for n_blocks in (1, 2, 64, 300):
        assert [launches(n_blocks, dev) for dev in (False, True)] == [5, 6], n_blocks
    assert [launches(3, dev, logs=[]) for dev in (False, True)] == [5, 6]
