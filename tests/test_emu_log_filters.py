"""Log filters over chain segments a second time on the CPU: the test bodies of tests/test_gpu_log_filters.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/filters.hip.h compiled for the host (tests/emu.py) -- and the launch counts DESIGN.md section 7t states.
The refused arguments run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_log_filters import (  # noqa: E402,F401
    P, test_logs_against_filters, test_matches_on_wave_edges_and_filter_boundaries, test_blocks_ranges_and_waves_that_leave_early,
    test_near_misses_positions_and_wildcards, test_set_sizes_around_the_threshold_and_a_set_of_copies,
    test_the_deposit_filter_selects_the_candidates_of_block_requests, test_subsets_of_the_outputs_a_short_cap_and_odd_addresses, test_refused_arguments,
    test_too_many_ballots_is_unsupported, test_filter_logs_on_host_arrays_and_device_tensors)


def test_launch_counts(P):
    """The launches depend on neither n_blocks, n_logs nor n_filters: the same logs in 1, 2, 64 and 300 blocks against 1 and 65 filters
    launch the same kernels -- count, one scan (a single tile at this size), emit: 3 --, the device form one more (its check), and a
    call with a set above the threshold one more (the table)."""
    import ctypes
    from phant_amd.context import default_context
    from tests import filters_ref as F
    from tests import test_gpu_log_filters as T
    ctx = default_context()

    def counter():
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        return out[0]

    logs = [T.log(k) for k in range(70)]

    def launches(n_blocks, nf, dev, large=False, logs=logs):
        first = [0] + sorted((k * len(logs)) // n_blocks for k in range(1, n_blocks)) + [len(logs)]
        rows = T.rows_by_hand([[logs[first[b]:first[b + 1]]] for b in range(n_blocks)])
        filters = [F.Filter([T.addr(k + j) for j in range(T.LINEAR_MAX() + 1 if large and k == 0 else 2)], lo=k % n_blocks) for k in range(nf)]
        before = counter()
        rc, _, nm = T.RawLF({k: rows[k] for k in T.ROWS}, dev=dev).call(ctx, filters)
        assert rc == 0 and nm == F.expected_matches(rows, filters)[1]
        return counter() - before

    for n_blocks in (1, 2, 64, 300):
        for nf in (1, 65):
            assert [launches(n_blocks, nf, dev) for dev in (False, True)] == [3, 4], (n_blocks, nf)
            assert [launches(n_blocks, nf, dev, large=True) for dev in (False, True)] == [4, 5], (n_blocks, nf)
    assert [launches(3, 2, dev, logs=[]) for dev in (False, True)] == [3, 4]
