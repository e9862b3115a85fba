"""radix_sort.hip's scan, pair sort and digest order a second time on the CPU: the test bodies of tests/test_gpu_sort.py (imported,
unchanged) against libphant_emu.so -- the kernel sources compiled for the host over the lockstep-wavefront shim (tests/emu.py) -- at
the reduced sizes tests/suite.py gives emulated runs.  The 524 289-key sorts and the scans of 2 048^2 counters run on the device and
under PHANT_CPU_SUITE=full only.  (tests/test_emu_scan.py reaches the scan through a test-only export instead of the C-ABI.)"""
import pytest

from tests import emu, suite


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_sort import (  # noqa: E402,F401
    ctx, ties, sizes, test_scan_one_level, test_scan_two_levels_every_tail_residue, test_sort_pairs_sizes_bits_and_key_sets,
    test_sort_pairs_random_values_with_repeats, test_sort_pairs_bits_zero_returns_the_input, test_the_references_and_the_flag_model_alone,
    test_order_digests_ties_runs_and_duplicates, test_order_digests_sizes_and_segments, test_refused_arguments_write_nothing,
    test_one_context_small_large_small)

if suite.FULL:
    from tests.test_gpu_sort import (  # noqa: E402,F401
        test_scan_three_levels_every_tail_residue, test_sort_pairs_256_and_257_tiles, test_order_digests_524289)
