"""A block's receipts a second time on the CPU: the test bodies of tests/test_gpu_receipts.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/receipts.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs.  The refused-argument cases run here before they ever
run on a GPU: a lying offset that got past the check would be a fault there, not a failed assertion."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_receipts import (  # noqa: E402,F401
    P, test_receipt_counts, test_rlp_boundaries, test_receipts_without_logs_between_receipts_with_logs,
    test_one_receipt_with_many_logs, test_a_block_without_any_log, test_a_large_payload_at_an_odd_offset, test_a_block_beyond_the_pinned_stage,
    test_fixture_receipt_tries, test_riding_lists, test_every_subset_of_outputs, test_capacity_one_byte_short,
    test_device_form_and_one_context_small_large_small, test_refused_arguments)
