"""The pre-state of an execution witness a second time on the CPU: the test bodies of tests/test_gpu_prestate.py (imported, unchanged)
against libphant_emu.so -- the same kernel sources compiled for the host over the lockstep-wavefront shim (tests/emu.py), at the
small sizes tests/suite.py gives emulated runs and on a subset of the golden allocs."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


from tests.test_gpu_prestate import (  # noqa: E402,F401
    test_golden_allocs_are_known_answers, test_block_witness_matches_the_reference, test_config4_scale_witness,
    test_damaged_nodes_and_a_wrong_root, test_leaves_that_are_not_values, test_codes, test_code_hash_forms_agree,
    test_new_payload_prestate_hook)
