"""The post-state root of an execution witness a second time on the CPU: the test bodies of tests/test_gpu_poststate.py (imported,
unchanged) against libphant_emu.so -- the same kernel sources compiled for the host over the lockstep-wavefront shim (tests/emu.py),
at the small sizes tests/suite.py gives emulated runs."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


from tests.test_gpu_poststate import (  # noqa: E402,F401
    test_fixture_post_state_roots, test_block_shaped_states, test_twenty_thousand_touched_accounts, test_collapses_and_splits,
    test_witness_without_the_neighbour_proofs, test_hostile_witnesses, test_keep_on_an_absent_account_with_a_slot_write,
    test_arguments_and_null_outputs, test_one_context_small_large_small, test_new_payload_poststate_hook,
    test_one_context_prestate_poststate_advance_interleaved,
    test_embedded_nodes_and_sixty_three_shared_nibbles)
