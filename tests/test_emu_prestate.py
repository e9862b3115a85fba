"""The pre-state of an execution witness a second time on the CPU: the test bodies of tests/test_gpu_prestate.py and
tests/test_gpu_prestate_more.py (imported, unchanged)
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

from tests import suite  # noqa: E402
from tests import test_gpu_prestate_more as more  # noqa: E402
from tests.test_gpu_prestate_more import (  # noqa: E402,F401
    test_account_leaf_corpus, test_slot_value_corpus, test_code_lengths_sweep, test_duplicate_code_floods,
    test_calls_share_one_context, test_degenerate_documents, test_null_outputs)


# (the two sizes on either side of the switch of the sponge's theta; the other two sizes in the full CPU suite and on the GPU)
@pytest.mark.parametrize("nc", more.CODE_COUNTS if suite.FULL else (2048, 2049))
def test_code_count_switches_sponge_variant(P, oracle, nc):
    more.code_count_case(P, oracle, nc)
