"""The trie hasher's launch-time choices a second time on the CPU: the test bodies of tests/test_gpu_trie_choices.py (imported,
unchanged) against libphant_emu.so -- phant_amd/csrc/trie_build.hip compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the sizes tests/suite.py gives emulated runs: smaller shapes, one setting of every kind, the bin sizes thinned
to the edges 512|513, 1 024|1 025 and 2 048|2 049, three repeats of the small pass's hand-off instead of twenty.  It checks the
sources' logic and that every shape reaches the path it aims at (the statistics assertions); what hipcc made of the kernels, the
helper stream beside the leaves and the fences are the -m gpu module's.  (The two-thread test stays there: the emulator runs one
launch at a time.)"""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_trie_choices import (  # noqa: E402,F401
    P, ctx, test_shape_under_every_setting, test_the_shapes_reach_what_they_aim_at, test_bins_of_exact_size,
    test_full_branch_waves_with_the_root_node_wanted, test_forests_under_forced_slots_and_the_helper_stream,
    test_one_context_small_large_small, test_the_call_after_refused_keys, test_the_call_after_a_refused_device_form_key,
    test_small_pass_hand_off_repeated)
