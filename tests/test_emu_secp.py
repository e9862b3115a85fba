"""Sender recovery a second time on the CPU: the test bodies of tests/test_gpu_secp.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/secp256k1.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_secp import (  # noqa: E402,F401
    P, genuine, test_field_and_scalar_primitives, test_square_roots, test_point_double_and_add_for_every_pair, test_known_answers,
    test_genuine_signatures_and_their_high_s_twins, test_ladder_corner_cases,
    test_batch_sizes_and_a_wave_with_every_second_lane_failing,
    test_every_output_choice_the_device_form_and_one_context_small_large_small, test_refused_arguments,
    test_fixture_and_mainnet_senders, test_signed_transactions_of_every_type, test_transactions_that_fail)
