"""Block headers a second time on the CPU: the test bodies of tests/test_gpu_headers.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/headers.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs.  The refused-argument cases run here before they ever
run on a GPU: a lying offset that got past the check would be a fault there, not a failed assertion."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_headers import (  # noqa: E402,F401
    P, test_fixture_headers_as_one_call_of_84_segments, test_mainnet_genesis, test_valid_chains, test_every_subset_of_outputs,
    test_capacity_one_byte_short, test_every_single_field_mutation_of_header_64, test_integer_boundaries, test_extra_data_lengths,
    test_every_field_count, test_device_form_and_one_context_small_large_small, test_a_call_beyond_the_pinned_stage,
    test_refused_arguments, test_decoded_fixture_headers_hash_to_the_fixtures_values, test_the_decoder_refuses, test_payload_block_hash)


def test_launch_counts():
    """what DESIGN.md section 7h states: a small call is four launches, a large one seven (the tiled scan is three); the device form
    adds its argument check"""
    import numpy as np
    from phant_amd.context import default_context
    from tests import test_gpu_headers as T
    import phant_amd
    lib = default_context()._lib
    rng = np.random.default_rng(5)

    def launches(n, dev):
        raw = T.Raw(phant_amd, T.chain(rng, 2) * (n // 2), dev=dev)
        out = (__import__("ctypes").c_ulonglong * 3)()
        lib.hipemu_counters(out)
        before = out[0]
        rc, _, _, _ = raw.call(default_context(), want=("hashes", "flags"))
        assert rc == 0
        lib.hipemu_counters(out)
        return out[0] - before

    assert (launches(256, False), launches(256, True)) == (4, 5)
    assert (launches(2100, False), launches(2100, True)) == (7, 8)
