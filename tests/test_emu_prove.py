"""Witness generation a second time on the CPU: the test bodies of tests/test_gpu_prove.py (imported, unchanged) against
libphant_emu.so -- the same kernel sources compiled for the host over the lockstep-wavefront shim (tests/emu.py), at the small sizes
tests/suite.py gives emulated runs.  The last test here is the emulator's launch log: a call that does not prove launches what it
launched before the prover existed."""
import numpy as np
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_prove import (  # noqa: E402,F401
    M, build_pass, test_oracle_parity, test_forests, test_round_trip_through_the_verifier, test_capacity_and_arguments, test_device_capacity_and_arguments,
    test_one_context_small_large_small, test_may_remove_adds_the_siblings, test_device_form, P,
    test_state_witness_of_every_fixture_alloc, test_state_witness_of_a_block_shaped_state, test_state_witness_arguments,
    test_removals_need_the_flag_and_the_flag_suffices)


def test_a_build_that_does_not_prove_launches_what_it_did(M, oracle):
    """Kernel launches by the emulator's counter: a prove call = its build's launches + the prover's own (reset, locate, size, scan,
    base, first, emit: seven, no sibling pass without flags), so the build inside it -- the very code path of phant_mpt_root -- has
    gained none; and phant_mpt_root itself launches the same number before and after a prove call on the same context."""
    from tests.witness_util import random_kv
    lib = emu.mirror_lib()
    count = lambda: (lambda out: (lib.hipemu_counters(out), out[0])[1])((__import__("ctypes").c_ulonglong * 3)())  # noqa: E731
    rng = np.random.default_rng(9)
    for n in (40, 700):  # the two-launch pass, the general pass
        keys, vals = random_kv(rng, n, 32, 1, 80)
        kv = [M.KeyVal(k, v) for k, v in zip(keys, vals)]
        c0 = count()
        M.mptize(kv)
        c1 = count()
        M.prove_nodeset(kv, keys[:5])
        c2 = count()
        M.mptize(kv)
        c3 = count()
        assert c3 - c2 == c1 - c0
        assert c2 - c1 == (c1 - c0) + 7
