"""Per-proof witness generation a second time on the CPU: the test bodies of tests/test_gpu_prove_batch.py (imported, unchanged)
against libphant_emu.so (tests/emu.py), at the small sizes tests/suite.py gives emulated runs; then the emulator's launch log: what
a batch call launches on top of its build is a constant, and a call that does not prove launches what it launched before."""
import ctypes as C

import numpy as np
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_prove_batch import (  # noqa: E402,F401
    M, build_pass, test_oracle_parity, test_forests, test_cross_form, test_through_the_verifier, test_device_form_feeds_the_verifier,
    test_capacity_and_arguments, test_device_capacity_and_arguments, test_one_context_small_large_small, P, test_state_proofs_of_fixture_allocs,
    test_state_proofs_of_a_block_shaped_state, test_state_proofs_arguments)

# reset, locate, size, scan, base, the set's emit; count, scan, place, gather
K_BATCH = 10


def test_a_batch_call_launches_its_build_plus_a_constant(M, oracle):
    from tests.witness_util import random_kv
    lib = emu.mirror_lib()

    def count():
        out = (C.c_ulonglong * 3)()
        lib.hipemu_counters(out)
        return out[0]

    rng = np.random.default_rng(9)
    for n, nq in ((40, 5), (700, 200)):  # the two-launch pass, the general pass
        keys, vals = random_kv(rng, n, 32, 1, 80)
        kv = [M.KeyVal(k, v) for k, v in zip(keys, vals)]
        c0 = count()
        M.mptize(kv)
        c1 = count()
        got = M.prove_batch(kv, keys[:nq])
        c2 = count()
        M.mptize(kv)
        c3 = count()
        assert got.total_nodes > 0
        assert c3 - c2 == c1 - c0
        assert c2 - c1 == (c1 - c0) + K_BATCH
