"""phant_exec_witness_advance a second time on the CPU: the test bodies of tests/test_gpu_advance.py (imported, unchanged) against
libphant_emu.so -- the same kernel sources compiled for the host over the lockstep-wavefront shim (tests/emu.py), at the small sizes
tests/suite.py gives emulated runs -- and, by the emulator's launch counter, that the sink costs phant_exec_witness_poststate nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


from tests.test_gpu_advance import (  # noqa: E402,F401
    test_fixture_post_states, test_block_shaped_states, test_collapses_and_splits, test_embedded_nodes_and_sixty_three_shared_nibbles,
    test_three_blocks_under_one_witness, test_a_sibling_for_a_later_removal_needs_keep_old, test_failures_give_no_next_witness,
    test_arguments, test_same_outputs_as_poststate_and_keep_old, test_the_same_call_twice_and_one_context_small_large_small,
    test_nodes_beyond_the_estimate_are_counted_and_the_call_runs_again)

# kernel launches of ONE phant_exec_witness_poststate call on the input below, counted with this test's own code on commit 3b13663
# (the last one without phant_exec_witness_advance): 37 accounts and 49 slots among the keys
POSTSTATE_LAUNCHES_BEFORE = 162


def test_poststate_launches_what_it_did_and_advance_no_more(P, oracle):
    from tests import poststate_ref as Q
    from tests import prestate_ref as R
    from tests.test_gpu_poststate import _block_case
    lib = emu.mirror_lib()
    count = lambda: (lambda out: (lib.hipemu_counters(out), out[0])[1])((C.c_ulonglong * 3)())  # noqa: E731
    rng = np.random.default_rng(31)
    accounts, writes, extra = _block_case(oracle, rng, 150, 8, 9, 30)
    doc, root = Q.witness_doc(oracle, accounts, writes, rng, extra_slots=extra)
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        info = w.info()
        assert (info["n_accounts"], info["n_slots"]) == (37, 49)
        arr = Q.write_arrays(oracle, info, writes)
        w.poststate_arrays(None, root, arr)  # (the arenas sized)
        c0 = count()
        got = w.poststate_arrays(None, root, arr)
        c1 = count()
        adv, nxt = w.advance_arrays(None, root, arr)
        c2 = count()
        assert got["n_failed"] == 0 and nxt is not None and nxt.info()["total_nodes"] > 0
        nxt.close()
        assert c1 - c0 == POSTSTATE_LAUNCHES_BEFORE
        assert c2 - c1 == c1 - c0  # the build of an advance call: the same launches, the nodes leave through copies
    finally:
        w.close()
