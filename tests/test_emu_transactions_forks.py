"""Blob and set-code transactions a second time on the CPU: the test bodies of tests/test_gpu_transactions_forks.py (imported, unchanged)
against libphant_emu.so -- phant_amd/csrc/transactions.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md section 7j states."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_transactions_forks import (  # noqa: E402,F401
    P, pool, tuples, test_batch_sizes_at_every_fork, test_subsets_of_the_new_outputs, test_authorization_totals, test_auth_cap,
    test_block_seams_of_both_sponges, test_authorization_message_seams, test_hostile_bytes, test_rule_boundaries, test_tuple_verdicts,
    test_blob_gas_used, test_refused_arguments, test_the_python_result)


def test_launch_counts(P, oracle, pool):
    """Below PRAGUE, or without a decodable tuple in the call, the launches of phant_block_transactions: 4 with and 3 without the
    recovery, the device form one more.  With tuples (up to 2 047 transactions): the scan of their counts, their rows, their hashes and
    their recovery -- four more, three without the recovery."""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_transactions_forks as G
    from tests import tx_ref_forks as F
    ctx = default_context()
    lib = ctx._lib
    plain = [pool[i] for i in (0, 1, 2, 4)]           # no type 4
    empty = plain + [pool[5], pool[14]]               # a type 4 without a tuple, an undecodable one with four
    some = plain + [pool[3]]

    def launches(txs, n, fork, dev, recover):
        raw = G.RawEx(P, [txs[i % len(txs)] for i in range(n)], dev=dev)
        out = (ctypes.c_ulonglong * 3)()
        lib.hipemu_counters(out)
        before = out[0]
        rc, _, _, na, _ = raw.call_ex(ctx, fork, recover=recover, want=("tx_hash", "flags", "auth_first"), auth_cap=0)
        assert rc == 0 and (na > 0) == (txs is some and fork == F.PRAGUE)
        lib.hipemu_counters(out)
        return out[0] - before

    launches(plain, 1, F.LONDON, False, True)  # (a context's first recovery also computes its table of G's multiples)
    forms = [(dev, rec) for dev in (False, True) for rec in (True, False)]
    for txs, fork in ((plain, F.LONDON), (some, F.LONDON), (some, F.CANCUN), (plain, F.PRAGUE), (empty, F.PRAGUE)):
        assert [launches(txs, n, fork, dev, rec) for n in (3, 70) for dev, rec in forms] == [4, 3, 5, 4] * 2, (txs is some, fork)
    assert [launches(some, n, F.PRAGUE, dev, rec) for n in (5, 70) for dev, rec in forms] == [8, 6, 9, 7] * 2
