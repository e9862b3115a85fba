"""A block's access lists a second time on the CPU: the test bodies of tests/test_gpu_access_lists.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/access_lists.hip.h and its kernels compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md section 7m states.  The
refused-argument cases run here before they ever run on a GPU: a lying span that got past the check would be a fault there, not a
failed assertion."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_access_lists import (  # noqa: E402,F401
    P, test_counts_and_empties, test_rlp_header_boundaries_of_a_tuple, test_work_distribution, test_malformed_spans, test_joins, test_duplicates,
    test_every_subset_of_outputs, test_capacities_one_short, test_one_context_small_large_small, test_refused_arguments,
    test_end_to_end_from_raw_transactions)


def test_launch_counts(P):
    """A call is 11 launches while its two scans fit a tile each (up to 1 023 transactions): the walk, the scan, the tuples' records, the
    keys' check, the verdicts, the scan, the address table, the slots' and the tuples' tables, the tuples, the keys' table, the keys.
    The device form one more (its arguments' check).  Neither the number of tuples and keys nor how they spread over the transactions
    changes that; without a witness the address table is left out"""
    import ctypes
    from phant_amd.context import default_context
    from tests import access_ref as R
    from tests import test_gpu_access_lists as G
    ctx = default_context()

    def launches(spans, dev, **tables):
        _, totals = R.expected(spans, **tables)
        raw = G.Raw(P, dev, spans, **tables)
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        before = out[0]
        rc, _, _ = raw.call(ctx, (totals["n_tuples"], totals["n_keys"]))
        assert rc == 0
        ctx._lib.hipemu_counters(out)
        return out[0] - before

    w = G.pool()
    for spans in ([R.encode(G.entries(2, 3, seed=i)) for i in range(20)], [R.encode(G.entries(90, 1, seed=1))], [b"", R.encode(G.entries(1, 300, seed=2))]):
        assert [launches(spans, dev, **w) for dev in (False, True)] == [11, 12]
        assert [launches(spans, dev) for dev in (False, True)] == [10, 11]


def test_how_the_call_crosses_the_bus(P):
    """below the pinned stage the host form is ONE upload (the spans' bytes, their offsets and the tables together), two
    memsets, ONE copy back that reaches over every output, and ONE synchronisation; the device form reads its check's verdict and its
    control words (two copies back), copies the eleven outputs device to device and synchronises three times.  Counted by the emulated
    runtime for the second of two equal calls, as tests/test_emu_call_staging.py does"""
    import ctypes
    import os
    from phant_amd.context import default_context
    from tests import access_ref as R
    from tests import test_gpu_access_lists as G
    if os.environ.get("PHANT_EMU_SANITIZE") == "1":
        pytest.skip("the sanitized library never stages")
    ctx = default_context()
    w = G.pool()
    spans = [R.encode(G.entries(2, 3, seed=i)) if i % 5 else b"" for i in range(40)]
    _, totals = R.expected(spans, **w)

    def bus(dev, caps):
        raw = G.Raw(P, dev, spans, **w)
        out = (ctypes.c_ulonglong * 5)()
        counts = []
        for _ in range(2):
            ctx._lib.hipemu_bus_counters(out)
            before = tuple(out)
            assert raw.call(ctx, caps)[0] == 0
            ctx._lib.hipemu_bus_counters(out)
            counts.append(tuple(a - b for a, b in zip(out, before)))
        return counts[1]  # (H2D, D2H, D2D, memsets, stream synchronisations)

    exact = (totals["n_tuples"], totals["n_keys"])
    assert bus(False, exact) == (1, 1, 0, 2, 1)
    assert bus(False, (exact[0] - 1, exact[1])) == (1, 1, 0, 2, 1)  # (a capacity one short: the same traffic, nothing handed out)
    assert bus(True, exact) == (0, 2, 11, 3, 3)
    assert bus(True, (exact[0], exact[1] - 1)) == (0, 2, 4, 3, 2)
