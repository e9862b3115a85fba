"""Bloom screening of log filters a second time on the CPU: the test bodies of tests/test_gpu_bloom_filters.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/filters.hip.h compiled for the host (tests/emu.py) -- and the launch counts DESIGN.md section 7t states."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_bloom_filters import (  # noqa: E402,F401
    P, test_blooms_against_filters, test_full_and_empty_blooms_and_two_bits_of_three, test_ranges_over_blooms, test_no_false_negatives_against_the_exact_call,
    test_refused_arguments)


def test_launch_counts(P):
    """1, 2, 64 and 300 blooms against 1 and 65 filters: the bits of the entries and the screen, two launches; the device form one more
    (its check)"""
    import ctypes
    from phant_amd.context import default_context
    from tests import filters_ref as F
    from tests import test_gpu_bloom_filters as T
    ctx = default_context()

    def counter():
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        return out[0]

    def launches(n, nf, dev):
        blooms = [T.bloom_of_log(b % 7) for b in range(n)]
        filters = [F.Filter([T.addr(k % 9), T.addr(k + 1)], lo=k % n) for k in range(nf)]
        before = counter()
        rc, got = T.RawBloom(blooms, dev=dev).call(ctx, filters)
        assert rc == 0 and got["may"] == F.expected_may(blooms, filters)[0]
        return counter() - before

    for n in (1, 2, 64, 300):
        for nf in (1, 65):
            assert [launches(n, nf, dev) for dev in (False, True)] == [2, 3], (n, nf)
