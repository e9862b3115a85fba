"""Chain segments of block bodies a second time on the CPU: the test bodies of tests/test_gpu_bodies.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/bodies.hip.h and the kernels it shares with transactions.hip.h compiled for the host over the
lockstep-wavefront shim (tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md
section 7o states.  The refused-argument cases run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_bodies import (  # noqa: E402,F401
    P, pool, tuples, test_one_block_equals_the_ex_call, test_block_boundaries_on_wave_edges_and_empty_blocks,
    test_the_same_bytes_pass_in_one_block_and_fail_in_its_neighbour, test_one_block_of_257_and_segments_without_transactions_or_blocks,
    test_list_lengths_around_the_key_orders_turns, test_many_small_blocks, test_blob_and_set_code_transactions_in_different_blocks,
    test_each_body_flag_alone, test_subsets_of_the_outputs_and_unaligned_byte_arrays, test_a_call_beyond_the_pinned_stage, test_refused_arguments,
    test_the_fixture_segment_and_its_senders)


def test_launch_counts(P, oracle, pool):
    """With no root wanted or expected: the launches of phant_block_transactions_ex plus two (every transaction's block; the blocks'
    verdicts), the device form one more (its check) -- the same whether the transactions lie in 1 block or are spread over 2, 64 or 300.
    With roots: three more (lengths, their scan, the pairs) in front of the forest pass, whose own launches are the trie hasher's."""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_bodies as G
    from tests import tx_ref_forks as F
    ctx = default_context()
    lib = ctx._lib
    plain = [pool[i] for i in (0, 1, 2, 4)]
    some = plain + [pool[3]]  # a type 4 with two tuples

    def spread(txs, n, n_blocks):
        cut = sorted((k * n) // n_blocks for k in range(1, n_blocks))
        first = [0] + cut + [n]
        return [[txs[i % len(txs)] for i in range(first[b], first[b + 1])] for b in range(n_blocks)]

    def launches(txs, n, n_blocks, fork, dev, recover, want=("tx_hash", "flags", "block_flags")):
        raw = G.RawBodies(P, spread(txs, n, n_blocks), dev=dev)
        out = (ctypes.c_ulonglong * 3)()
        lib.hipemu_counters(out)
        before = out[0]
        rc, _, _ = raw.call(ctx, fork, recover=recover, want=want, base_fee=[7] * n_blocks)
        assert rc == 0
        lib.hipemu_counters(out)
        return out[0] - before

    launches(plain, 1, 1, F.LONDON, False, True)  # (a context's first recovery also computes its table of G's multiples)
    forms = [(dev, rec) for dev in (False, True) for rec in (True, False)]
    for n_blocks in (1, 2, 64, 300):
        assert [launches(plain, 70, n_blocks, F.PRAGUE, dev, rec) for dev, rec in forms] == [6, 5, 7, 6], n_blocks
        assert [launches(some, 70, n_blocks, F.PRAGUE, dev, rec) for dev, rec in forms] == [10, 8, 11, 9], n_blocks
    # with a root: lengths, one scan (a single tile at this size), pairs -- and the forest pass, whose launches are the trie hasher's own:
    # the ones phant_block_roots makes over the same lists
    lists = spread(plain, 70, 2)
    base = launches(plain, 70, 2, F.LONDON, False, False)
    with_roots = launches(plain, 70, 2, F.LONDON, False, False, want=("flags", "transactions_root"))
    out = (ctypes.c_ulonglong * 3)()
    lib.hipemu_counters(out)
    before = out[0]
    P.mpt.block_roots(lists)
    lib.hipemu_counters(out)
    assert with_roots - base == 3 + (out[0] - before)
