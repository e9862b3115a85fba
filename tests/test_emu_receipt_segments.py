"""Receipts of chain segments a second time on the CPU: the test bodies of tests/test_gpu_receipt_segments.py (imported, unchanged) against
libphant_emu.so -- phant_amd/csrc/receipt_segments.hip.h compiled for the host over the lockstep-wavefront shim (tests/emu.py) -- at the
reduced sizes tests/suite.py gives emulated runs, and the launch counts DESIGN.md section 7q states.  The refused-argument cases and the
malformed rows run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_receipt_segments import (  # noqa: E402,F401
    P, test_one_block_equals_block_receipts_from_fields, test_block_boundaries_on_wave_edges_and_empty_blocks, test_many_small_blocks,
    test_logs_topics_and_data_lengths, test_receipt_lengths_on_each_side_of_the_header_turns, test_gas_types_and_a_post_state_root, test_each_flag_alone,
    test_malformed_rows_all_in_one_call, test_subsets_of_the_outputs_unaligned_byte_arrays_and_short_caps, test_a_call_beyond_the_pinned_stage_between_small_ones,
    test_refused_arguments, test_validate_receipts_on_the_fixture_segment)


def test_launch_counts(P):
    """The launches depend on neither n_blocks nor n: the same receipts in 1, 2, 64 and 300 blocks launch the same kernels.  Without a root or
    encodings: decode, one scan (a single tile at this size), the logs' rows, the bloom items, the rows, the verdict -- 6 in the consensus
    form, which always hashes for PHANT_RCPT_BLOOM; 5 in the ETH69 form when nothing needs a bloom; the device form one more (its check).
    With roots: lengths, their scan and the pairs in front of the forest pass -- 3 more, and the ETH69 form's bloom items -- and the forest's
    own launches, which are the trie hasher's: the ones phant_block_roots makes over the same lists.  With encodings the ETH69 form adds
    its gather."""
    import ctypes
    from phant_amd.context import default_context
    from tests import receipts_seg_ref as G
    from tests import test_gpu_receipt_segments as T
    ctx = default_context()
    lib = ctx._lib
    receipts = [T._plain(i, logs=[T._log(i, i % 3, b"xy")] * (i % 2)) for i in range(70)]

    def counter():
        out = (ctypes.c_ulonglong * 3)()
        lib.hipemu_counters(out)
        return out[0]

    def spread(form, n_blocks):
        first = [0] + sorted((k * 70) // n_blocks for k in range(1, n_blocks)) + [70]
        rows = [[(t, ok, 21000 * (i - first[b] + 1), logs) for i, (t, ok, _, logs) in enumerate(receipts) if first[b] <= i < first[b + 1]] for b in range(n_blocks)]
        return T._enc(rows, form)

    def launches(form, n_blocks, dev, want):
        raw = T.RawSegs(P, spread(form, n_blocks), form, dev=dev)
        before = counter()
        rc, _, sc = raw.call(ctx, want=want, encoded_cap=1 << 20)
        assert rc == 0 and sc[0] == n_blocks
        return counter() - before

    plain, rooted, stored = ("flags", "block_flags"), ("flags", "receipts_root"), ("flags", "encoded", "encoded_off")
    lists = spread(G.CONSENSUS, 2)
    before = counter()
    P.mpt.block_roots(lists)
    forest = counter() - before
    for n_blocks in (1, 2, 64, 300):
        assert [launches(G.CONSENSUS, n_blocks, dev, plain) for dev in (False, True)] == [6, 7], n_blocks
        assert [launches(G.ETH69, n_blocks, dev, plain) for dev in (False, True)] == [5, 6], n_blocks
        assert launches(G.CONSENSUS, n_blocks, False, stored) == 6 and launches(G.ETH69, n_blocks, False, stored) == 10, n_blocks
    assert launches(G.CONSENSUS, 2, False, rooted) == 9 + forest and launches(G.ETH69, 2, False, rooted) == 9 + forest
    assert launches(G.CONSENSUS, 2, True, rooted) == 10 + forest
