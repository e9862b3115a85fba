"""Range proofs a second time on the CPU: the test bodies of tests/test_gpu_ranges.py (imported, unchanged) against libphant_emu.so --
phant_amd/csrc/range_verify.hip.h and the post-state build it shares compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the reduced sizes tests/suite.py gives emulated runs, plus the launch counts and the bus traffic DESIGN.md section
7p states.  The refused-argument cases run here before they ever run on a GPU: an offset that got past the check would be a fault
there, not a failed assertion."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_ranges import (  # noqa: E402,F401
    P, test_leaves_per_range, test_one_large_range, test_ranges_per_call, test_every_status_mixed_in_one_call_and_isolation, test_status_precedence,
    test_tries_sharing_one_node_set_with_garbage, test_value_lengths, test_value_of_561_bytes, test_embedded_leaves_and_a_root_extension, test_origins,
    test_whole_tries, test_one_context_small_large_small, test_every_output_as_null, test_the_item_list_outgrows_its_room, test_the_leaf_pass_switched_off,
    test_refused_arguments, test_end_to_end_with_the_library_s_own_prover)


def _calls():
    """(ranges, nodes) of very different sizes: one small range; many ranges, a third of them failing; whole tries without a proof; a
    call where everything fails"""
    from tests import test_gpu_ranges as G
    t = G.trie("random", 300, seed=5)
    one = t.served(t.keys[3], 4)
    many, nodes = [], []
    for i in range(20):
        r, nd = t.served(t.keys[10 * i], 1 + i)
        many.append((r[0], r[1], r[2][1:], True) if i % 3 == 2 else r)
        nodes += nd
    whole = [G.trie("random", n, seed=90 + n).served(bytes(32), None, has_proof=False)[0] for n in (1, 2, 17, 200)]
    failing = [(c[1], c[2]) for c in G.one_of_every_status()[1:]]
    return [([one[0]], one[1]), (many, nodes), (whole, []), ([f[0] for f in failing], [x for f in failing for x in f[1]])]


def test_launch_counts(P):
    """a call is 74 launches in the host form -- the node set's hash, the leaf rules, the count, the scan, the emit, the
    link, the two leaf passes, the 64 levels, the roots, the finish -- whatever the number of leaves, of ranges and of failures; the
    device form one more (its offsets' check); without a leaf the leaf rules have no lane: one less.  Two steps depend on sheer size, as
    everywhere in the library: the scan is three launches beyond one tile (2 047 leaves + 2 x ranges), the node set's hash two beyond
    its wave-per-node bound"""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_ranges as G
    ctx = default_context()

    def launches(ranges, nodes, dev):
        raw = G.Raw(P, dev, ranges, nodes)
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        before = out[0]
        rc, _, _ = raw.call(ctx)
        assert rc == 0
        ctx._lib.hipemu_counters(out)
        return out[0] - before

    for ranges, nodes in _calls():
        assert [launches(ranges, nodes, dev) for dev in (False, True)] == [74, 75], len(ranges)
    t = G.trie("random", 30, seed=100)
    r, nd = t.served(bytes([255]) * 32, 0)
    assert [launches([r], nd, dev) for dev in (False, True)] == [73, 74]
    big = G.trie("random", 2100, seed=130, vlen=8)
    assert launches([big.served(bytes(32), None, has_proof=False)[0]], [], False) == 76


def test_the_second_run_is_a_whole_run(P):
    """DESIGN.md 7p, "the item list's room": a call whose list outgrows its room is exactly two calls' launches -- the first run counts
    and every kernel behind the count finds nothing to do, the second has the counted room -- and the same call with the estimate is one"""
    import ctypes
    from phant_amd.context import default_context
    from tests import test_gpu_ranges as G
    ctx = default_context()
    ranges, nodes, items = G.crowded()
    assert items > sum(len(r[2]) for r in ranges) + 64
    exp, counts, _ = G.expected(ranges, nodes)

    def launches(dev):
        raw = G.Raw(P, dev, ranges, nodes)
        out = (ctypes.c_ulonglong * 3)()
        ctx._lib.hipemu_counters(out)
        before = out[0]
        rc, got, tot = raw.call(ctx)
        ctx._lib.hipemu_counters(out)
        assert rc == 0 and tot == counts and all(got[k] == exp[k] and got[k, "guards"] for k in G.ALL)
        return out[0] - before

    assert [launches(dev) for dev in (False, True)] == [74, 75]
    ctx.diag_set("ranges_items_per_range", 0)
    try:
        assert [launches(dev) for dev in (False, True)] == [148, 150]
    finally:
        ctx.diag_set("ranges_items_per_range", -1)
    assert [launches(dev) for dev in (False, True)] == [74, 75]


def test_how_the_call_crosses_the_bus(P):
    """below the pinned stage the host form is ONE upload (every input together), two memsets, ONE copy back that reaches
    over every output, and ONE synchronisation; the device form reads its check's verdict and its control words (two copies back),
    copies the four outputs device to device and synchronises twice, once behind either read.  Counted by the emulated runtime for the
    second of two equal calls, as tests/test_emu_call_staging.py does"""
    import ctypes
    import os
    from phant_amd.context import default_context
    from tests import test_gpu_ranges as G
    if os.environ.get("PHANT_EMU_SANITIZE") == "1":
        pytest.skip("the sanitized library never stages")
    ctx = default_context()

    def bus(ranges, nodes, dev, want=None):
        raw = G.Raw(P, dev, ranges, nodes)
        out = (ctypes.c_ulonglong * 5)()
        counts = []
        for _ in range(2):
            ctx._lib.hipemu_bus_counters(out)
            before = tuple(out)
            assert raw.call(ctx, want)[0] == 0
            ctx._lib.hipemu_bus_counters(out)
            counts.append(tuple(a - b for a, b in zip(out, before)))
        return counts[1]  # (H2D, D2H, D2D, memsets, stream synchronisations)

    for ranges, nodes in _calls():
        assert bus(ranges, nodes, False) == (1, 1, 0, 2, 1), len(ranges)
        assert bus(ranges, nodes, False, want=("status",)) == (1, 1, 0, 2, 1)
        assert bus(ranges, nodes, True) == (0, 2, 4, 2, 2), len(ranges)
        assert bus(ranges, nodes, True, want=("status", "bad_leaf")) == (0, 2, 2, 2, 2)
