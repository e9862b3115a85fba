"""The node-set verifier's hash paths a second time on the CPU: the test bodies of tests/test_gpu_nodeset_choices.py (imported,
unchanged) against libphant_emu.so -- phant_amd/csrc/mpt_verify_nodeset.hip compiled for the host over the lockstep-wavefront shim
(tests/emu.py) -- at the sizes tests/suite.py gives emulated runs: windows of lengths instead of every length, one blob per kind of
boundary, two of the list-count sets, floods of 300 copies instead of 3 000.  The bodies set nodeset_wave_max and
phant_nodeset_tune themselves and put the emulated default (emu.EMU_NODESET_WAVE_NODES) back afterwards.  It checks the sources' logic
and that every shape reaches the path it aims at (the statistics assertions); what hipcc made of the kernels, their cross-lane
instructions and the atomics between waves that really run at once are the -m gpu module's."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_nodeset_choices import (  # noqa: E402,F401
    P, ctx, test_shape_under_every_setting, test_the_shapes_reach_what_they_aim_at, test_wave_grid_edges, test_overflow_counts,
    test_an_older_launch_never_answers, test_verdict_counters, test_deep_chains_and_key_lengths)


def test_the_knobs_are_back_at_the_emulated_default(ctx, oracle):
    """(runs last) the bodies above restore what tests/emu.py::mirror_context set: a later launch on this context takes the wave per node
    up to emu.EMU_NODESET_WAVE_NODES nodes and the class lists beyond."""
    import numpy as np
    from tests import nodeset_shapes as S, suite
    import phant_amd
    bound = 3500 if suite.FULL else emu.EMU_NODESET_WAVE_NODES
    for n, path in ((3, 1), (bound + 1, 3)):
        rng = np.random.default_rng(n)
        keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
        s = S.single_leaf_set(oracle, keys, [k[:5] for k in keys])
        got = phant_amd.mpt.verify_nodeset(*s.astuple(), ctx=ctx)
        assert (got[0] == S.PRESENT).all() and ctx.nodeset_stats()[0] == path
