"""The hash kernels' grids a second time on the CPU: the test bodies of tests/test_gpu_verify_grids.py (imported, unchanged)
against libphant_emu.so, the same kernel sources compiled for the host (tests/emu.py) -- which proof rides, which wave comes
back for which depth and which wave strides over which chunk are logic and address arithmetic of the sources."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module", params=["levels0", "levels2", "levels5"])
def M(request):
    import phant_amd
    from tests.test_gpu_verify import _Mode
    ctx = emu.mirror_context(emu.mirror_lib(), request.param)
    if request.param == "levels0":
        ctx.diag_set("verify_no_coop", 1)
    yield _Mode(phant_amd.mpt, ctx, request.param)
    ctx.close()


@pytest.fixture
def ctx4():
    ctx = emu.mirror_context(emu.mirror_lib(), "levels4")
    yield ctx
    ctx.close()


from tests.test_gpu_verify_grids import (  # noqa: E402,F401
    test_wave_edges, test_riding_on_and_off_in_one_batch, test_two_leaf_lengths_in_one_wave,
    test_damage_at_the_riding_node_and_at_its_parent, test_list_queue_longer_than_its_grid, test_multi_root_block_witness)
