"""The last-node decoder of the deep tier and the walk's fast exit a second time on the CPU: the test bodies of
tests/test_gpu_verify_last_node.py (imported, unchanged) against libphant_emu.so, the same kernel sources compiled for the host
(tests/emu.py) -- which leaves the decoder accepts and what it records are logic and byte arithmetic of the sources."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module", params=["levels1", "levels2", "levels0"])
def M(request):
    import phant_amd
    from tests.test_gpu_verify import _Mode
    ctx = emu.mirror_context(emu.mirror_lib(), request.param)
    if request.param == "levels0":
        ctx.diag_set("verify_no_coop", 1)
    yield _Mode(phant_amd.mpt, ctx, request.param)
    ctx.close()


from tests.test_gpu_verify_last_node import (  # noqa: E402,F401
    test_wave_sizes, test_leaf_index, test_value_length, test_key_length, test_absence, test_malformed_last_nodes,
    test_mixed_batches, test_stale_records)
