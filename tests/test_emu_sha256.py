"""SHA-256 a second time on the CPU: the test bodies of tests/test_gpu_sha256.py (imported, unchanged) against libphant_emu.so --
phant_amd/csrc/sha256.hip.h compiled for the host over the shim's restatements of v_bitop3_b32 and v_alignbit_b32 (tests/emu.py).  The
refused arguments and the reads at the end of an allocation run here before they ever run on a GPU."""
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


from tests.test_gpu_sha256 import (  # noqa: E402,F401
    P, test_fips_vectors, test_block_edges_at_every_skew, test_batches_of_mixed_lengths, test_refused_offsets_and_pointers)
