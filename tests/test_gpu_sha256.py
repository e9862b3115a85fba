"""Batched SHA-256 on the device (phant_sha256_batch, phant_sha256_batch_dev, phant_amd.crypto.hasher.sha256 / sha256_batch) against
hashlib.sha256, bit for bit, in the host and the device form.  Every blob ENDS with its allocation (the `_up` trick of
tests/test_gpu_receipt_segments.py), so a lane that reads behind its message leaves the buffer, and every output sits between guards.
tests/test_emu_sha256.py runs the same bodies over the kernel sources compiled for the host.

Not tested: messages of 2^29 bytes and more, where the bit count no longer fits 32 bits -- the 64-bit count is written as
(total >> 29, total << 3) in sha256.hip.h and no test here allocates half a gigabyte to reach its upper word."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1
LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 192, 193, 1 + 192 * 5)
GUARD = 64


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx():
    from phant_amd.context import default_context
    return default_context()


def _bytes(n, seed=0):
    return np.random.default_rng(7000 + 31 * n + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Raw:
    """one call of the raw C-ABI over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, dev):
        import torch
        self.dev, self.torch = dev, torch

    def _up(self, a, skew=0):
        """-> (what keeps the memory alive, its address): the array `skew` bytes into an allocation that ENDS with it"""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.concatenate([np.zeros(skew, np.uint8), raw])
        if not len(buf):
            buf = np.zeros(1, np.uint8)
        if not self.dev:
            return buf, buf.ctypes.data + skew
        t = self.torch.from_numpy(buf).cuda()
        return t, t.data_ptr() + skew

    def call(self, messages, skew=0, off=None, out_skew=0):
        """-> (rc, the n x 32 bytes written, whether the guards around them stand)"""
        ctx = _ctx()
        n = len(messages)
        if off is None:
            off = np.zeros(n + 1, np.uint64)
            np.cumsum([len(m) for m in messages], out=off[1:])
        keep_b, p_blob = self._up(np.frombuffer(b"".join(messages), np.uint8), skew)
        keep_o, p_off = self._up(np.asarray(off, np.uint64))
        size = GUARD + 32 * n + GUARD
        out = self.torch.full((size,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(size, 0xEE, np.uint8)
        p_out = (out.data_ptr() if self.dev else out.ctypes.data) + GUARD + out_skew
        fn = ctx._lib.phant_sha256_batch_dev if self.dev else ctx._lib.phant_sha256_batch
        rc = fn(ctx.handle, p_blob, p_off, n, p_out)
        if self.dev:
            self.torch.cuda.synchronize()
            out = out.cpu().numpy()
        at = GUARD + out_skew
        del keep_b, keep_o
        return rc, out[at:at + 32 * n].tobytes(), bool((out[:at] == 0xEE).all() and (out[at + 32 * n:] == 0xEE).all())


def _want(messages):
    return b"".join(hashlib.sha256(m).digest() for m in messages)


def test_fips_vectors(P):
    H = P.crypto.hasher
    assert H.sha256(b"").hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert H.sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert H.sha256(b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq").hex() == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"
    assert H.sha256_batch([]).shape == (0, 32)
    assert H.sha256_batch([b"abc", b"", b"abc"]).tobytes() == _want([b"abc", b"", b"abc"])


@pytest.mark.parametrize("dev", (False, True))
def test_block_edges_at_every_skew(P, dev):
    """lengths on each side of the 55 / 56 turn (one block or two for the padding) and of every block edge, the 193 bytes of a deposit
    request and a type-0 message of five deposits; the blob 0 .. 3 bytes off its allocation's alignment and flush with its end"""
    raw = Raw(dev)
    for n in LENGTHS:
        for skew in range(4):
            m = [_bytes(n, skew)]
            rc, got, guards = raw.call(m, skew=skew)
            assert rc == OK and guards and got == _want(m), (n, skew)


@pytest.mark.parametrize("dev", (False, True))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 256, 257))
def test_batches_of_mixed_lengths(P, dev, n):
    """wave and workgroup edges: lanes of one wave run different numbers of blocks; the last message ends the allocation"""
    messages = [_bytes(LENGTHS[(5 * i + n) % len(LENGTHS)] + i % 3, i) for i in range(n)]
    rc, got, guards = Raw(dev).call(messages, skew=n % 4)
    assert rc == OK and guards
    want = _want(messages)
    assert got == want, next(i for i in range(n) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32])


def test_refused_offsets_and_pointers(P):
    """the host form refuses offsets that go backwards, as phant_keccak256_batch does, and writes nothing; n == 0 is PHANT_OK whatever the
    pointers; the device form refuses an output that is not 16-byte aligned"""
    ctx = _ctx()
    lib = ctx._lib
    messages = [_bytes(10), _bytes(20), _bytes(30)]
    for off in ([0, 10, 9, 60], [0, 30, 30, 29], [5, 4, 30, 60]):
        rc, got, guards = Raw(False).call(messages, off=off)
        assert rc == E_INVALID_ARG and guards and set(got) == {0xEE}, off
    rc, got, guards = Raw(False).call(messages, off=[3, 10, 30, 57])  # (a base offset is legal)
    assert rc == OK and guards and got == _want([b"".join(messages)[a:b] for a, b in ((3, 10), (10, 30), (30, 57))])
    blob, off, out = np.zeros(4, np.uint8), np.zeros(2, np.uint64), np.full(32, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn in (lib.phant_sha256_batch, lib.phant_sha256_batch_dev):
        assert fn(ctx.handle, None, None, 0, None) == OK
        assert fn(None, p(blob), p(off), 1, p(out)) == E_INVALID_ARG
        assert fn(ctx.handle, p(blob), None, 1, p(out)) == E_INVALID_ARG
        assert fn(ctx.handle, p(blob), p(off), 1, None) == E_INVALID_ARG
    off[1] = 4
    assert lib.phant_sha256_batch(ctx.handle, None, p(off), 1, p(out)) == E_INVALID_ARG
    assert set(out.tolist()) == {0xEE}
    rc, got, guards = Raw(True).call(messages, out_skew=8)
    assert rc == E_INVALID_ARG and guards and set(got) == {0xEE}
