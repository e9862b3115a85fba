"""How the four block-level calls cross the bus (phant_amd/csrc/staging.h): the number of host-to-device,
device-to-host and device-to-device hipMemcpyAsync calls, of hipMemsetAsync calls and of hipStreamSynchronize calls that the SECOND call
of a shape makes on one context (the first may grow the arena and allocate the pinned stage), counted by the emulated runtime
(tests/native/shim/hip/hip_runtime.h: hipemu_bus_counters).  Each call in the host form below the 8 MiB pinned stage, in the host form
beyond it and in the device form; the transactions with and without authorization tuples.

The numbers are those of commit 7c5f874, the last one in which each of the four drivers carried its own copy of the protocol: they
were recorded there, with this file, before the drivers were rewritten on top of staging.h, and have not been touched since.  This
module runs against the plain emulated library: the sanitized one poisons the arena's padding, so it never stages."""
import ctypes
import os

import numpy as np
import pytest

from tests import emu


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    if os.environ.get("PHANT_EMU_SANITIZE") == "1":
        pytest.skip("the sanitized library never stages")
    yield from emu.emulated_backend()


from tests.test_gpu_transactions_forks import P, pool  # noqa: E402,F401


def _ctx():
    from phant_amd.context import default_context
    return default_context()


def bus_of_second(call):
    """(H2D, D2H, D2D, memsets, stream synchronisations) of the second of two equal calls"""
    lib = _ctx()._lib
    out = (ctypes.c_ulonglong * 5)()
    call()
    lib.hipemu_bus_counters(out)
    before = tuple(out)
    call()
    lib.hipemu_bus_counters(out)
    return tuple(a - b for a, b in zip(out, before))


def test_receipts(P):
    """a small host-form block is one copy in and one span back; the device form reads its control words twice"""
    from tests import test_gpu_receipts as G
    rng = np.random.default_rng(1)
    small = [G._receipt(rng, logs=[G._log(rng)]) for _ in range(5)]
    # (no root is asked of the large block: its 9 MB trie value would take the emulated hasher minutes, and the trie builder's copies are
    # not this protocol's)
    large = [G._receipt(rng, logs=[G._log(rng, topics=1, data_len=3 * 1024 * 1024 + k) for k in range(3)])]
    txs = [G._bytes(rng, 70) for _ in range(3)]

    def counts(receipts, dev, want, other=()):
        raw = G.Raw(P, receipts, dev=dev, other=other, at=len(other))
        raw.enc_total = sum(len(G.R.encode(r)) for r in receipts)

        def call():
            rc, _, enc_len = raw.call(_ctx(), want=want)
            assert rc == 0 and enc_len == raw.enc_total
        return bus_of_second(call)

    assert sum(v.nbytes for v in P.types.receipt.pack_receipts(G._objs(P, large))[0].values()) > 8 << 20
    no_root = ("logs_bloom", "blooms", "encoded", "encoded_off")
    got = {("small", "host"): counts(small, False, G.Raw.OUTS, [txs]), ("small", "device"): counts(small, True, G.Raw.OUTS, [txs]),
           ("small, no root", "host"): counts(small, False, no_root), ("small, no root", "device"): counts(small, True, no_root),
           ("beyond, no root", "host"): counts(large, False, no_root)}
    print(got)
    assert got == RECEIPTS, got


def test_headers(P):
    """the host form is one copy in, one span back and, where the encodings are wanted, their copy"""
    from tests import test_gpu_headers as G
    rng = np.random.default_rng(2)
    small = G.chain(rng, 6)
    large = [dict(h, extra_data=h["extra_data"] + bytes(2800)) for h in (G.chain(rng, 64) * 47)[:3000]]

    def counts(headers, dev, want):
        raw = G.Raw(P, headers, dev=dev)
        raw.enc_total = sum(len(G.H.encode(h)) for h in headers)

        def call():
            rc, _, _, enc_len = raw.call(_ctx(), want=want)
            assert rc == 0 and enc_len == raw.enc_total
        return bus_of_second(call)

    assert sum(v.nbytes for v in P.types.block.pack_headers(G._objs(P, large)).values()) > 8 << 20
    got = {(size, form, len(want)): counts(headers, form == "device", want)
           for size, headers in (("small", small), ("beyond", large)) for form in ("host", "device")
           for want in (G.Raw.OUTS, ("hashes", "flags")) if not (size == "beyond" and form == "device")}
    print(got)
    assert got == HEADERS, got


def test_transactions(P, oracle, pool):
    """the host form is one copy in and one span back, two plain copies in beyond the stage; with authorization tuples the
    control words are read once more in the middle of the call and the tuples' rows come back by copies of their own"""
    from tests import test_gpu_transactions as G0
    from tests import test_gpu_transactions_forks as G
    from tests import tx_ref_forks as F
    plain = [pool[i] for i in (0, 1, 2, 4)] * 2
    tuples = plain + [pool[3]]
    large = [G0.raw_tx(i % 3, nonce=i, data=G0._data(49152 + (i % 2), i), gas=10**7) for i in range(180)]

    def counts(txs, dev, fork, n_auth):
        raw = G.RawEx(P, txs, dev=dev)

        def call():
            rc, _, _, na, _ = raw.call_ex(_ctx(), fork, recover=False, auth_cap=n_auth)
            assert rc == 0 and na == n_auth
        return bus_of_second(call)

    many = [pool[i] for i in (0, 1)] * 10000
    assert sum(map(len, large)) > 8 << 20 and sum(G.WIDTH[k] for k in G.ALL + G.TX_EX) * len(many) > 8 << 20
    got = {(name, form): counts(txs, form == "device", fork, n_auth)
           for name, txs, fork, n_auth in (("small", plain, F.LONDON, 0), ("small, no tuple at PRAGUE", plain, F.PRAGUE, 0),
                                           ("small, tuples", tuples, F.PRAGUE, 2), ("inputs beyond", large, F.LONDON, 0),
                                           ("outputs beyond", many, F.LONDON, 0))
           for form in ("host", "device") if not ("beyond" in name and form == "device")}
    print(got)
    assert got == TRANSACTIONS, got


def test_txstate(P):
    """the host form is one copy in and one span back.  Beyond the stage: inputs that end beyond 8 MiB while the outputs
    in front of them still come back as one span (90 000 pre-state rows), and both directions array by array (170 000 transactions)"""
    from tests import test_gpu_txstate as G
    from tests import txstate_ref as R
    rng = np.random.default_rng(4)

    def counts(n, na, dev):
        accounts = G.make_accounts(na, rng)
        raw = G.Raw(P, dev, G.make_block(n, accounts, "distinct", rng), accounts, probes=[G.addr(1)], auth_first=[0] * n + [1], auths=[(G.addr(2), 0)])

        def call():
            assert raw.call(_ctx(), R.PRAGUE)[0] == 0
        return bus_of_second(call)

    shapes = [("small", 70, 300, "host"), ("small", 70, 300, "device"), ("general", 300, 300, "host"), ("general", 300, 300, "device"),
              ("inputs beyond", 64, 90000, "host")] + [("both beyond", 170000, 2048, "host")]
    got = {(name, form): counts(n, na, form == "device") for name, n, na, form in shapes}
    print(got)
    assert got == TXSTATE, got


# ---- recorded at commit 7c5f874 (see the module's docstring): (H2D, D2H, D2D, memsets, stream synchronisations)
RECEIPTS = {("small", "host"): (1, 1, 0, 1, 1), ("small", "device"): (1, 2, 4, 1, 2), ("small, no root", "host"): (1, 1, 0, 1, 1),
            ("small, no root", "device"): (1, 2, 2, 1, 2), ("beyond, no root", "host"): (10, 4, 0, 1, 2)}
# (size, form, outputs wanted: all four, or digests and flags alone)
HEADERS = {("small", "host", 4): (1, 2, 0, 1, 2), ("small", "host", 2): (1, 1, 0, 1, 1), ("small", "device", 4): (0, 2, 4, 1, 2),
           ("small", "device", 2): (0, 2, 2, 1, 2), ("beyond", "host", 4): (23, 5, 0, 2, 2), ("beyond", "host", 2): (23, 3, 0, 2, 2)}
TRANSACTIONS = {("small", "host"): (1, 1, 0, 1, 1), ("small", "device"): (0, 2, 26, 1, 2), ("small, no tuple at PRAGUE", "host"): (1, 1, 0, 1, 1),
                ("small, no tuple at PRAGUE", "device"): (0, 3, 26, 1, 3), ("small, tuples", "host"): (1, 7, 0, 1, 2),
                ("small, tuples", "device"): (0, 3, 31, 1, 3), ("inputs beyond", "host"): (2, 1, 0, 1, 1), ("outputs beyond", "host"): (2, 27, 0, 1, 1)}
TXSTATE = {("small", "host"): (1, 1, 0, 1, 1), ("small", "device"): (0, 2, 8, 1, 2), ("general", "host"): (1, 1, 0, 2, 1),
           ("general", "device"): (0, 2, 8, 2, 2), ("inputs beyond", "host"): (16, 1, 0, 2, 1), ("both beyond", "host"): (16, 9, 0, 2, 1)}
