"""Chain segments of block bodies on the device (phant_block_bodies, phant_block_bodies_dev, phant_amd.types.block.block_bodies /
validate_segment) against tests/bodies_ref.py, which defines every output from tests/tx_ref_forks.py and the oracle's index-keyed
roots, and against phant_block_transactions_ex for one block.  Every comparison is exact, in both forms.
tests/test_emu_bodies.py runs the same bodies over the kernel sources compiled for the host."""
import ctypes as C

import numpy as np
import pytest

from tests import bodies_ref as B
from tests import secp_ref as S
from tests import suite
from tests import tx_ref as T
from tests import tx_ref_forks as F
from tests.test_gpu_transactions import ALL, D, NO_SENDER, OK, E_INVALID_ARG, E_UNSUPPORTED, _ctx, _data, _first_difference
from tests.test_gpu_transactions import raw_tx as raw_tx_012
from tests.test_gpu_transactions_forks import AUTH, AUTH_NO_RECOVERY, TX_EX, RawEx, _auth, pool, tuples  # noqa: F401

pytestmark = pytest.mark.gpu
BLOCK = B.BLOCK_NAMES
WIDTH = B.WIDTH
SCALARS_UNTOUCHED = (0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE)


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _rows32(values):
    return np.frombuffer(b"".join(v if isinstance(v, bytes) else int(v).to_bytes(32, "big") for v in values) or bytes(32), np.uint8).copy()


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class RawBodies:
    """phant_bodies_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""

    def __init__(self, P, block_txs, block_wds=None, dev=False):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        a = P.types.block.pack_bodies(block_txs, block_wds)
        self.nb, self.n, self.n_wd = len(block_txs), len(a["tx_off"]) - 1, (len(a["wd_off"]) - 1 if block_wds is not None else 0)
        self.tx_bytes, self.wd_bytes = int(a["tx_off"][-1]), (int(a["wd_off"][-1]) if block_wds is not None else 0)
        self.host = a

    def _up(self, a, skew=0):
        """-> (something that keeps the memory alive, its address): the array as it is, or `skew` bytes into a longer one"""
        if a is None:
            return None, None
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = np.concatenate([np.zeros(skew, np.uint8), raw, np.zeros(8, np.uint8)])
        if not self.dev:
            return buf, buf.ctypes.data + skew
        t = self.torch.from_numpy(buf).cuda()
        return t, t.data_ptr() + skew

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def _ptr(self, x):
        return x.data_ptr() if self.dev else x.ctypes.data

    def call(self, ctx, fork, chain_id=1, base_fee=None, gas_limit=None, blob_base_fee=None, exp_txs_root=None, exp_wd_root=None, exp_blob_gas=None,
             recover=True, want=None, auth_cap=None, guard=64, flags=None, sizes=None, reserved=0, skew=None, in_skew=0, over=None):
        """-> (rc, {output: bytes}, (first_bad_block, first_bad, n_auth, blob_gas_used)); every buffer has `guard` bytes of 0xEE in front of and
        behind its rows.  The per-block inputs are lists with a value per block.  over: {field of phant_bodies_in: value} put in last (an
        array value is uploaded); in_skew: bytes every byte array of the inputs is moved up by"""
        L, nb, n = self.L, self.nb, self.n
        has_wd = self.host["wd_first"] is not None
        if want is None:
            want = (ALL if recover else NO_SENDER) + TX_EX + (AUTH if recover else AUTH_NO_RECOVERY) + tuple(k for k in BLOCK if has_wd or k != "withdrawals_root")
        if flags is None:
            flags = (L.TXS_HAVE_GAS_LIMIT if gas_limit is not None else 0) | (0 if recover else L.TXS_NO_RECOVERY)
        ins = dict(self.host)
        ins.update(base_fee=None if base_fee is None else _rows32(base_fee), blob_base_fee=None if blob_base_fee is None else _rows32(blob_base_fee),
                   gas_limit=None if gas_limit is None else np.asarray(gas_limit, np.uint64),
                   transactions_root=None if exp_txs_root is None else _rows32(exp_txs_root), withdrawals_root=None if exp_wd_root is None else _rows32(exp_wd_root),
                   blob_gas_used=None if exp_blob_gas is None else np.asarray(exp_blob_gas, np.uint64))
        counts = dict(n=n, n_wd=self.n_wd, n_blocks=nb, tx_bytes=self.tx_bytes, wd_bytes=self.wd_bytes)
        for k, v in (over or {}).items():
            if k in counts:
                counts[k] = v
            else:
                ins[k] = v
        keep, ptr = {}, {}
        for k in L.BODIES_INPUTS:
            byte_array = ins[k] is not None and np.asarray(ins[k]).dtype == np.uint8
            keep[k], ptr[k] = self._up(ins[k], in_skew if byte_array else 0)
        for count, names in (("n", ("txs", "tx_off")), ("n_wd", ("withdrawals", "wd_off"))):  # (never-empty stand-ins: a zero count passes NULL)
            for k in names:
                if not counts[count] and k not in (over or {}):
                    ptr[k] = None
        arg = L.PhantBodiesIn(C.sizeof(L.PhantBodiesIn), fork, flags, counts["n_blocks"], counts["n"], counts["n_wd"], auth_cap or 0, reserved, chain_id,
                              ptr["txs"], ptr["tx_off"], counts["tx_bytes"], ptr["block_first"], ptr["withdrawals"], ptr["wd_off"], counts["wd_bytes"],
                              *[ptr[k] for k in L.BODIES_INPUTS[5:]])
        rows = {k: (n + 1 if k == "auth_first" else (auth_cap or 0) if k in AUTH else n if k in ALL + TX_EX + ("tx_block",) else nb) for k in want}
        size = {k: WIDTH[k] * rows[k] for k in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out_ptr = lambda k: self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None  # noqa: E731
        base = L.PhantTxsOut(C.sizeof(L.PhantTxsOut), 0xEEEEEEEE, *[out_ptr(k) for k in ALL])
        xout = L.PhantTxsExOut(C.sizeof(L.PhantTxsExOut), 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE, base, *[out_ptr(k) for k in TX_EX + AUTH])
        out = L.PhantBodiesOut(C.sizeof(L.PhantBodiesOut), 0xEEEEEEEE, xout, *[out_ptr(k) for k in BLOCK])
        if sizes:
            arg.struct_size, out.struct_size, out.txs.struct_size, out.txs.base.struct_size = sizes
        fn = ctx._lib.phant_block_bodies_dev if self.dev else ctx._lib.phant_block_bodies
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        del keep
        return rc, got, (int(out.first_bad_block), int(out.txs.base.first_bad), int(out.txs.n_auth), int(out.txs.blob_gas_used))


def check_bodies(P, oracle, block_txs, fork, block_wds=None, forms=(False, True), ctx=None, recover=False, **kw):
    """every answer of the call against the definition, in both forms -> the definition's arrays"""
    exp, *scalars = B.expected(oracle, block_txs, 1, fork, kw.get("base_fee"), kw.get("gas_limit"), kw.get("blob_base_fee"), recover, block_wds,
                               kw.get("exp_txs_root"), kw.get("exp_wd_root"), kw.get("exp_blob_gas"))
    ctx = ctx or _ctx(P)
    for dev in forms:
        rc, got, sc = RawBodies(P, block_txs, block_wds, dev=dev).call(ctx, fork, recover=recover, auth_cap=scalars[2], **kw)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert sc == tuple(scalars), (dev, sc, scalars)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(got[k], exp[k], WIDTH[k]))
    return {k: np.frombuffer(exp[k], "<u4") for k in ("flags", "block_flags", "block_first_bad", "tx_block")} | {"raw": exp}


def _blocks(txs, counts):
    """the transactions dealt out: counts[b] to block b"""
    out, at = [], 0
    for c in counts:
        out.append([txs[(at + k) % len(txs)] for k in range(c)])
        at += c
    return out


def _small(i, **kw):
    """a short transaction of type i % 3 that no rule flags"""
    return raw_tx_012(i % 3, nonce=i, gas=30000, **kw)


# ------------------------------------------------------------------------------------------------------------- one block
@pytest.mark.parametrize("fork", (F.LONDON, F.CANCUN, F.PRAGUE))
def test_one_block_equals_the_ex_call(P, oracle, pool, fork):
    """n_blocks == 1: answer for answer phant_block_transactions_ex over the same bytes, tuples and an auth_cap below n_auth included"""
    txs = pool[:suite.scale(18, 8)]
    ctx = _ctx(P)
    exp, _, n_auth, _ = F.expected(oracle, txs, 1, fork, 7, 30_000_000, 3, True)
    for dev in (False, True):
        for cap in (n_auth, max(n_auth - 1, 0)):
            rc0, got0, fb0, na0, bg0 = RawEx(P, txs, dev=dev).call_ex(ctx, fork, 1, 7, 30_000_000, 3, True, auth_cap=cap)
            rc1, got1, sc = RawBodies(P, [txs], dev=dev).call(ctx, fork, base_fee=[7], gas_limit=[30_000_000], blob_base_fee=[3], recover=True, auth_cap=cap)
            assert rc0 == rc1 == OK and sc[1:] == (fb0, na0, bg0) and na0 == n_auth, (dev, cap)
            for k in ALL + TX_EX + AUTH:
                assert got1[k, "guards"] and got1[k] == got0[k], (dev, cap, k)
                assert got1[k] == (exp[k][:cap * WIDTH[k]] if k in AUTH else exp[k]), (dev, cap, k)
    check_bodies(P, oracle, [txs], fork, base_fee=[7], gas_limit=[30_000_000], blob_base_fee=[3], recover=True)


# ------------------------------------------------------------------------------------------------------------ boundaries
def test_block_boundaries_on_wave_edges_and_empty_blocks(P, oracle, pool):
    """blocks of 0, 1, 63, 0, 0, 64, 65, 1, 0 transactions: boundaries on wave edges, empty blocks first, last and adjacent; every block
    with parameters of its own"""
    counts = (0, 1, 63, 0, 0, 64, 65, 1, 0)
    blocks = _blocks(pool, counts)
    r = check_bodies(P, oracle, blocks, F.PRAGUE, base_fee=[3 + 400_000_000 * b for b in range(9)], gas_limit=[10**5 * (b + 1) for b in range(9)],
                     blob_base_fee=[b for b in range(9)])
    assert r["tx_block"].tolist() == [b for b, c in enumerate(counts) for _ in range(c)]
    assert len(set(r["block_flags"].tolist())) == 2 and [r["block_first_bad"][b] for b in (0, 3, 4, 8)] == [0, 0, 0, 0]


def test_the_same_bytes_pass_in_one_block_and_fail_in_its_neighbour(P, oracle):
    tx = raw_tx_012(2, gas_price=100, max_priority=30, gas=50_000)
    blocks = [[tx, tx], [tx], [tx, tx, tx], [tx]]
    r = check_bodies(P, oracle, blocks, F.LONDON, base_fee=[50, 101, 90, 100], gas_limit=[50_000, 50_000, 49_999, 50_000])
    want = [0, 0, T.FEE_BELOW_BASE, T.GAS_ABOVE_BLOCK, T.GAS_ABOVE_BLOCK, T.GAS_ABOVE_BLOCK, 0]
    assert r["flags"].tolist() == want and r["block_flags"].tolist() == [0, 1, 1, 0] and r["block_first_bad"].tolist() == [2, 0, 0, 1]
    eff = [int.from_bytes(r["raw"]["effective_gas_price"][32 * i:32 * i + 32], "big") for i in range(7)]
    assert eff == [80, 80, 0, 100, 100, 100, 100]


def test_one_block_of_257_and_segments_without_transactions_or_blocks(P, oracle, pool):
    n = suite.scale(257, 70)
    r = check_bodies(P, oracle, [[pool[i % len(pool)] for i in range(n)]], F.PRAGUE, base_fee=[7], gas_limit=[30_000_000])
    assert r["block_first_bad"].tolist() == [int(np.flatnonzero(r["flags"] & F.ERROR_BITS)[0])]
    w = [[B.withdrawal(k) for k in range(b)] for b in range(5)]
    r = check_bodies(P, oracle, [[]] * 5, F.PRAGUE, block_wds=w, base_fee=[1] * 5, exp_blob_gas=[0, 0, 1, 0, 0])
    assert r["block_flags"].tolist() == [0, 0, B.BODY_BLOB_GAS, 0, 0] and r["raw"]["transactions_root"] == oracle.index_root_rlp([]) * 5
    check_bodies(P, oracle, [[]] * 5, F.LONDON)
    for dev in (False, True):
        rc, got, sc = RawBodies(P, [], dev=dev).call(_ctx(P), F.PRAGUE, want=("flags", "auth_first", "block_flags", "transactions_root"))
        assert rc == OK and sc == (0, 0, 0, 0) and all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str))


# ---------------------------------------------------------------------------------------------------------- list lengths
def test_list_lengths_around_the_key_orders_turns(P, oracle):
    """lists of 0, 1, 2, 0x7f, 0x80, 0x81, 0x100 and 0x101 transactions and withdrawals: the keys' turn at 0x80, their second byte at 0x100;
    the roots against the oracle's"""
    lengths = suite.scale((0, 1, 2, 0x7F, 0x80, 0x81, 0x100, 0x101), (0, 1, 2, 0x7F, 0x80, 0x81))
    blocks = [[_small(i, value=i + 7 * b) for i in range(c)] for b, c in enumerate(lengths)]
    wds = [[B.withdrawal(k, amount=k * 1000 + b) for k in range(c)] for b, c in enumerate(reversed(lengths))]
    r = check_bodies(P, oracle, blocks, F.LONDON, block_wds=wds)
    assert not r["block_flags"].any() and len(set(r["raw"]["transactions_root"][32 * b:32 * b + 32] for b in range(len(lengths)))) == len(lengths)
    # only one of the two roots; none: no trie is built, and the other outputs are what they were
    for dev in (False, True):
        raw = RawBodies(P, blocks, wds, dev=dev)
        for want in (("transactions_root",), ("withdrawals_root", "block_flags"), ("block_flags", "flags")):
            rc, got, _ = raw.call(_ctx(P), F.LONDON, recover=False, want=want)
            assert rc == OK and all(got[k, "guards"] and got[k] == r["raw"][k] for k in want), (dev, want)


# ----------------------------------------------------------------------------------------------------------- many blocks
@pytest.mark.parametrize("n_blocks", (255, 256, 257, 300))
def test_many_small_blocks(P, oracle, n_blocks):
    """0 - 2 transactions a block: the bisection over block_first, more tries than a workgroup has lanes"""
    if suite.EMULATED and not suite.FULL and n_blocks in (255, 256):
        n_blocks //= 8
    counts = [(5 * b + b // 7) % 3 for b in range(n_blocks)]
    bad = raw_tx_012(0, gas=20_999)
    blocks = [[bad if (b % 5 == 4 and k == c - 1) else _small(b + k) for k in range(c)] for b, c in enumerate(counts)]
    wds = [[B.withdrawal(b)] * (b % 2) for b in range(n_blocks)]
    r = check_bodies(P, oracle, blocks, F.PRAGUE, block_wds=wds, base_fee=[1 + b for b in range(n_blocks)])
    assert r["block_flags"].any() and r["block_flags"].sum() == sum(1 for b, c in enumerate(counts) if b % 5 == 4 and c)


# ------------------------------------------------------------------------------------------- types 3 and 4, senders
def test_blob_and_set_code_transactions_in_different_blocks(P, oracle):
    """per-block blob_gas_used, a blob base fee that flags one block only, auth_first global over the segment, senders and authorities"""
    mk = lambda typ, **kw: F.make_tx(oracle, D, typ, 1, **kw)  # noqa: E731
    hs = [F.versioned(k) for k in range(5)]
    blocks = [[mk(3, hashes=hs[:2], blob_fee=5), mk(0, nonce=1)], [mk(4, auths=[_auth(oracle, 0), _auth(oracle, 1)], nonce=2)], [],
              [mk(3, hashes=hs[:3], blob_fee=5, nonce=3), mk(4, auths=[_auth(oracle, 2)], nonce=4), mk(3, hashes=hs[4:], blob_fee=9, nonce=5)],
              [mk(2, nonce=6), mk(4, auths=[_auth(oracle, k) for k in range(3, 6)], nonce=7, high_s=True)]]
    kw = dict(base_fee=[7] * 5, gas_limit=[30_000_000] * 5, blob_base_fee=[5, 1, 1, 6, 1], recover=True)
    r = check_bodies(P, oracle, blocks, F.PRAGUE, exp_blob_gas=[2 * 131072, 0, 0, 4 * 131072, 1], **kw)
    assert r["flags"].tolist() == [0, 0, 0, F.BLOB_FEE_BELOW_BASE, 0, 0, 0, T.SIGNATURE]
    assert r["block_flags"].tolist() == [0, 0, 0, B.BODY_TX, B.BODY_TX | B.BODY_BLOB_GAS] and r["block_first_bad"].tolist() == [2, 1, 0, 0, 1]
    assert np.frombuffer(r["raw"]["auth_first"], "<u4").tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 6]
    assert np.frombuffer(r["raw"]["block_blob_gas_used"], "<u8").tolist() == [2 * 131072, 0, 0, 4 * 131072, 0]
    me = oracle.keccak256(S.pubkey_bytes(S.mul(D, S.G)))[12:]
    assert r["raw"]["sender"] == me * 7 + bytes(20)
    x = P.types.block
    res = x.block_bodies(x.pack_bodies(blocks), 1, F.PRAGUE, base_fee=[7] * 5, gas_limit=[30_000_000] * 5, blob_base_fee=[5, 1, 1, 6, 1])
    assert (res.first_bad_block, res.first_bad, res.n_auth, res.blob_gas_used) == (3, 3, 6, 6 * 131072) and res.errors(3) == ["Transaction"]
    assert res.transactions_root.tobytes() == r["raw"]["transactions_root"] and not hasattr(res, "withdrawals_root")
    assert res.sender.tobytes() == r["raw"]["sender"] and len(res.authority) == 6 and res.tx_block.tolist() == [0, 0, 1, 3, 3, 3, 4, 4]
    check_bodies(P, oracle, blocks, F.CANCUN, **kw)


# ------------------------------------------------------------------------------------------------------------ body flags
def test_each_body_flag_alone(P, oracle):
    good, bad = _small(0), raw_tx_012(1, gas=20_999)
    blocks = [[good], [good, good], [good, good, bad, bad], [F.raw_tx(3, hashes=[F.versioned(0)])], [good], []]
    wds = [[B.withdrawal(b)] for b in range(6)]
    exp, *_ = B.expected(oracle, blocks, 1, F.CANCUN, recover=False, block_wds=wds)
    root = lambda k, b: exp[k][32 * b:32 * b + 32]  # noqa: E731
    txr = [root("transactions_root", b) for b in range(6)]
    wdr = [root("withdrawals_root", b) for b in range(6)]
    txr[1], wdr[4] = txr[0], bytes(31) + b"\x01"
    r = check_bodies(P, oracle, blocks, F.CANCUN, block_wds=wds, exp_txs_root=txr, exp_wd_root=wdr, exp_blob_gas=[0, 0, 0, 0, 0, 0])
    assert r["block_flags"].tolist() == [0, B.BODY_TXS_ROOT, B.BODY_TX, B.BODY_BLOB_GAS, B.BODY_WD_ROOT, 0]
    assert r["block_first_bad"].tolist() == [1, 2, 2, 1, 1, 0]
    rc, _, sc = RawBodies(P, blocks[3:], wds[3:]).call(_ctx(P), F.CANCUN, recover=False, exp_wd_root=wdr[3:], exp_blob_gas=[131072, 0, 0], want=("block_flags",))
    assert rc == OK and sc[0] == 1  # the least bad block, not the first in flag order
    rc, _, sc = RawBodies(P, blocks[:1], wds[:1]).call(_ctx(P), F.CANCUN, recover=False, exp_wd_root=wdr[:1], want=())
    assert rc == OK and sc[:2] == (1, 1)


# --------------------------------------------------------------------------------------------------- outputs and buffers
def test_subsets_of_the_outputs_and_unaligned_byte_arrays(P, oracle, pool):
    """each per-block output alone and seeded subsets of everything: the span the host form fetches ends at every position; the byte arrays
    of inputs and outputs at odd addresses"""
    blocks = _blocks(pool, suite.scale((3, 0, 9, 6), (2, 0, 3, 1)))
    wds = [[B.withdrawal(b + k) for k in range(b)] for b in range(4)]
    kw = dict(base_fee=[7, 8, 9, 10], gas_limit=[30_000_000] * 4, blob_base_fee=[3] * 4)
    exp, *scalars = B.expected(oracle, blocks, 1, F.PRAGUE, recover=True, block_wds=wds, **kw)
    rng = np.random.default_rng(11)
    everything = ALL + TX_EX + AUTH + BLOCK
    subsets = [()] + [(k,) for k in BLOCK] + [tuple(k for k in everything if rng.integers(0, 2)) for _ in range(suite.scale(16, 3))]
    ctx = _ctx(P)
    for dev in (False, True):
        raw = RawBodies(P, blocks, wds, dev=dev)
        for want in subsets:
            rc, got, sc = raw.call(ctx, F.PRAGUE, want=want, auth_cap=scalars[2], **kw)
            assert rc == OK and sc == tuple(scalars), (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)
        odd = {k: 1 for k in everything if WIDTH[k] not in (4, 8)}
        rc, got, sc = raw.call(ctx, F.PRAGUE, auth_cap=scalars[2], skew=odd, in_skew=1 if dev else 3, exp_txs_root=[bytes(32)] * 4, **kw)
        assert rc == OK and sc[1:] == tuple(scalars[1:]) and sc[0] == 0
        assert all(got[k, "guards"] and got[k] == exp[k] for k in everything if k != "block_flags")


def test_a_call_beyond_the_pinned_stage(P, oracle):
    """more bytes than the 8 MiB stage holds: the same answers by plain copies"""
    n = suite.scale(180, 3)
    txs = [raw_tx_012(i % 3, nonce=i, data=_data(49152 + (i % 2), i), to=b"" if i % 2 else b"\x22" * 20, gas=10**7) for i in range(n)]
    r = check_bodies(P, oracle, [txs[:2], txs[2:]], F.LONDON, block_wds=[[B.withdrawal(0)], []], gas_limit=[10**7, 10**7 - 1])
    assert r["block_flags"].tolist() == [1, 1] and r["block_first_bad"].tolist() == [1, 0]


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refused_arguments(P, oracle, pool):
    """each returns PHANT_E_INVALID_ARG and touches nothing; in the device form the offsets are caught by the checking kernel"""
    ctx = _ctx(P)
    blocks = _blocks(pool, (2, 0, 3))
    wds = [[B.withdrawal(0)], [], [B.withdrawal(1), B.withdrawal(2)]]
    L = __import__("phant_amd")._lib
    sizes = (C.sizeof(L.PhantBodiesIn), C.sizeof(L.PhantBodiesOut), C.sizeof(L.PhantTxsExOut), C.sizeof(L.PhantTxsOut))

    def refused(raw, code=E_INVALID_ARG, **kw):
        kw.setdefault("auth_cap", 8)
        kw.setdefault("recover", False)
        rc, got, sc = raw.call(ctx, kw.pop("fork", F.PRAGUE), **kw)
        assert rc == code, (rc, kw)
        assert sc == SCALARS_UNTOUCHED, kw
        assert all(set(v) <= {0xEE} for k, v in got.items() if isinstance(k, str)) and all(v for k, v in got.items() if not isinstance(k, str)), kw

    for dev in (False, True):
        raw = RawBodies(P, blocks, wds, dev=dev)
        a = raw.host
        for k in range(4):
            for by in (-8, 8):
                refused(raw, sizes=tuple(s + (by if i == k else 0) for i, s in enumerate(sizes)))
        refused(raw, fork=3)
        refused(raw, reserved=1)
        refused(raw, flags=4)
        refused(raw, flags=L.TXS_HAVE_GAS_LIMIT)  # without gas_limit
        for want in (("sender",), ("sig_status", "flags"), ("authority",), ("auth_status", "block_flags")):
            refused(raw, want=want)
        for k in ("txs", "tx_off", "block_first", "withdrawals", "wd_off"):
            refused(raw, over={k: None})
        refused(raw, over={"n_blocks": 0})
        # offsets and firsts that go backwards, do not begin at 0 or do not end at their totals
        for k in ("tx_off", "wd_off", "block_first", "wd_first"):
            for at, by in ((0, 1), (1, 100), (-1, 1), (-1, -1)):
                lie = a[k].copy()
                lie[at] = (int(lie[at - 1]) - 1 if by == 100 else int(lie[at]) + by) & 0xFFFFFFFF
                if k in ("tx_off", "wd_off") and at == -1 and not dev:
                    continue  # (the host form has no other total than the last offset: its last transaction is as long as that says)
                refused(raw, over={k: lie})
        if dev:
            refused(raw, over={"tx_bytes": raw.tx_bytes + 1})
            refused(raw, over={"wd_bytes": raw.wd_bytes - 1})
        refused(raw, over={"n": raw.n - 1})
        refused(raw, over={"n_wd": raw.n_wd + 1})
        huge = a["wd_off"].copy()
        huge[-1] += 1 << 32
        if not dev:
            refused(raw, code=E_UNSUPPORTED, over={"wd_off": huge})
        # withdrawals without wd_first
        bare = RawBodies(P, blocks, None, dev=dev)
        refused(bare, over={"n_wd": 3})
        refused(bare, over={"withdrawals": a["withdrawals"]})
        refused(bare, over={"wd_off": a["wd_off"]})
        refused(bare, exp_wd_root=[bytes(32)] * 3)
        refused(bare, want=("withdrawals_root",))
    dev = RawBodies(P, blocks, wds, dev=True)
    for k, by in (("blob_off", 4), ("nonce", 2), ("auth_first", 3), ("tx_block", 2), ("block_first_bad", 1), ("block_blob_gas_used", 4), ("block_flags", 2)):
        refused(dev, skew={k: by})


# -------------------------------------------------------------------------------------------------------------- fixtures
def test_the_fixture_segment_and_its_senders(P, oracle):
    """the reference's 87 fixture blocks, each behind its own anchor, through validate_segment: no header flag, no body flag; their 81
    senders through the segment call"""
    from tests import golden
    from tests import headers_ref as H
    chains = H.load_vectors()
    cases = golden.fixtures()["cases"]
    if suite.EMULATED and not suite.FULL:
        chains, cases = chains[::6], cases[::6]
    raws, seg = [], [0]
    for chain in chains:
        raws += [c[3] for c in chain]
        seg.append(len(raws))
    x = P.types.block
    v = x.validate_segment(raws, seg_first=seg, fork=F.LONDON)
    n_bodies = len(raws) - len(chains)
    assert v.first_bad == len(raws) and not v.header_flags.any() and not v.body_flags.any() and v.bodies.n_blocks == n_bodies
    assert v.hashes == [c[1] for chain in chains for c in chain] and v.bodies.first_bad_block == n_bodies
    want = [bytes.fromhex(t) for c in cases for b in c["blocks"] for t in b["tx_values"]]
    assert v.bodies.n == len(want) and (suite.EMULATED or len(want) == 70) and not v.bodies.sig_status.any()
    status, txs, wds = B.split_all([c[3] for chain in chains for c in chain[1:]])
    assert [t for b in txs for t in b] == want and not any(status)
    a, st = x.split_blocks([c[3] for chain in chains for c in chain[1:]])
    assert not st.any() and a["txs"][:int(a["tx_off"][-1])].tobytes() == b"".join(want) and a["wd_first"].tolist() == np.cumsum([0] + [len(w) for w in wds]).tolist()
    # a wrong root in one header: that block alone
    bad = x.block_bodies(a, 1, F.LONDON, transactions_root=[bytes(32)] + [oracle.index_root_rlp(t) for t in txs[1:]], recover=False)
    assert bad.first_bad_block == 0 and bad.block_flags.tolist() == [B.BODY_TXS_ROOT] + [0] * (n_bodies - 1)
    vec = S.load_vectors()["fixtures"]
    if suite.EMULATED and not suite.FULL:
        vec = vec[::13]
    per = [[t["tx"] for t in vec[i:i + 4]] for i in range(0, len(vec), 4)]
    r = x.block_bodies(x.pack_bodies(per), 1, F.PRAGUE, roots=False)
    assert (suite.EMULATED or r.n == 81) and [bytes(s).hex() for s in r.sender] == [t["sender"] for t in vec] and not hasattr(r, "transactions_root")
