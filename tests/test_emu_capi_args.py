"""Argument handling of the C-ABI (capi.hip) exercised on the emulated library: what a binding gets back for
NULL pointers, empty batches, optional outputs left out, a slot used twice -- the error codes and messages
include/phant_gpu.h promises ("nothing aborts or throws across the boundary").  The GPU box cannot tell more
about these host-side paths than the host does."""
import ctypes as C

import numpy as np
import pytest

from tests import emu
from tests.witness_util import random_kv, pack_proofs

OK, E_INVALID_ARG, E_UNSORTED = 0, -1, -5


@pytest.fixture(scope="module")
def L():
    try:
        lib = emu.mirror_lib()
    except RuntimeError as e:
        pytest.skip(str(e))
    return lib


@pytest.fixture()
def ctx(L):
    c = emu.mirror_context(L)
    yield c
    c.close()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _small_batch(oracle):
    rng = np.random.default_rng(3)
    keys, vals = random_kv(rng, 40, 32, 1, 60)
    t = oracle.Trie(keys, vals)
    nodes, node_off, pfn = pack_proofs([t.prove(k) for k in keys[:10]])
    return (np.frombuffer(t.root(), np.uint8).copy(), np.frombuffer(b"".join(keys[:10]), np.uint8).copy(), nodes,
            node_off, pfn)


def test_null_ctx_and_empty_batches(L, ctx, oracle):
    root, keys, nodes, node_off, pfn = _small_batch(oracle)
    st = np.zeros(10, np.uint8)
    assert L.phant_mpt_verify_batch(None, _p(root), 1, None, _p(keys), 32, _p(nodes), nodes.size, _p(node_off), _p(pfn),
                                    10, _p(st), None, None) == E_INVALID_ARG
    assert L.phant_keccak256_batch(None, None, None, 0, None) == E_INVALID_ARG
    # n == 0 is a no-op whatever else is passed
    assert L.phant_mpt_verify_batch(ctx.handle, None, 0, None, None, 32, None, 0, None, None, 0, None, None, None) == OK
    assert L.phant_keccak256_batch(ctx.handle, None, None, 0, None) == OK
    assert L.phant_logs_bloom(ctx.handle, None, None, None, 0, 0, None) == OK
    assert L.phant_sender_addresses(ctx.handle, None, 64, 0, None) == OK
    out = np.zeros(32, np.uint8)
    assert L.phant_mpt_root(ctx.handle, None, None, None, None, 0, _p(out)) == OK
    assert out.tobytes().hex() == "56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421"  # mpt.zig:10


def test_null_pointers_are_reported_not_dereferenced(L, ctx, oracle):
    root, keys, nodes, node_off, pfn = _small_batch(oracle)
    st = np.zeros(10, np.uint8)
    args = [ctx.handle, _p(root), 1, None, _p(keys), 32, _p(nodes), nodes.size, _p(node_off), _p(pfn), 10, _p(st), None, None]
    assert L.phant_mpt_verify_batch(*args) == OK and (st == 1).all()       # optional outputs left out: fine
    for hole in (1, 4, 8, 9, 11):                                          # roots, keys, node_off, pfn, status
        bad = list(args)
        bad[hole] = None
        assert L.phant_mpt_verify_batch(*bad) == E_INVALID_ARG, hole
        assert L.phant_last_error(ctx.handle)                              # a message, ctx-owned
    bad = list(args)
    bad[2] = 0                                                             # no roots
    assert L.phant_mpt_verify_batch(*bad) == E_INVALID_ARG
    assert L.phant_keccak256_batch(ctx.handle, _p(nodes), None, 3, _p(st)) == E_INVALID_ARG
    off = np.array([0, 10, 5], np.uint64)                                  # not monotone
    assert L.phant_keccak256_batch(ctx.handle, _p(nodes), _p(off), 2, _p(np.zeros(64, np.uint8))) == E_INVALID_ARG
    assert L.phant_sender_addresses(ctx.handle, _p(nodes), 63, 1, _p(st)) == E_INVALID_ARG  # stride < 64
    assert L.phant_logs_bloom(ctx.handle, _p(nodes), None, None, 2, 1, _p(np.zeros(256, np.uint8))) == E_INVALID_ARG


def test_value_outputs_are_optional_one_by_one(L, ctx, oracle):
    root, keys, nodes, node_off, pfn = _small_batch(oracle)
    want = oracle.mpt_verify_batch(root, None, keys, 32, nodes, node_off, pfn)
    for with_off, with_len in ((True, False), (False, True), (True, True)):
        st, vo, vl = np.zeros(10, np.uint8), np.zeros(10, np.uint64), np.zeros(10, np.uint32)
        rc = L.phant_mpt_verify_batch(ctx.handle, _p(root), 1, None, _p(keys), 32, _p(nodes), nodes.size, _p(node_off),
                                      _p(pfn), 10, _p(st), _p(vo) if with_off else None, _p(vl) if with_len else None)
        assert rc == OK and np.array_equal(st, want[0])
        assert not with_off or np.array_equal(vo, want[1])
        assert not with_len or np.array_equal(vl, want[2])


def test_unsorted_keys_and_slot_reuse(L, ctx, oracle):
    keys = np.frombuffer(b"\x02\x01", np.uint8).copy()
    koff = np.array([0, 1, 2], np.uint32)
    vals = np.frombuffer(b"ab", np.uint8).copy()
    voff = np.array([0, 1, 2], np.uint64)
    out = np.zeros(32, np.uint8)
    assert L.phant_mpt_root(ctx.handle, _p(keys), _p(koff), _p(vals), _p(voff), 2, _p(out)) == E_UNSORTED  # mpt.zig:39
    root, k, nodes, node_off, pfn = _small_batch(oracle)
    st, vo, vl = np.zeros(10, np.uint8), np.zeros(10, np.uint64), np.zeros(10, np.uint32)
    sub = [ctx.handle, 1, _p(root), 1, None, _p(k), 32, _p(nodes), nodes.size, _p(node_off), _p(pfn), 10, _p(st), _p(vo), _p(vl)]
    assert L.phant_mpt_verify_submit(*sub) == OK
    assert L.phant_mpt_verify_submit(*sub) == E_INVALID_ARG                # the slot is in flight
    assert L.phant_wait(ctx.handle, 1) == OK and (st == 1).all()
    assert L.phant_wait(ctx.handle, 1) == OK                               # waiting on an idle slot is harmless
    sub[1] = 99
    assert L.phant_mpt_verify_submit(*sub) == E_INVALID_ARG                # no such slot
    assert L.phant_wait(ctx.handle, 99) == E_INVALID_ARG


def test_plain_c_caller(L, tmp_path):
    """include/phant_gpu.h from plain C99 (what Zig's @cImport sees): compiles with -pedantic, links against the
    library by symbol name, gets the reference's known answers."""
    import os
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lib_dir = os.path.dirname(emu.build())
    exe = str(tmp_path / "c_binding")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(emu.ROOT, "include"),
                        os.path.join(emu.ROOT, "tests", "native", "c_binding.c"), "-L", lib_dir, "-lphant_emu",
                        "-Wl,-rpath," + lib_dir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "c binding OK" in r.stdout, r.stdout + r.stderr


MAX_SLOTS = 4  # PHANT_MAX_SLOTS


def _verify_entry_points(h, comm, oracle):
    """name -> (valid arguments, indices of the pointers it refuses to go without, index of n, index of the slot or None,
    index of the fail counts or None) for the ten verify entry points; the arrays behind the pointers; the fail counts."""
    root, keys, nodes, node_off, pfn = _small_batch(oracle)
    rng = np.random.default_rng(5)
    k2, v2 = random_kv(rng, 40, 32, 1, 60)
    t = oracle.Trie(k2, v2)
    from tests.witness_util import node_set
    snodes, soff = node_set([t.prove(k) for k in k2[:10]])
    sroot, skeys = np.frombuffer(t.root(), np.uint8).copy(), np.frombuffer(b"".join(k2[:10]), np.uint8).copy()
    st, vo, vl, fail = np.zeros(10, np.uint8), np.zeros(10, np.uint64), np.zeros(10, np.uint32), np.zeros(1, np.uint32)
    m, total = soff.size - 1, node_off.size - 1
    keep = (root, keys, nodes, node_off, pfn, snodes, soff, sroot, skeys, st, vo, vl, fail)
    proof = [_p(root), 1, None, _p(keys), 32, _p(nodes), nodes.size, _p(node_off)]
    nset = [_p(sroot), 1, None, _p(skeys), 32, _p(snodes), snodes.size, _p(soff)]
    outs = [_p(st), _p(vo), _p(vl)]
    E = {
        "phant_mpt_verify_batch": ([h, *proof, _p(pfn), 10, *outs], (1, 4, 6, 8, 9, 11), 10, None, None),
        "phant_mpt_verify_batch_dev": ([h, *proof, total, _p(pfn), 10, *outs], (1, 4, 8, 10, 12), 11, None, None),
        "phant_mpt_verify_verdict_dev": ([h, *proof, total, _p(pfn), 10, *outs, _p(fail)], (1, 4, 8, 10, 12, 15), 11, None, 15),
        "phant_mpt_verify_nodeset": ([h, *nset, m, 10, *outs], (1, 4, 6, 8, 11), 10, None, None),
        "phant_mpt_verify_nodeset_dev": ([h, *nset, m, 10, *outs], (1, 4, 8, 11), 10, None, None),
        "phant_mpt_verify_nodeset_verdict_dev": ([h, *nset, m, 10, *outs, _p(fail)], (1, 4, 8, 11), 10, None, 14),
        "phant_mpt_verify_submit": ([h, 2, *proof, _p(pfn), 10, *outs], (2, 5, 7, 9, 10, 12), 11, 1, None),
        "phant_mpt_verify_nodeset_submit": ([h, 2, *nset, m, 10, *outs], (2, 5, 7, 9, 12), 11, 1, None),
        "phant_mpt_verify_sharded": ([comm, *proof, _p(pfn), 10, *outs, _p(fail)], (1, 4, 6, 8, 9, 11), 10, None, 14),
        # (node_group null: every node shared)
        "phant_mpt_verify_nodeset_sharded": ([comm, *nset, m, None, 10, *outs, _p(fail)], (1, 4, 6, 8, 12), 11, None, 15),
    }
    return E, keep, fail


@pytest.fixture()
def comm1(L):
    h = C.c_void_p()
    assert L.phant_comm_create(None, 1, 0, C.byref(h)) == OK
    yield h
    L.phant_comm_destroy(h)


def test_verify_entry_point_contracts(L, ctx, comm1, oracle):
    """The argument contract of every verify entry point, table-driven: what each refuses (with a message of its own) and
    what it accepts as a no-op, including where the forms differ (the _verdict_dev forms with n == 0)."""
    E, _keep, fail = _verify_entry_points(ctx.handle, comm1, oracle)
    assert len(E) == 10

    def refused(name, args, fresh_message=True):
        f = getattr(L, name)
        sharded = name.endswith("_sharded")
        # a message nothing of the call under test writes, so that the one read afterwards is the refusal's own
        if sharded:
            assert L.phant_comm_allreduce_verdict(comm1, (C.c_void_p * 1)(None), 1) == E_INVALID_ARG
            before = L.phant_comm_last_error(comm1)
        else:
            assert L.phant_diag_set(ctx.handle, 0xFFFF, 0) == E_INVALID_ARG
            before = L.phant_last_error(ctx.handle)
        assert f(*args) == E_INVALID_ARG, (name, args)
        msg = L.phant_comm_last_error(comm1) if sharded else L.phant_last_error(ctx.handle)
        assert msg, name
        if fresh_message:
            assert msg != before and b"mpt_verify" in msg, (name, msg)

    for name, (args, required, n_at, slot_at, fail_at) in E.items():
        f = getattr(L, name)
        handle_at = 0
        n_roots_at, key_len_at = (3, 6) if slot_at is not None else (2, 5)
        # the valid call
        fail[:] = 7
        assert f(*args) == OK, (name, L.phant_last_error(ctx.handle))
        if slot_at is not None:
            assert L.phant_wait(ctx.handle, args[slot_at]) == OK
        # a null handle
        bad = list(args)
        bad[handle_at] = None
        assert f(*bad) == E_INVALID_ARG, name
        # each required pointer missing, one at a time
        for hole in required:
            bad = list(args)
            bad[hole] = None
            refused(name, bad)
        # no roots; a key length beyond 2^30 - 1
        bad = list(args)
        bad[n_roots_at] = 0
        refused(name, bad)
        bad = list(args)
        bad[key_len_at] = 0x40000000
        refused(name, bad)
        # n == 0 with every array null: a no-op -- except for phant_mpt_verify_verdict_dev, which insists on its counts
        empty = [a if i == handle_at or i == slot_at or not (a is None or isinstance(a, C.c_void_p)) else None
                 for i, a in enumerate(args)]
        empty[n_at], empty[n_roots_at] = 0, 0
        if name == "phant_mpt_verify_verdict_dev":
            refused(name, empty)
        else:
            assert f(*empty) == OK, name
        # n == 0 with counts to fill: zeroed by every form that takes them
        if fail_at is not None:
            zero = list(empty)
            zero[n_roots_at], zero[fail_at] = 1, _p(fail)
            fail[:] = 7
            assert f(*zero) == OK, name
            assert fail[0] == 0, name
            if name == "phant_mpt_verify_verdict_dev":
                zero[n_roots_at] = 0
                refused(name, zero)
        # the streaming forms: a slot in flight (of either form) and a slot that does not exist
        if slot_at is not None:
            assert f(*args) == OK
            for other in ("phant_mpt_verify_submit", "phant_mpt_verify_nodeset_submit"):
                refused(other, E[other][0])
                busy_empty = list(E[other][0])
                busy_empty[11] = 0
                refused(other, busy_empty)
            assert L.phant_wait(ctx.handle, args[slot_at]) == OK
            bad = list(args)
            bad[slot_at] = MAX_SLOTS
            refused(name, bad, fresh_message=False)
