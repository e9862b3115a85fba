"""How the trie hasher's, the prover's and the state root's calls cross the bus (phant_amd/csrc/trie_build.hip, state_root.hip; DESIGN.md
sections 7d and 7l): the number of host-to-device, device-to-host and device-to-device hipMemcpyAsync calls, of hipMemsetAsync calls and
of hipStreamSynchronize calls that the SECOND call of a shape makes on one context (the first may grow an arena and allocate the pinned
stage), counted by the emulated runtime (tests/native/shim/hip/hip_runtime.h: hipemu_bus_counters), after the method of
tests/test_emu_call_staging.py.

The numbers in PARENT are those of commit 8264687, the last one in which the host forms of the trie and of the prover each carried
their own validation, staging arrays, rebasing and uploads and every arena was sized by a hand-written sum: they were recorded there,
with this file, before that code was rewritten on top of staging.h's stage_pairs and lay_out_arena.  Every tuple is reproduced exactly
but for one deliberate change: the host form of phant_mpt_prove_nodeset now sends its inputs through the pinned stage, ONE host-to-device
copy where there were five to nine (PROVE_HOST holds the new tuples beside the parent's).  This module runs against the plain emulated
library: the sanitized one poisons the arena's padding, so it never stages.  PROVE_BATCH, ("state_proofs", 40) and ("prove_batch", 50)
were recorded the same way at commit d344bc8, before the prover's two forms were given one host driver.

The last section holds the kernel launches of the same kind of calls (the emulated runtime's hipemu::M.launches, through
tests/native/hipemu_export.cpp: hipemu_counters): LAUNCHES was recorded on commit 343780c, the last one whose forest_device was one
function with its choices, its mailbox protocol and its bins' launches inline, with this file, before that driver was rewritten on top
of trie_plan.h's plan."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import emu
from tests.test_emu_call_staging import bus_of_second


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    if os.environ.get("PHANT_EMU_SANITIZE") == "1":
        pytest.skip("the sanitized library never stages")
    yield from emu.emulated_backend()


def _ctx():
    from phant_amd.context import default_context
    return default_context()


def _kv(seed, n, val_max=80):
    from phant_amd import mpt
    from tests.witness_util import random_kv
    keys, vals = random_kv(np.random.default_rng(seed), n, 32, 1, val_max)
    return keys, vals, [mpt.KeyVal(k, v) for k, v in zip(keys, vals)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def test_trie_roots():
    """phant_mpt_root in both passes and without keys, its device form, the forest with root nodes, the block's lists"""
    from phant_amd import mpt, shard
    got = {}
    for n in (0, 1, 50, 3000):  # (no key, one, the small pass, the general pass: the emulated context takes the small one up to 300 keys)
        kv = _kv(10 + n, n)[2]
        got[("mpt_root", n)] = bus_of_second(lambda: mpt.mptize(kv))
    keys, vals, _ = _kv(3, 50)
    kb, ko = mpt._pack(keys, np.uint32)
    vb, vo = mpt._pack(vals, np.uint64)
    dev = [_dev(a) for a in (kb, ko, vb, vo)]
    got[("mpt_root_dev", 50)] = bus_of_second(lambda: mpt.mptize_dev(dev[0], dev[1].view(__import__("torch").int32), dev[2],
                                                                      dev[3].view(__import__("torch").int64)))
    keys, vals, _ = _kv(4, 200)
    cuts = sorted(np.random.default_rng(4).integers(0, 201, 13).tolist())
    seg = [0] + cuts[:6] + [cuts[5]] + cuts[6:] + [cuts[-1], 200]  # 16 tries, (at least) two of them empty
    assert len(seg) == 17
    got[("mpt_root_nodes", 200)] = bus_of_second(lambda: shard.gpu_root_nodes(keys, vals, seg))
    rng = np.random.default_rng(5)
    lists = [[rng.integers(0, 256, int(rng.integers(60, 200)), dtype=np.uint8).tobytes() for _ in range(20)] for _ in range(3)]
    got[("block_roots", 60)] = bus_of_second(lambda: mpt.block_roots(lists))
    got[("index_root_be32", 20)] = bus_of_second(lambda: mpt.index_root_be32(lists[0]))
    print(got)
    assert got == {k: PARENT[k] for k in got}, got


def _prove_call(keys, vals, queries, seg=None, q_trie=None, q_flags=None, want=True, dev=False, batch=False):
    """-> a closure that makes one phant_mpt_prove_nodeset[_dev] (batch: phant_mpt_prove_batch[_dev]) call with every output wanted, or none"""
    import torch
    from phant_amd import _lib as L, mpt
    ctx = _ctx()
    kb, ko = mpt._pack(keys, np.uint32)
    vb, vo = mpt._pack(vals, np.uint64)
    qb, qo = mpt._pack(queries, np.uint32)
    n, nq = len(keys), len(queries)
    n_tries = 1 if seg is None else len(seg) - 1
    ins = [kb, ko, vb, vo, None if seg is None else np.asarray(seg, np.uint32), qb, qo,
           None if q_trie is None else np.asarray(q_trie, np.uint32), None if q_flags is None else np.asarray(q_flags, np.uint8)]
    max_nodes, cap = 8 * nq + 64, (8 * nq + 64) * 256
    outs = [np.zeros(cap, np.uint8), np.zeros(max_nodes + 1, np.uint64), np.zeros((nq if batch else n_tries) + 1, np.uint32),
            np.zeros(n_tries * 32, np.uint8), np.zeros(max(nq, 1), np.uint8)]
    if dev:
        ins = [None if a is None else _dev(a) for a in ins]
        outs = [torch.from_numpy(a.view(np.uint8)).cuda() for a in outs]
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr()) if dev else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    po = [p(a) if want else None for a in outs]
    Out = L.PhantProveBatchOut if batch else L.PhantProveOut
    o = Out(C.sizeof(Out), max_nodes, cap, *po, 0, 0, 0)

    def call():
        if batch and dev:
            rc = ctx._lib.phant_mpt_prove_batch_dev(ctx.handle, p(ins[0]), p(ins[1]), len(kb) if n else 0, p(ins[2]), p(ins[3]), int(vo[-1]), n,
                                                    p(ins[4]), n_tries, p(ins[5]), p(ins[6]), int(qo[-1]), p(ins[7]), nq, C.byref(o))
        elif batch:
            rc = ctx._lib.phant_mpt_prove_batch(ctx.handle, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), n, p(ins[4]), n_tries, p(ins[5]), p(ins[6]),
                                                p(ins[7]), nq, C.byref(o))
        elif dev:
            rc = ctx._lib.phant_mpt_prove_nodeset_dev(ctx.handle, p(ins[0]), p(ins[1]), len(kb) if n else 0, p(ins[2]), p(ins[3]),
                                                      int(vo[-1]), n, p(ins[4]), n_tries, p(ins[5]), p(ins[6]), int(qo[-1]), p(ins[7]), p(ins[8]),
                                                      nq, C.byref(o))
        else:
            rc = ctx._lib.phant_mpt_prove_nodeset(ctx.handle, p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), n, p(ins[4]), n_tries, p(ins[5]),
                                                  p(ins[6]), p(ins[7]), p(ins[8]), nq, C.byref(o))
        ctx.check(rc)
        assert o.total_nodes <= max_nodes and o.nodes_len <= cap and (o.total_nodes > 0) == (n > 0 and nq > 0)
    call.keep = (ins, outs)
    return call


def test_prove_nodeset():
    """phant_mpt_prove_nodeset: one trie with every output and with none, three tries with q_trie and q_flags, no keys; the device form"""
    keys, vals, _ = _kv(6, 200)
    rng = np.random.default_rng(6)
    queries = [keys[i] for i in rng.choice(200, 7, replace=False)] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
    got = {("all outputs", 200): bus_of_second(_prove_call(keys, vals, queries)),
           ("no output", 200): bus_of_second(_prove_call(keys, vals, queries, want=False)),
           ("three tries", 200): bus_of_second(_prove_call(keys, vals, queries, seg=[0, 70, 70, 200], q_trie=[0, 2, 2, 0, 1, 2, 0, 2, 1, 0],
                                                             q_flags=[1, 0, 0, 1, 0, 0, 0, 1, 0, 0])),
           ("no keys", 0): bus_of_second(_prove_call([], [], queries[:3]))}
    print(got)
    for k, v in got.items():
        parent, now = PROVE_HOST[k]
        assert v == now, (k, v)
        assert now[1:] == parent[1:] and now[0] == 1 and now[0] <= parent[0], k  # (every shape has a query: there is input)
    dev = {("prove_nodeset_dev", 200): bus_of_second(_prove_call(keys, vals, queries, dev=True))}
    print(dev)
    assert dev == {k: PARENT[k] for k in dev}, dev


def test_prove_batch():
    """phant_mpt_prove_batch on the shapes of test_prove_nodeset (it has no q_flags), and its device form"""
    keys, vals, _ = _kv(6, 200)
    rng = np.random.default_rng(6)
    queries = [keys[i] for i in rng.choice(200, 7, replace=False)] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
    got = {("all outputs", 200): bus_of_second(_prove_call(keys, vals, queries, batch=True)),
           ("no output", 200): bus_of_second(_prove_call(keys, vals, queries, want=False, batch=True)),
           ("three tries", 200): bus_of_second(_prove_call(keys, vals, queries, seg=[0, 70, 70, 200], q_trie=[0, 2, 2, 0, 1, 2, 0, 2, 1, 0],
                                                             batch=True)),
           ("no keys", 0): bus_of_second(_prove_call([], [], queries[:3], batch=True)),
           ("prove_batch_dev", 200): bus_of_second(_prove_call(keys, vals, queries, dev=True, batch=True))}
    print(got)
    assert got == PROVE_BATCH, got


def _state(seed=7, n=40, m=200):
    from phant_amd.state import AccountState
    rng = np.random.default_rng(seed)
    per = np.bincount(rng.integers(0, n, m), minlength=n)
    acc = []
    for i in range(n):
        storage = {}
        while len(storage) < per[i]:  # (a few zero values among them: slots that do not exist)
            storage[int.from_bytes(rng.bytes(32), "big")] = 0 if rng.integers(0, 10) == 0 else int.from_bytes(rng.bytes(int(rng.integers(1, 33))), "big")
        acc.append(AccountState(rng.bytes(20), int(rng.integers(0, 1000)), int.from_bytes(rng.bytes(12), "big"),
                                rng.bytes(int(rng.integers(0, 300))) if i % 3 == 0 else b"", storage))
    return acc


def test_state():
    """phant_state_root without and with accounts, its device form, the sub-trie nodes and phant_state_witness on the same state"""
    from phant_amd import state, stateless
    acc = _state()
    got = {("state_root", 0): bus_of_second(lambda: state.state_root([])),
           ("state_root", 40): bus_of_second(lambda: state.state_root(acc))}
    soa = state.soa_dev(acc)
    got[("state_root_dev", 40)] = bus_of_second(lambda: state.state_root_dev(soa))
    got[("state_subtrie_nodes", 40)] = bus_of_second(lambda: state.state_subtrie_nodes(acc))
    rng = np.random.default_rng(8)
    held = [a for a in acc if a.storage]
    touched = [acc[1].addr, acc[2].addr, rng.bytes(20), rng.bytes(20)]  # accounts: two held, two absent
    touched += [a.addr + int(s).to_bytes(32, "big") for a in held[:3] for s in list(a.storage)[:1]]  # slots: three held,
    touched += [held[0].addr + rng.bytes(32), held[1].addr + rng.bytes(32), rng.bytes(52)]  # two absent, one of an absent account
    assert len(touched) == 10
    got[("state_witness", 40)] = bus_of_second(lambda: stateless.build_witness(acc, touched, may_remove=touched[4:6]))
    got[("state_proofs", 40)] = bus_of_second(lambda: state.get_proofs(acc, touched))
    print(got)
    assert got == {k: PARENT[k] for k in got}, got


# ---- kernel launches ----
LAUNCH_SETTINGS = {"side": {"trie_side_min_keys": 0}, "side_behind": {"trie_side_min_keys": 0, "trie_ahead_max_keys": 0},
                   "side_join": {"trie_side_min_keys": 0, "trie_join_in_stream": 1}, "blocks1_grid1": {"trie_slot_blocks": 1, "trie_fallback_grid": 1},
                   "no_wave": {"trie_no_wave": 1}, "no_coop": {"trie_no_coop": 1}}
LAUNCH_KNOB_DEFAULTS = {"trie_side_min_keys": -1, "trie_ahead_max_keys": -1, "trie_join_in_stream": 0, "trie_slot_blocks": 0, "trie_fallback_grid": -1,
                        "trie_no_wave": 0, "trie_no_coop": 0}


def launches_of_second(call):
    """kernel launches of the second of two equal calls"""
    lib = _ctx()._lib
    out = (C.c_ulonglong * 3)()
    call()
    lib.hipemu_counters(out)
    before = out[0]
    call()
    lib.hipemu_counters(out)
    return out[0] - before


def test_launches_held_to_parent():
    """phant_mpt_root without keys, with one, in the small and in the general pass; the general pass under the knobs that move its
    launches (the helper stream with the leaves ahead, behind and joined in the stream, one-block slots with a one-workgroup fallback,
    no wave-per-node and no thin-bin kernels at all); the forest with root nodes; a block's lists; one host call of the prover"""
    from phant_amd import mpt, shard
    from tests.witness_util import random_kv
    ctx = _ctx()
    got = {}
    for n in (0, 1, 50, 3000):
        kv = _kv(10 + n, n)[2]
        got[("mpt_root", n)] = launches_of_second(lambda: mpt.mptize(kv))
    # (keys that share their first byte: the root is an extension, no bin at depth 0 -- order_kernel sends bins to the helper stream)
    kv = [mpt.KeyVal(k, v) for k, v in zip(*random_kv(np.random.default_rng(3010), 3000, 32, 1, 80, shared_prefix_nibbles=2))]
    for name, knobs in dict({"shared_byte": {}}, **LAUNCH_SETTINGS).items():
        try:
            for k, v in knobs.items():
                ctx.diag_set(k, v)
            got[(name, 3000)] = launches_of_second(lambda: mpt.mptize(kv))
        finally:
            for k, v in LAUNCH_KNOB_DEFAULTS.items():
                ctx.diag_set(k, v)
    keys, vals, _ = _kv(4, 200)
    cuts = sorted(np.random.default_rng(4).integers(0, 201, 13).tolist())
    seg = [0] + cuts[:6] + [cuts[5]] + cuts[6:] + [cuts[-1], 200]  # 16 tries, (at least) two of them empty
    got[("mpt_root_nodes", 200)] = launches_of_second(lambda: shard.gpu_root_nodes(keys, vals, seg))
    rng = np.random.default_rng(5)
    lists = [[rng.integers(0, 256, int(rng.integers(60, 200)), dtype=np.uint8).tobytes() for _ in range(20)] for _ in range(3)]
    got[("block_roots", 60)] = launches_of_second(lambda: mpt.block_roots(lists))
    keys, vals, _ = _kv(6, 50)
    rng = np.random.default_rng(6)
    queries = [keys[i] for i in rng.choice(50, 7, replace=False)] + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(3)]
    got[("prove_nodeset", 50)] = launches_of_second(_prove_call(keys, vals, queries))
    got[("prove_batch", 50)] = launches_of_second(_prove_call(keys, vals, queries, batch=True))
    print(got)
    assert got == LAUNCHES, got


# ---- recorded at commit 343780c (see the module's docstring): kernel launches
LAUNCHES = {("mpt_root", 0): 1, ("mpt_root", 1): 2, ("mpt_root", 50): 2, ("mpt_root", 3000): 13, ("shared_byte", 3000): 14, ("side", 3000): 15,
            ("side_behind", 3000): 15, ("side_join", 3000): 15, ("blocks1_grid1", 3000): 21, ("no_wave", 3000): 14, ("no_coop", 3000): 14,
            ("mpt_root_nodes", 200): 2, ("block_roots", 60): 2, ("prove_nodeset", 50): 9, ("prove_batch", 50): 12}

# ---- recorded at commit 8264687 (see the module's docstring): (H2D, D2H, D2D, memsets, stream synchronisations)
PARENT = {("mpt_root", 0): (1, 0, 0, 0, 1), ("mpt_root", 1): (1, 0, 0, 0, 1), ("mpt_root", 50): (1, 0, 0, 0, 1), ("mpt_root", 3000): (1, 0, 0, 0, 1),
          ("mpt_root_dev", 50): (1, 0, 0, 0, 0), ("mpt_root_nodes", 200): (1, 0, 0, 0, 1), ("block_roots", 60): (1, 0, 0, 0, 1),
          ("index_root_be32", 20): (1, 0, 0, 0, 1), ("prove_nodeset_dev", 200): (1, 1, 0, 2, 2),
          ("state_root", 0): (1, 0, 0, 0, 1), ("state_root", 40): (9, 6, 0, 2, 5), ("state_root_dev", 40): (1, 6, 1, 3, 4),
          ("state_subtrie_nodes", 40): (9, 8, 0, 3, 5), ("state_witness", 40): (15, 13, 0, 6, 11),
          ("state_proofs", 40): (13, 16, 0, 6, 13)}
# ---- recorded at commit d344bc8, the last one in which the two forms of the prover each had their own host driver: phant_mpt_prove_batch
# on the shapes of PROVE_HOST and its device form; ("state_proofs", 40) in PARENT and ("prove_batch", 50) in LAUNCHES are of that commit too
PROVE_BATCH = {("all outputs", 200): (1, 6, 0, 2, 4), ("no output", 200): (1, 1, 0, 2, 4), ("three tries", 200): (1, 6, 0, 2, 4),
               ("no keys", 0): (1, 4, 0, 2, 2), ("prove_batch_dev", 200): (1, 1, 0, 2, 4)}
# phant_mpt_prove_nodeset, host form: (the parent's tuple, the tuple since its inputs cross through the pinned stage)
PROVE_HOST = {("all outputs", 200): ((7, 6, 0, 2, 3), (1, 6, 0, 2, 3)), ("no output", 200): ((7, 1, 0, 2, 3), (1, 1, 0, 2, 3)),
              ("three tries", 200): ((9, 6, 0, 2, 3), (1, 6, 0, 2, 3)), ("no keys", 0): ((5, 5, 0, 2, 3), (1, 5, 0, 2, 3))}
