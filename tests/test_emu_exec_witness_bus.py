"""How the execution-witness calls cross the bus (phant_exec_witness_prestate, phant_exec_witness_poststate and
phant_exec_witness_advance): the number of host-to-device, device-to-host and device-to-device hipMemcpyAsync
calls, of hipMemsetAsync calls and of hipStreamSynchronize calls that the SECOND of two equal calls makes on one context (the first may
grow the arena and the node-set workspace), counted by the emulated runtime (tests/native/hipemu_export.cpp: hipemu_bus_counters), the
launchers' own memsets included.  These calls do not use the pinned stage: every array is a copy of its own, a NULL output or an empty
array is no copy.

The numbers are those of commit 98de331, the last one in which the pre-state call and the post-state run each carried their own copy
of the pre-state stage: they were recorded there, with this file, before the stage was written once, and have not been touched since.
A count may only ever fall below its entry here where a copy of zero bytes went away, and the entry then says so; none does."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import emu
from tests import poststate_ref as Q
from tests import prestate_ref as R


@pytest.fixture(scope="module", autouse=True)
def _emulated_backend():
    yield from emu.emulated_backend()


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


from tests.test_gpu_poststate import _acc, _contract, _raw_case, small_case  # noqa: E402


def _ctx():
    from phant_amd.context import default_context
    return default_context()


def bus_of_second(call):
    """(H2D, D2H, D2D, memsets, stream synchronisations) of the second of two equal calls (as tests/test_emu_call_staging.py counts)"""
    lib = _ctx()._lib
    out = (C.c_ulonglong * 5)()
    call()
    lib.hipemu_bus_counters(out)
    before = tuple(out)
    call()
    lib.hipemu_bus_counters(out)
    return tuple(a - b for a, b in zip(out, before))


def test_prestate(P, oracle):
    rng = np.random.default_rng(5)
    full = R.full_witness(oracle, [_contract(rng, b"\x60\x01"), _contract(rng, b"\x60\x02\x00"), _acc(rng)], rng)
    plain = R.full_witness(oracle, [_acc(rng), _acc(rng)], rng)
    only_code = ({"state": [], "codes": [R._hex(b"\x60\x00")], "keys": []}, full[1])
    got = {}
    for name, (doc, root), shape in (("3 accounts, 4 slots, 2 codes", full, (3, 4, 2)), ("2 accounts", plain, (2, 0, 0)),
                                     ("no account, one code", only_code, (0, 0, 1))):
        w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
        try:
            i = w.info()
            assert (i["n_accounts"], i["n_slots"], i["n_codes"]) == shape
            want = R.prestate_ref(oracle, doc, root, strict=True)

            def wanted():
                r = w.prestate_arrays(None, root)
                assert all(r[k] == want[k] for k in ("n_failed", "n_missing_code", "n_unused_codes")) and r["n_failed"] == 0
                assert np.array_equal(r["slot_vals"], want["slot_vals"]) and np.array_equal(r["code_index"], want["code_index"])

            def nothing_wanted():
                o = P.stateless.PrestateOut()
                o.struct_size = C.sizeof(P.stateless.PrestateOut)
                ctx = _ctx()
                assert ctx._lib.phant_exec_witness_prestate(ctx.handle, w._h, C.create_string_buffer(root, 32), C.byref(o)) == 0
                assert (o.n_failed, o.n_missing_code, o.n_unused_codes) == (0, want["n_missing_code"], want["n_unused_codes"])

            got[name, "all outputs"] = bus_of_second(wanted)
            if shape == (3, 4, 2):
                got[name, "no output"] = bus_of_second(nothing_wanted)
        finally:
            w.close()
    print(got)
    assert got == PRESTATE, got


def test_poststate_and_advance(P, oracle):
    rng = np.random.default_rng(6)
    doc, root, accounts, writes = small_case(oracle, rng)
    got = {}
    w = P.stateless.StatelessWitness.parse_json(R.dumps(doc))
    try:
        info = w.info()
        assert (info["n_accounts"], info["n_slots"]) == (3, 4)
        arr = Q.write_arrays(oracle, info, writes)
        assert sorted(arr["account_op"].tolist()) == [Q.KEEP, Q.SET, Q.DELETE] and arr["slot_write"].all()
        want = Q.expected(oracle, info, accounts, writes)

        def post(arrays, want_root):
            def call():
                r = w.poststate_arrays(None, root, arrays)
                assert r["n_failed"] == 0 and r["state_root"] == want_root
            return call

        def advance(keep_old):
            def call():
                r, nxt = w.advance_arrays(None, root, arr, keep_old)
                assert r["n_failed"] == 0 and r["state_root"] == want["state_root"] and nxt is not None
                nxt.close()
            return call

        got["poststate", "SET, DELETE, KEEP with a slot write"] = bus_of_second(post(arr, want["state_root"]))
        got["poststate", "all KEEP, no post array"] = bus_of_second(post({"account_op": np.zeros(3, np.uint8)}, root))
        got["advance", "plain"] = bus_of_second(advance(False))
        got["advance", "KEEP_OLD"] = bus_of_second(advance(True))
    finally:
        w.close()

    # PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS: the slots' 32 bytes take the place of their hashes on the device
    stem = "ab" + "0" * 61

    def raw():
        r, sroot, want_root = _raw_case(P, oracle, {"c" + "1" * 63: 7, stem + "1": 5}, {stem + "2": 6}, copy.deepcopy(rng))
        assert r["n_failed"] == 0 and r["state_root"] == want_root and r["storage_roots"][0].tobytes() == sroot

    got["poststate", "raw slot keys"] = bus_of_second(raw)
    print(got)
    assert got == POSTSTATE, got


# ---- recorded at commit 98de331 (see the module's docstring): (H2D, D2H, D2D, memsets, stream synchronisations)
PRESTATE = {("3 accounts, 4 slots, 2 codes", "all outputs"): (8, 9, 0, 3, 1), ("3 accounts, 4 slots, 2 codes", "no output"): (8, 1, 0, 3, 1),
            ("2 accounts", "all outputs"): (6, 7, 0, 3, 1), ("no account, one code", "all outputs"): (5, 1, 0, 3, 1)}
POSTSTATE = {("poststate", "SET, DELETE, KEEP with a slot write"): (13, 7, 0, 4, 1), ("poststate", "all KEEP, no post array"): (8, 7, 0, 4, 1),
             ("poststate", "raw slot keys"): (13, 7, 1, 4, 1), ("advance", "plain"): (13, 11, 0, 6, 1), ("advance", "KEEP_OLD"): (13, 11, 0, 6, 1)}
