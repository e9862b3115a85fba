"""What the prover's entry points say when they refuse their arguments: phant_last_error after every refusal that phant_mpt_prove_nodeset,
phant_mpt_prove_batch, their device forms, phant_state_witness and phant_state_proofs can make from bad arguments alone, character for
character, on the emulated library (these are host-side paths).  The texts were recorded at commit d344bc8, when each of the four
prover entry points carried its own copy of the checks, with this file, before those were folded into one check per form; the order
of the rows of a form is the order of its checks, and every row breaks one thing in otherwise good arguments, so a refusal that moved
in front of another shows as that other's text."""
import ctypes as C

import numpy as np
import pytest

from tests import emu
from tests.witness_util import random_kv

E_INVALID_ARG, E_UNSORTED, E_UNSUPPORTED = -1, -5, -6

HOST = "keys key_off vals val_off n seg_first n_tries qkeys qkey_off q_trie q_flags n_queries out".split()
DEV = "keys key_off key_bytes vals val_off val_bytes n seg_first n_tries qkeys qkey_off qkey_bytes q_trie q_flags n_queries out".split()
STATE = "addrs nonces balances code code_off slot_keys slot_vals slot_first n wkeys wkey_off wkey_flags n_wkeys out root".split()
# entry point -> (its arguments behind the context, the name in its own texts, the name in its driver's texts)
ENTRY = {"phant_mpt_prove_nodeset": (HOST, "mpt_prove_nodeset", "prove_nodeset"),
         "phant_mpt_prove_batch": ([a for a in HOST if a != "q_flags"], "mpt_prove_batch", "prove_batch"),
         "phant_mpt_prove_nodeset_dev": (DEV, "mpt_prove_nodeset_dev", "prove_nodeset"),
         "phant_mpt_prove_batch_dev": ([a for a in DEV if a != "q_flags"], "mpt_prove_batch_dev", "prove_batch"),
         "phant_state_witness": (STATE, "state_witness", "state_witness"),
         "phant_state_proofs": ([a for a in STATE if a != "wkey_flags"], "state_proofs", "state_proofs")}

TWO_TRIES = {"seg_first": np.array([0, 3, 6], np.uint32), "n_tries": 2, "q_trie": np.array([0, 1, 1], np.uint32)}
u32 = lambda *v: np.array(v, np.uint32)  # noqa: E731
# (what is broken, the code, the text; {name}: the entry point's, {call}: its driver's, {first}: its first-node table's, {d}: "d_" in a device form)
BOTH = [({"out": None}, E_INVALID_ARG, "{name}: out is null"),
        ({"struct_size": 8}, E_INVALID_ARG, "{name}: wrong struct_size"),
        ({"n_tries": 0}, E_INVALID_ARG, "{name}: {d}seg_first is null, or no trie"),
        ({"n_tries": 2}, E_INVALID_ARG, "{name}: {d}seg_first is null, or no trie"),
        ({"key_off": None}, E_INVALID_ARG, "{name}: null pointer"),
        ({"val_off": None}, E_INVALID_ARG, "{name}: null pointer")]
ROWS = {"host": BOTH + [({"qkey_off": None}, E_INVALID_ARG, "{name}: qkey_off is null"),
                        (dict(TWO_TRIES, q_trie=None), E_INVALID_ARG, "{name}: q_trie is null with several tries"),
                        ({"key_off": u32(0, 32, 64, 60, 128, 160, 192)}, E_INVALID_ARG, "offsets not monotone"),
                        ({"key_off": u32(0, 300, 332, 364, 396, 428, 460)}, E_UNSUPPORTED, "key longer than 255 bytes"),
                        (dict(TWO_TRIES, seg_first=u32(0, 7, 6)), E_INVALID_ARG, "seg_first not monotone"),
                        (dict(TWO_TRIES, seg_first=u32(0, 3, 5)), E_INVALID_ARG, "seg_first must span [0, n]"),
                        ({"qkey_off": u32(0, 32, 16, 96)}, E_INVALID_ARG, "query key offsets not monotone"),
                        (dict(TWO_TRIES, q_trie=u32(0, 1, 2)), E_INVALID_ARG, "{call}: q_trie[2] is not below n_tries"),
                        ({"swap_keys": True}, E_UNSORTED, "keys are not strictly increasing (mpt.zig:39)")],
        "dev": BOTH + [({"keys": None}, E_INVALID_ARG, "{name}: null pointer"),
                       ({"vals": None}, E_INVALID_ARG, "{name}: null pointer"),
                       ({"qkey_off": None}, E_INVALID_ARG, "{name}: null query pointer"),
                       ({"qkeys": None}, E_INVALID_ARG, "{name}: null query pointer"),
                       (dict(TWO_TRIES, q_trie=None), E_INVALID_ARG, "{name}: d_q_trie is null with several tries"),
                       ({"misalign": "roots"}, E_INVALID_ARG, "{name}: roots / {first} 4-byte, node_off 8-byte aligned"),
                       ({"misalign": "node_off"}, E_INVALID_ARG, "{name}: roots / {first} 4-byte, node_off 8-byte aligned"),
                       ({"misalign": "first"}, E_INVALID_ARG, "{name}: roots / {first} 4-byte, node_off 8-byte aligned"),
                       (dict(TWO_TRIES, q_trie=u32(0, 1, 2)), E_INVALID_ARG, "{call}: a q_trie index is not below n_tries"),
                       ({"swap_keys": True}, E_UNSORTED, "keys are not strictly increasing (mpt.zig:39)")],
        "state": [({"out": None}, E_INVALID_ARG, "{name}: out / state_root_out is null"),
                  ({"root": None}, E_INVALID_ARG, "{name}: out / state_root_out is null"),
                  ({"addrs": None}, E_INVALID_ARG, "{name}: null pointer"),
                  ({"slot_first": None}, E_INVALID_ARG, "{name}: null pointer"),
                  ({"wkeys": None}, E_INVALID_ARG, "{name}: wkeys / wkey_off is null"),
                  ({"wkey_off": None}, E_INVALID_ARG, "{name}: wkeys / wkey_off is null"),
                  ({"wkey_off": u32(0, 20, 10)}, E_INVALID_ARG, "{name}: wkey_off not monotone"),
                  ({"wkey_off": u32(0, 20, 41)}, E_INVALID_ARG,
                   "{name}: key 1 is 21 bytes: a key is a 20-byte address or a 52-byte address ++ slot")]}


@pytest.fixture(scope="module")
def L():
    try:
        return emu.mirror_lib()
    except RuntimeError as e:
        pytest.skip(str(e))


@pytest.fixture(scope="module")
def ctx(L):
    c = emu.mirror_context(L)
    yield c
    c.close()


def _good(entry):
    """-> good arguments of `entry` by name (numpy arrays, numbers), and the out struct's buffers"""
    from phant_amd import _lib as Lb, mpt
    rng = np.random.default_rng(1)
    if entry.startswith("phant_state"):
        a = {"addrs": rng.integers(0, 256, 40, dtype=np.uint8), "nonces": np.ones(2, np.uint64), "balances": np.ones(64, np.uint8),
             "code": np.zeros(1, np.uint8), "code_off": np.zeros(3, np.uint64), "slot_keys": np.zeros(32, np.uint8),
             "slot_vals": np.zeros(32, np.uint8), "slot_first": np.zeros(3, np.uint32), "n": 2, "wkeys": rng.integers(0, 256, 72, dtype=np.uint8),
             "wkey_off": u32(0, 20, 72), "wkey_flags": np.zeros(2, np.uint8), "n_wkeys": 2, "out": C.c_void_p(), "root": np.zeros(32, np.uint8)}
        return a, None
    keys, vals = random_kv(rng, 6, 32, 1, 40)
    kb, ko = mpt._pack(keys, np.uint32)
    vb, vo = mpt._pack(vals, np.uint64)
    qb, qo = mpt._pack([keys[0], keys[4], bytes(32)], np.uint32)
    a = {"keys": kb, "key_off": ko, "key_bytes": int(ko[-1]), "vals": vb, "val_off": vo, "val_bytes": int(vo[-1]), "n": 6, "seg_first": None,
         "n_tries": 1, "qkeys": qb, "qkey_off": qo, "qkey_bytes": int(qo[-1]), "q_trie": None, "q_flags": None, "n_queries": 3}
    # (one spare element in front of each buffer: `misalign` starts it a byte in)
    buf = {"nodes": np.zeros(1 << 14, np.uint8), "node_off": np.zeros(66, np.uint64), "first": np.zeros(6, np.uint32),
           "roots": np.zeros(96, np.uint8), "q_status": np.zeros(8, np.uint8)}
    a["out"] = (Lb.PhantProveBatchOut if "batch" in entry else Lb.PhantProveOut)
    return a, buf


def _call(L, ctx, entry, broken):
    from phant_amd import _lib as Lb
    order = ENTRY[entry][0]
    a, buf = _good(entry)
    broken = dict(broken)
    if broken.pop("swap_keys", False):
        a["keys"] = np.concatenate([a["keys"][32:64], a["keys"][:32], a["keys"][64:]])  # (the keys are 32 bytes each)
    struct_size, misalign = broken.pop("struct_size", None), broken.pop("misalign", None)
    a.update(broken)
    keep = []
    if buf is not None and a["out"] is not None:
        Out = a["out"]
        ptr = {k: v.ctypes.data + (1 if k == misalign else 0) for k, v in buf.items()}
        o = Out(C.sizeof(Out) if struct_size is None else struct_size, 64, 1 << 13, ptr["nodes"], ptr["node_off"], ptr["first"], ptr["roots"],
                ptr["q_status"], 0, 0, 0)
        keep.append(o)
        a["out"] = C.byref(o)
    elif buf is None and a["out"] is not None:
        out_handle = a["out"]
        a["out"] = C.byref(out_handle)
    p = lambda v: v.ctypes.data_as(C.c_void_p) if isinstance(v, np.ndarray) else v  # noqa: E731
    rc = getattr(L, entry)(ctx.handle, *[p(a[k]) for k in order])
    if buf is None and rc == 0:
        (L.phant_exec_witness_free if entry == "phant_state_witness" else L.phant_witness_free)(out_handle)
    return rc, L.phant_last_error(ctx.handle).decode()


@pytest.mark.parametrize("entry", list(ENTRY))
def test_every_refusal_says_what_it_said(L, ctx, entry):
    _, name, call = ENTRY[entry]
    rows = ROWS["state" if entry.startswith("phant_state") else "dev" if entry.endswith("_dev") else "host"]
    fill = {"name": name, "call": call, "first": "proof_first_node" if "batch" in entry else "trie_first_node", "d": "d_" if entry.endswith("_dev") else ""}
    got = [(_call(L, ctx, entry, broken)) for broken, _, _ in rows]
    want = [(rc, text.format(**fill)) for _, rc, text in rows]
    for row, g, w in zip(rows, got, want):
        print(entry, row[0], g)
    assert got == want
    assert _call(L, ctx, entry, {})[0] == 0  # (the good arguments are good)
