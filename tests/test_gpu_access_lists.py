"""A block's access lists on the device (phant_block_access_lists, phant_block_access_lists_dev, phant_amd.types.transaction.access_lists)
against tests/access_ref.py, which defines every output.  Every comparison is exact, in the host form and in the device form.
tests/test_emu_access_lists.py runs the same bodies over the kernel sources compiled for the host, at the sizes tests/suite.py gives it."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

from tests import access_ref as R
from tests import suite

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG = 0, -1
ALL = tuple(name for name, _, _, _, _ in R.OUTPUTS)
PER_TX = ALL[:4]
UNSET = 0xEEEEEEEE


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def _ctx(P):
    from phant_amd.context import default_context
    return default_context()


def addr(k):
    """address number k: bytes nobody chose"""
    return hashlib.sha256(b"access address" + int(k).to_bytes(8, "big")).digest()[:20]


def key(k):
    return hashlib.sha256(b"access key" + int(k).to_bytes(8, "big")).digest()


def witness(rows):
    """[(address, [slot key, ...]), ...] -> the tables of phant_exec_witness_info as keywords of R.define"""
    first = [0]
    for _, ks in rows:
        first.append(first[-1] + len(ks))
    return dict(addresses=[a for a, _ in rows], slot_first=first, slots=[k for _, ks in rows for k in ks])


# ---------------------------------------------------------------------------------------------------- the raw C-ABI
class Raw:
    """phant_access_in / _out over numpy arrays (host form) or torch tensors on the device (device form)"""
    INPUTS = ("txs", "al_off", "al_len", "addresses", "slot_first", "slots")

    def __init__(self, P, dev, spans, addresses=(), slot_first=None, slots=()):
        import torch
        from phant_amd import _lib as L
        self.L, self.dev, self.torch = L, dev, torch
        self.counts = {"n": len(spans), "n_accounts": len(addresses), "n_slots": len(slots)}
        arrays = R.inputs(spans, addresses, slot_first, slots)
        self.tx_bytes = int(arrays["txs"].size)
        self.arrays = {k: None if a is None else self._up(a) for k, a in arrays.items()}

    def _up(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size == 0:
            a = np.zeros(8, np.uint8)  # (a pointer that is not NULL, to nothing the call may read)
        return self.torch.from_numpy(a.copy()).cuda() if self.dev else a.copy()

    def _ptr(self, x):
        return None if x is None else x.data_ptr() if self.dev else x.ctypes.data

    def _buf(self, nbytes):
        return self.torch.full((nbytes,), 0xEE, dtype=self.torch.uint8).cuda() if self.dev else np.full(nbytes, 0xEE, np.uint8)

    def call(self, ctx, caps, want=None, guard=64, null=(), counts=None, sizes=None, reserved=(0, 0), skew=None, tx_bytes=None):
        """caps: (tuple_cap, key_cap), the rows of the buffers -> (rc, {output: bytes, (output, "guards"): bool}, {total: int}); every
        buffer has `guard` bytes of 0xEE in front of and behind its rows.  null: inputs passed as NULL; counts: counts other than the
        arrays'; skew: {array: bytes its pointer moves up}"""
        L = self.L
        want = ALL if want is None else want
        cnt = dict(self.counts, **(counts or {}))
        rows = {"n": cnt["n"], "n_tuples": caps[0], "n_keys": caps[1]}
        ptr = lambda k: None if k in null or self.arrays[k] is None else self._ptr(self.arrays[k]) + (skew or {}).get(k, 0)  # noqa: E731
        arg = L.PhantAccessIn(C.sizeof(L.PhantAccessIn), cnt["n"], cnt["n_accounts"], cnt["n_slots"], ptr("txs"),
                              self.tx_bytes if tx_bytes is None else tx_bytes, ptr("al_off"), ptr("al_len"), ptr("addresses"), ptr("slot_first"),
                              ptr("slots"), (C.c_uint32 * 2)(*reserved))
        size = {name: np.dtype(dt).itemsize * k * (rows[r] + extra) for name, dt, k, r, extra in R.OUTPUTS if name in want}
        bufs = {k: self._buf(guard + (size[k] + 7) // 8 * 8 + guard) for k in want}
        out = L.PhantAccessOut(C.sizeof(L.PhantAccessOut), UNSET, UNSET, UNSET, UNSET, UNSET, caps[0], caps[1],
                               *[self._ptr(bufs[k]) + guard + (skew or {}).get(k, 0) if k in bufs else None for k in ALL])
        if sizes:
            arg.struct_size, out.struct_size = sizes
        fn = ctx._lib.phant_block_access_lists_dev if self.dev else ctx._lib.phant_block_access_lists
        rc = fn(ctx.handle, C.byref(arg), C.byref(out))
        got = {}
        for k, b in bufs.items():
            if self.dev:
                self.torch.cuda.synchronize()
                b = b.cpu().numpy()
            at = guard + (skew or {}).get(k, 0)
            got[k] = b[at:at + size[k]].tobytes()
            got[k, "guards"] = bool((b[:at] == 0xEE).all() and (b[at + size[k]:] == 0xEE).all())
        return rc, got, {t: int(getattr(out, t)) for t in R.TOTALS}


def _first_difference(name, a, b):
    width = {n: np.dtype(dt).itemsize * k for n, dt, k, _, _ in R.OUTPUTS}[name]
    for i in range(0, max(len(a), len(b)), width):
        if a[i:i + width] != b[i:i + width]:
            return i // width, a[i:i + width].hex(), b[i:i + width].hex()
    return None


def check(P, spans, forms=(False, True), want=None, **tables):
    """every answer of the call against the definition, in both forms, the buffers exactly as large as the totals ask -> the definition's
    (outputs as lists, totals)"""
    exp, totals = R.expected(spans, **tables)
    ctx = _ctx(P)
    for dev in forms:
        rc, got, tot = Raw(P, dev, spans, **tables).call(ctx, (totals["n_tuples"], totals["n_keys"]), want)
        assert rc == OK, (dev, ctx._lib.phant_last_error(ctx.handle))
        assert tot == totals, (dev, tot, totals)
        for k in (k for k in got if isinstance(k, str)):
            assert got[k, "guards"], (dev, k)
            assert got[k] == exp[k], (dev, k, _first_difference(k, got[k], exp[k]))
    return R.define(spans, **tables)


def entries(n_tuples, n_keys, seed=0, accounts=50, keys=40):
    """n_tuples tuples of n_keys keys each, addresses and keys drawn from small pools (some repeat, some the witness of `pool` has)"""
    rng = np.random.default_rng(seed)
    return [(addr(int(rng.integers(0, accounts))), [key(int(rng.integers(0, keys))) for _ in range(n_keys)]) for _ in range(n_tuples)]


def pool(accounts=30, keys=25, per=4, seed=1):
    """a witness with every second address of entries()'s pool and a few of its keys under each"""
    rng = np.random.default_rng(seed)
    return witness([(addr(2 * j), [key(int(x)) for x in rng.integers(0, keys, per)]) for j in range(accounts // 2)])


# ------------------------------------------------------------------------------------------------------------------- the cases
def test_counts_and_empties(P):
    """no transaction at all, a block of legacy transactions only, an empty list, a tuple without keys, one tuple of one key"""
    ctx = _ctx(P)
    for dev in (False, True):
        rc, got, tot = Raw(P, dev, []).call(ctx, (0, 0))
        assert rc == OK and tot == dict.fromkeys(R.TOTALS, 0), (dev, tot)
        assert got["tuple_first"] == got["key_first"] == bytes(4) and all(got[k, "guards"] for k in ALL)
    o, tot = check(P, [b""] * 5, **pool())
    assert tot["n_tuples"] == 0 and o["tuple_first"] == [0] * 6 and tot["first_malformed"] == 5
    o, tot = check(P, [R.encode([(addr(0), [])])], **pool())
    assert (tot["n_tuples"], tot["n_keys"], o["key_first"], o["warm_addresses"], o["warm_keys"]) == (1, 0, [0, 0], [1], [0])
    o, tot = check(P, [R.encode([(addr(0), [key(1)])])], **pool())
    assert (tot["n_tuples"], tot["n_keys"], o["key_first"]) == (1, 1, [0, 1])
    o, tot = check(P, [b"", R.encode([(addr(0), [])]), b"", R.encode([(addr(1), [key(1)]), (addr(2), [])]), b""], **pool())
    assert o["tuple_first"] == [0, 0, 1, 1, 3, 3] and o["key_first"] == [0, 0, 1, 1]


def test_rlp_header_boundaries_of_a_tuple(P):
    """keys per tuple at which a header grows: the tuple's payload is 55 bytes at 1 key (the last short header), the key list's header
    has 2 bytes at 2 keys, 3 at 8, and 4 at 1 986 (1 985: the last with 3)"""
    assert len(R.encode([(addr(0), [key(0)])])) == 1 + 55 and R.encode([(addr(0), [key(0)] * 2)])[:2] == b"\xf8\x59"
    for nk, hdr in ((2, b"\xf8\x42"), (7, b"\xf8\xe7"), (8, b"\xf9\x01\x08"), (1985, b"\xf9\xff\xe1"), (1986, b"\xfa\x01\x00\x02")):
        assert R.rlp_list(b"".join(R.rlp_str(key(0)) for _ in range(nk)))[:len(hdr)] == hdr
    w = pool()
    for nk in (0, 1, 2, 7, 8) + suite.scale((1985, 1986), (1986,)):
        ks = [key(j % 60) for j in range(nk)]
        o, tot = check(P, [R.encode([(addr(1), ks)]), b"", R.encode([(addr(2), [key(3)]), (addr(4), ks), (addr(5), [])])], **w)
        assert tot["n_keys"] == 2 * nk + 1 and o["key_first"] == [0, nk, nk + 1, 2 * nk + 1, 2 * nk + 1] and tot["first_malformed"] == 3


def test_work_distribution(P):
    """many transactions of one tuple, one transaction of many tuples, one tuple of many keys: each time a transaction with an empty
    list between two with lists (an offset carried across rows would show)"""
    w = pool()
    n = suite.scale(300, 130)
    one_each = [R.encode(entries(1, 2, seed=i)) for i in range(n)]
    o, tot = check(P, one_each[:n // 2] + [b""] + one_each[n // 2:], **w)
    assert tot["n_tuples"] == n and tot["n_keys"] == 2 * n and o["tuple_first"][n // 2:n // 2 + 2] == [n // 2] * 2
    many = R.encode(entries(n, 1, seed=7, accounts=10 * n))
    o, tot = check(P, [R.encode(entries(2, 3, seed=8)), b"", many, b"", R.encode(entries(1, 1, seed=9))], **w)
    assert o["tuple_first"] == [0, 2, 2, n + 2, n + 2, n + 3]
    nk = suite.scale(4000, 700)
    big = R.encode([(addr(2), [key(j) for j in range(nk)])])
    o, tot = check(P, [R.encode(entries(3, 2, seed=10)), b"", big, b"", R.encode(entries(2, 2, seed=11))], **w)
    assert tot["n_keys"] == nk + 10 and o["warm_keys"][2] == nk and o["al_flags"][2] == 0


A, B = addr(1), addr(2)
K1, K2 = key(1), key(2)


def tuple_of(address_item, keys_payload, tail=b""):
    return R.rlp_list(address_item + R.rlp_list(keys_payload) + tail)


MALFORMED_SPANS = {
    "a 19-byte address": tuple_of(R.rlp_str(A[:19]), R.rlp_str(K1)),
    "a 21-byte address": tuple_of(R.rlp_str(A + b"\x01"), R.rlp_str(K1)),
    "a 31-byte key": tuple_of(R.rlp_str(A), R.rlp_str(K1[:31])),
    "a 33-byte key": tuple_of(R.rlp_str(A), R.rlp_str(K1 + b"\x01")),
    "a 31-byte and a 33-byte key, 66 bytes together": tuple_of(R.rlp_str(A), R.rlp_str(K1[:31]) + R.rlp_str(K1 + b"\x01")),
    "a key that is a list": tuple_of(R.rlp_str(A), R.rlp_str(K1) + R.rlp_list(bytes(32))),
    "a byte behind the keys": tuple_of(R.rlp_str(A), R.rlp_str(K1), tail=b"\x01"),
    "a tuple one byte longer than the span": (lambda t: bytes([t[0], t[1] + 1]) + t[2:])(tuple_of(R.rlp_str(A), R.rlp_str(K1) + R.rlp_str(K2))),
    "a long header where the short one would do": b"\xf8\x37" + tuple_of(R.rlp_str(A), R.rlp_str(K1))[1:],
    "an address that is a list": tuple_of(R.rlp_list(bytes(20)), R.rlp_str(K1)),
    "keys that are a string": R.rlp_list(R.rlp_str(A) + R.rlp_str(K1 + b"\x00")),
    "a good tuple, then a cut one": R.encode([(A, [K1])]) + tuple_of(R.rlp_str(B), R.rlp_str(K2))[:-1],
    "a bad key in the last of three tuples": R.encode([(A, [K1, K2]), (B, [])]) + tuple_of(R.rlp_str(B), R.rlp_str(K1) + b"\xa1" + K2),
}


def test_malformed_spans(P):
    """each malformed span is flagged and contributes nothing, the rows before and after keep their exact entries; first_malformed is
    the least flagged row.  The spans are built by hand: the transactions call would refuse such a transaction, this call has to be
    safe on its own"""
    w = witness([(A, [K1]), (B, [K2, K1])])
    good = [R.encode([(A, [K1, K2]), (B, [])]), R.encode([(B, [K2])])]
    assert all(R.walk(s) is None for s in MALFORMED_SPANS.values()) and all(R.walk(s) is not None for s in good)
    for name, span in MALFORMED_SPANS.items():
        o, tot = check(P, [good[0], span, good[1]], **w)
        assert o["al_flags"] == [0, R.MALFORMED, 0] and tot["first_malformed"] == 1 and o["tuple_first"] == [0, 2, 2, 3], name
        assert (o["warm_addresses"], o["warm_keys"], tot["n_keys"], o["slot_row"]) == ([2, 0, 1], [2, 0, 1], 3, [0, R.NONE, 1]), name
    # all of them in one block between good rows of several tuples, flagged by the walk and by the key lanes alike
    spans = []
    for i, span in enumerate(MALFORMED_SPANS.values()):
        spans += [R.encode(entries(1 + i % 3, i % 4, seed=i)), span]
    o, tot = check(P, spans + [good[0]], **w)
    assert o["al_flags"][1::2] == [R.MALFORMED] * len(MALFORMED_SPANS) and tot["first_malformed"] == 1
    o, tot = check(P, [good[0], good[1]] + list(MALFORMED_SPANS.values())[4:6], **w)
    assert tot["first_malformed"] == 2


def test_joins(P):
    """addresses the witness has, lacks and has twice (the lowest row wins); a key the witness has under ANOTHER account; a key under an
    address the witness lacks; the same key under two accounts; no table, a table of one row; an account without slots"""
    a, b, c, d, x = (addr(k) for k in range(5))
    w = witness([(a, [K1, K2]), (b, []), (c, [K2, K1, K2]), (a, [key(3)]), (d, [K1])])
    spans = [R.encode([(a, [K1, key(3)]), (x, [K1]), (b, [K1]), (c, [K2, K1]), (d, [K2, K1])]), R.encode([(c, [key(9)]), (a, [K2])])]
    o, tot = check(P, spans, **w)
    assert o["account_row"] == [0, R.NONE, 1, 2, 4, 2, 0]
    assert o["slot_row"] == [0, R.NONE, R.NONE, R.NONE, 2, 3, R.NONE, 6, R.NONE, 1]  # (key(3) lies under row 3, not under a's row 0)
    assert (tot["n_missing_accounts"], tot["n_missing_slots"]) == (1, 5)
    o, tot = check(P, spans)
    assert set(o["account_row"]) == set(o["slot_row"]) == {R.NONE} and (tot["n_missing_accounts"], tot["n_missing_slots"]) == (7, 10)
    o, tot = check(P, spans, **witness([(c, [K1])]))
    assert o["account_row"] == [R.NONE, R.NONE, R.NONE, 0, R.NONE, 0, R.NONE] and o["slot_row"][4:6] == [R.NONE, 0]
    check(P, spans, **witness([(c, [])]))
    # a table in which every row is the same address: the first row's slots alone count
    o, tot = check(P, spans, **witness([(c, [K1])] + [(c, [K2])] * suite.scale(300, 70)))
    assert o["slot_row"][4:6] == [R.NONE, 0]


def test_duplicates(P):
    """an address repeated in one transaction, next to itself and apart; repeated across transactions (no duplicate); a pair repeated
    within a tuple and across two tuples of one address; the warm counts, the flag, the missing counts over first occurrences"""
    a, b, x = addr(0), addr(1), addr(2)
    w = witness([(a, [K1]), (b, [])])
    spans = [R.encode([(a, [K1, K2, K1]), (a, [K2, key(3)]), (b, [K1]), (x, [K1]), (a, []), (x, [K1, K2])]),
             R.encode([(a, [K1]), (b, [K1])]), R.encode([(x, [])]), R.encode([(b, [K2, K2])])]
    o, tot = check(P, spans, **w)
    assert o["tuple_same"] == [0, 0, 2, 3, 0, 3, 6, 7, 8, 9]
    assert o["key_same"] == [0, 1, 0, 1, 4, 5, 6, 6, 8, 9, 10, 11, 11]
    assert o["al_flags"] == [R.DUPLICATES, 0, 0, R.DUPLICATES] and o["warm_addresses"] == [3, 2, 1, 1] and o["warm_keys"] == [6, 2, 0, 1]
    assert (tot["n_missing_accounts"], tot["n_missing_slots"]) == (2, 7)
    # many repeats of few addresses and keys in one transaction, more than a wave of them
    n = suite.scale(500, 150)
    o, tot = check(P, [R.encode(entries(n, 3, seed=3, accounts=7, keys=5)), R.encode(entries(n // 2, 2, seed=4, accounts=7, keys=5))], **pool())
    assert o["warm_addresses"] == [7, 7] and max(o["warm_keys"]) <= 35 and o["al_flags"] == [R.DUPLICATES] * 2


def test_every_subset_of_outputs(P):
    """every subset of the output pointers on one small block: the span the host form fetches ends at every position.  (The device
    form copies every output by itself, and the emulated run is slow: none, all, each alone, each left out.)"""
    w = pool()
    spans = [R.encode(entries(3, 2, seed=1)), b"", MALFORMED_SPANS["a key that is a list"], R.encode(entries(2, 0, seed=2)), R.encode(entries(4, 3, seed=3))]
    exp, totals = R.expected(spans, **w)
    some = [(), ALL] + [(k,) for k in ALL] + [tuple(x for x in ALL if x != k) for k in ALL]
    every = suite.scale([c for r in range(len(ALL) + 1) for c in itertools.combinations(ALL, r)], some)
    ctx = _ctx(P)
    for dev in (False, True):
        raw = Raw(P, dev, spans, **w)
        for want in (some if dev else every):
            rc, got, tot = raw.call(ctx, (totals["n_tuples"], totals["n_keys"]), want, guard=8)
            assert rc == OK and tot == totals, (dev, want)
            for k in want:
                assert got[k, "guards"] and got[k] == exp[k], (dev, want, k)


def test_capacities_one_short(P):
    """a capacity one short, for tuples and for keys: the totals and the per-transaction outputs are written, no per-tuple or per-key
    buffer is touched; the second call with what the totals ask succeeds.  A buffer nobody wants has no capacity to exceed"""
    w = pool()
    spans = [R.encode(entries(3, 2, seed=1)), b"", R.encode(entries(4, 3, seed=3))]
    exp, totals = R.expected(spans, **w)
    nt, nk = totals["n_tuples"], totals["n_keys"]
    ctx = _ctx(P)
    for dev in (False, True):
        raw = Raw(P, dev, spans, **w)
        for caps in ((nt - 1, nk), (nt, nk - 1), (0, 0)):
            rc, got, tot = raw.call(ctx, caps)
            assert rc == OK and tot == totals, (dev, caps)
            for k in ALL:
                assert got[k, "guards"], (dev, caps, k)
                if k in PER_TX:
                    assert got[k] == exp[k], (dev, caps, k)
                else:
                    assert set(got[k]) <= {0xEE}, (dev, caps, k)
            rc, got, tot = raw.call(ctx, (tot["n_tuples"], tot["n_keys"]))
            assert rc == OK and all(got[k] == exp[k] for k in ALL), (dev, caps)
        rc, got, tot = raw.call(ctx, (0, nk), want=PER_TX + ("key", "slot_row", "key_same"))  # nobody wants a per-tuple buffer
        assert rc == OK and got["key"] == exp["key"] and got["slot_row"] == exp["slot_row"], dev
        rc, got, tot = raw.call(ctx, (nt, 0), want=("address", "key_first", "account_row"))
        assert rc == OK and got["address"] == exp["address"] and got["key_first"] == exp["key_first"], dev


def test_one_context_small_large_small(P):
    """one context through a small, a large and the same small block again, in both forms: the arena grows and is carved anew"""
    w = pool()
    small = [R.encode(entries(2, 2, seed=5)), b"", R.encode(entries(1, 4, seed=6))]
    n = suite.scale(1500, 90)
    large = [R.encode(entries(1 + i % 5, i % 7, seed=100 + i, accounts=400, keys=40)) if i % 9 else b"" for i in range(n)]
    first, _ = check(P, small, **w)
    o, tot = check(P, large, **pool(accounts=400, keys=40, per=6))
    assert tot["n_keys"] > 2 * n and len(set(o["slot_row"])) > 10 and any(f & R.DUPLICATES for f in o["al_flags"])
    again, _ = check(P, small, **w)
    assert again == first


def test_refused_arguments(P):
    """one refusal per rule of the header, in both forms; nothing is written.  (The emulated module runs them before any GPU does: a
    lying span that got past the check would be a fault there, not a failed assertion.)"""
    w = pool()
    spans = [R.encode(entries(3, 2, seed=1)), b"", R.encode(entries(4, 3, seed=3))]
    _, totals = R.expected(spans, **w)
    caps = (totals["n_tuples"], totals["n_keys"])
    ctx = _ctx(P)

    def refused(dev, tables=w, **kw):
        rc, got, tot = Raw(P, dev, spans, **tables).call(ctx, caps, **kw)
        assert rc == E_INVALID_ARG, (dev, kw, rc)
        assert all(set(got[k]) <= {0xEE} for k in ALL) and tot == dict.fromkeys(R.TOTALS, UNSET), (dev, kw)
        assert ctx._lib.phant_last_error(ctx.handle)

    for dev in (False, True):
        probe = Raw(P, dev, spans, **w)
        last = int(R.inputs(spans)["al_off"][-1]) + len(spans[-1])
        refused(dev, sizes=(8, C.sizeof(probe.L.PhantAccessOut)))                  # a wrong struct_size, either struct
        refused(dev, sizes=(C.sizeof(probe.L.PhantAccessIn), 8))
        refused(dev, reserved=(1, 0))
        refused(dev, reserved=(0, 1))
        for name in Raw.INPUTS:
            refused(dev, null=(name,))                                           # a NULL input whose count is not zero
        refused(dev, tx_bytes=last - 1)                                          # a span that ends behind tx_bytes
        refused(dev, tx_bytes=int(R.inputs(spans)["al_off"][-1]) - 1)            # ... that begins behind it
        refused(dev, tx_bytes=0)
        first = list(w["slot_first"])
        refused(dev, dict(w, slot_first=[1] + first[1:]))                        # slot_first does not begin at 0
        refused(dev, dict(w, slot_first=first[:-1] + [first[-1] - 1]))           # ... does not end at n_slots
        refused(dev, dict(w, slot_first=first[:-1] + [first[-1] + 1]))
        refused(dev, dict(w, slot_first=first[:3] + [first[2] - 1] + first[4:]))  # ... goes backwards
        refused(dev, dict(w, slot_first=first[:3] + [first[-1] + 5] + first[4:]))  # ... beyond n_slots in the middle
        # ... and no refusal where the count is zero
        rc, _, _ = Raw(P, dev, spans).call(ctx, caps, null=("addresses", "slot_first", "slots"))
        assert rc == OK
        rc, _, tot = Raw(P, dev, [b"", b""], **w).call(ctx, (0, 0), null=("txs",), tx_bytes=0)
        assert rc == OK and tot["n_tuples"] == 0
    refused(True, skew={"al_off": 4})                                            # device form: a misaligned array
    refused(True, skew={"slot_row": 2})


def test_end_to_end_from_raw_transactions(P, oracle):
    """raw type-1, type-2 and type-4 transactions with access lists (and a legacy one, and one the decode refuses) ->
    block_transactions(fork=FORK_PRAGUE) -> access_lists with the spans it returned -> against the definition; the sums of al_addresses
    and al_keys over the decodable rows are the call's totals"""
    from phant_amd.types import transaction as TX
    from tests import tx_ref_forks as F
    w = pool()
    lists = [entries(2, 3, seed=1), [], entries(1, 0, seed=2), entries(5, 2, seed=3) + entries(1, 2, seed=3), entries(3, 1, seed=4)]
    raws = [F.make_tx(oracle, 11, 1, 1, access_list=lists[0], nonce=0), F.make_tx(oracle, 12, 0, 1), F.make_tx(oracle, 13, 2, 1, access_list=lists[2]),
            F.make_tx(oracle, 14, 4, 1, access_list=lists[3]), b"\x01\xc0", F.make_tx(oracle, 15, 2, 1, access_list=lists[4], nonce=3)]
    bt = TX.block_transactions(raws, 1, fork=TX.FORK_PRAGUE)
    decodable = [i for i in range(bt.n) if not int(bt.flags[i]) & 1]
    assert decodable == [0, 1, 2, 3, 5]
    spans = [bt.access_list(i).tobytes() for i in range(bt.n)]
    info = {"n_accounts": len(w["addresses"]), "n_slots": len(w["slots"]), "addresses": np.frombuffer(b"".join(w["addresses"]), np.uint8),
            "slot_first": np.asarray(w["slot_first"], np.uint32), "slots": np.frombuffer(b"".join(w["slots"]), np.uint8)}
    r = TX.access_lists(bt, info)
    o, totals = R.define(spans, **w)
    assert r.lists == [lists[0], [], lists[2], lists[3], [], lists[4]]
    assert (r.n_tuples, r.n_keys) == (totals["n_tuples"], totals["n_keys"]) == (int(bt.al_addresses[decodable].sum()), int(bt.al_keys[decodable].sum()))
    assert (r.n_missing_accounts, r.n_missing_slots, r.first_malformed) == (totals["n_missing_accounts"], totals["n_missing_slots"], bt.n)
    for name in ALL:
        assert getattr(r, name).reshape(-1).tolist() == (list(b"".join(o[name])) if name in ("address", "key") else o[name]), name
    assert any(f & r.DUPLICATES for f in r.al_flags.tolist()) and not any(r.malformed(i) for i in range(r.n))
    none = TX.access_lists({"blob": bt.blob, "al_off": bt.al_off, "al_len": bt.al_len})
    assert none.lists == r.lists and set(none.account_row.tolist()) == {R.NONE}
