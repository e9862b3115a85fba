"""The trie hasher's launch-time choices (stated in phant_amd/csrc/trie_plan.h: resolve_choices, small_pass, leaves_ahead, side_ok,
plan_bin; launched by phant_amd/csrc/trie_build.hip: general_forest's stages, launch_bin), each FORCED on the GPU over
tries chosen for it, against the oracle -- and, through Context.trie_stats() (phant_trie_stats), the proof that the call took
the path the case names: the pass, whether the leaves went ahead, the depth from which the bins ran on the helper stream, the
bins per kernel class, the nodes on the fallback lists, whether the kernel for 136 .. 543-byte leaves ran.

What a call SHOULD have chosen is worked out here, from the keys alone, by `plan` and `expect` below: the branch nodes of a trie
are the LCP-intervals of its sorted keys, a node's depth is the interval's LCP, and the launcher's rules are restated from its
documentation (a wave per node up to 2 048 nodes of a bin, a node per half wave up to 4 096, a lane per node beyond; the helper
stream from the shallowest bin on when that is not depth 0, there are two bins and no leaf can reach a rate block; the small
pass up to 2 048 keys, up to 4 096 where the mean value is a rate block).  The numbers are written out again, not imported.

tests/test_emu_trie_choices.py runs the same bodies over the emulated library at the sizes tests/suite.py gives emulated runs."""
import threading
from contextlib import contextmanager

import numpy as np
import pytest

from tests import suite
from tests.witness_util import _rlp_list, _rlp_str

pytestmark = pytest.mark.gpu

RATE = 136

# ---- the settings (include/phant_gpu_diag.h); every one has trie_small_max_keys = 0 unless it says otherwise ----
SIDE_LDS_MAX = 65536 - 4 * 256 * 35  # what a launch may add to a leaf workgroup's 35 840 bytes of static LDS
SETTINGS = {
    "default": {},
    "blocks1": {"trie_slot_blocks": 1},
    "blocks1_grid1": {"trie_slot_blocks": 1, "trie_fallback_grid": 1},
    "blocks2": {"trie_slot_blocks": 2},
    "blocks2_grid1": {"trie_slot_blocks": 2, "trie_fallback_grid": 1},
    "blocks4": {"trie_slot_blocks": 4},
    "blocks4_grid1": {"trie_slot_blocks": 4, "trie_fallback_grid": 1},
    "no_coop": {"trie_no_coop": 1},
    "no_wave": {"trie_no_wave": 1},
    "coop_max0": {"trie_coop_max": 0},
    "side": {"trie_side_min_keys": 0},
    "side_behind": {"trie_side_min_keys": 0, "trie_ahead_max_keys": 0},
    "side_join": {"trie_side_min_keys": 0, "trie_join_in_stream": 1},
    "side_lds0": {"trie_side_min_keys": 0, "trie_side_lds": 0},
    "side_ldsmax": {"trie_side_min_keys": 0, "trie_side_lds": SIDE_LDS_MAX},
    "side_blocks1_grid1": {"trie_side_min_keys": 0, "trie_slot_blocks": 1, "trie_fallback_grid": 1},  # a misfit list on the helper stream
    "small": {"trie_small_max_keys": -1},
}
KNOB_DEFAULTS = {"trie_small_max_keys": -1, "trie_slot_blocks": 0, "trie_fallback_grid": -1, "trie_no_coop": 0, "trie_no_wave": 0,
                 "trie_coop_max": -1, "trie_side_min_keys": -1, "trie_ahead_max_keys": -1, "trie_join_in_stream": 0, "trie_side_lds": -1}
# the emulated run of a shape's matrix: one setting of every kind (the lockstep emulator pays ~10 000 x for every node)
EMULATED_SETTINGS = ("default", "blocks1_grid1", "blocks2", "no_coop", "no_wave", "side", "side_behind", "side_join",
                     "side_blocks1_grid1", "small")


def knobs_of(setting):
    return dict({"trie_small_max_keys": 0}, **(SETTINGS[setting] if isinstance(setting, str) else setting))


@contextmanager
def forced(ctx, setting):
    knobs = knobs_of(setting)
    try:
        for k, v in knobs.items():
            ctx.diag_set(k, v)
        yield knobs
    finally:
        for k, v in KNOB_DEFAULTS.items():
            ctx.diag_set(k, v)


def settings_for_matrix():
    return [s for s in SETTINGS if not suite.EMULATED or suite.FULL or s in EMULATED_SETTINGS]


@pytest.fixture(scope="module")
def P():
    import phant_amd
    return phant_amd


def new_context(P):
    """A Context of the test's own (the emulated library's under tests/test_emu_trie_choices.py)."""
    if suite.EMULATED:
        from tests import emu
        return emu.mirror_context(emu.mirror_lib())
    return P.Context(0)


@pytest.fixture(scope="module")
def ctx(P):
    c = new_context(P)
    yield c
    c.close()


# ---- what a call should have chosen, from the keys ----
def _nibbles(k):
    return [x for b in k for x in (b >> 4, b & 15)]


def _lcp(a, b):
    na, nb = _nibbles(a), _nibbles(b)
    m = 0
    while m < len(na) and m < len(nb) and na[m] == nb[m]:
        m += 1
    return m


def plan(keys, vals, seg=None):
    """-> nodes per depth {depth: count} of the forest (trie t = keys seg[t] .. seg[t + 1]) and whether some leaf may reach a rate
    block (key bytes + value bytes + 9 >= 136: identify_kernel's test for launching leaf_big_kernel and against the helper stream)."""
    seg = seg or [0, len(keys)]
    hist = {}
    for a, b in zip(seg, seg[1:]):
        stack = []
        for i in range(a + 1, b):
            v = _lcp(keys[i - 1], keys[i])
            while stack and stack[-1] > v:
                d = stack.pop()
                hist[d] = hist.get(d, 0) + 1
            if not stack or stack[-1] < v:
                stack.append(v)
        for d in stack:
            hist[d] = hist.get(d, 0) + 1
    return {"hist": hist, "n": len(keys), "val_bytes": sum(len(v) for v in vals),
            "maybe_big": any(len(k) + len(v) + 9 >= RATE for k, v in zip(keys, vals))}


def _class_of(c, knobs):
    coop_max = knobs.get("trie_coop_max", -1)
    coop_max = 4096 if coop_max < 0 else coop_max
    forced_blocks = knobs.get("trie_slot_blocks", 0)
    if c <= coop_max and not knobs.get("trie_no_coop") and not forced_blocks:
        return "wave" if c <= 2048 and not knobs.get("trie_no_wave") else "half_wave"
    return "blocks%d" % (forced_blocks or 4)


def expect(pl, knobs):
    """the part of trie_stats() that follows from the trie and the knobs alone"""
    n, hist = pl["n"], pl["hist"]
    small_max = knobs.get("trie_small_max_keys", -1)
    small = n <= 4096 and (n <= small_max if small_max >= 0 else (n <= 2048 or pl["val_bytes"] >= RATE * n))
    if small:
        return {"pass": "small", "n": n}
    want = {"pass": "general", "n": n, "leaves_ahead": knobs.get("trie_ahead_max_keys", -1) != 0, "bins": len(hist),
            "max_bin": max(hist.values(), default=0), "n_rep": sum(hist.values()), "leaf_big": pl["maybe_big"],
            "wave": 0, "half_wave": 0, "blocks1": 0, "blocks2": 0, "blocks4": 0}
    for c in hist.values():
        want[_class_of(c, knobs)] += 1
    side = knobs.get("trie_side_min_keys", -1) == 0 and not pl["maybe_big"] and len(hist) >= 2 and min(hist) > 0
    want["deep_from"] = min(hist) if side else -1
    want["side_bins"] = len(hist) if side else 0
    return want


def check_stats(got, want, what):
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"{what}: trie_stats() (got, expected) {bad}"


# ---- the shapes: deterministic, built once, the oracle's root beside them ----
class Shape:
    def __init__(self, P, oracle, keys, vals):
        order = sorted(range(len(keys)), key=lambda i: keys[i])
        self.keys, self.vals = [keys[i] for i in order], [vals[i] for i in order]
        assert all(a < b for a, b in zip(self.keys, self.keys[1:]))
        self.kb, self.ko = P.mpt._pack(self.keys, np.uint32)
        self.vb, self.vo = P.mpt._pack(self.vals, np.uint64)
        self.root = oracle.mptize_packed(self.kb, self.ko, self.vb, self.vo)
        self.plan = plan(self.keys, self.vals)

    def run(self, P, ctx):
        return P.mpt.mptize_packed(self.kb, self.ko, self.vb, self.vo, ctx=ctx)


def _bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


BRANCH_VALUE_LENS = (1, 5, 6, 7, 8, 9, 31, 32, 55, 56, 57, 135, 136, 200, 600)


def value_branches(rng):
    """BranchPlan::staged (trie_build.hip: `p.payload < BRANCH_STAGE_BYTES - 8u`): sixteen hashed children are 528 bytes, so a
    branch value of up to 6 bytes (7 encoded) still builds in the lane's four-block LDS slot and one of 7 goes to the scratch
    blob; from 136 bytes the node no longer fits four rate blocks at all.  The value-carrying branches alternate with plain full
    ones at ONE depth: branch_kernel<4>'s register path (`p.full`, cleared by a value) must leave a wave alone that holds one
    of them, and branch_coop_kernel's `plain` sends both halves of a wave the general way when either has a value."""
    keys, vals = [], []
    for j in range(suite.scale(120, 32)):  # (1 980 keys: the small pass takes up to 2 048 whatever the values)
        if j % 2 == 0:
            keys.append(bytes([j]))
            vals.append(_bytes(rng, BRANCH_VALUE_LENS[(j // 2) % len(BRANCH_VALUE_LENS)]))
        for x in range(16):
            keys.append(bytes([j, x << 4]))
            vals.append(_bytes(rng, 40))
    return keys, vals


def full_waves(rng):
    """branch_kernel<4>'s ballot for the register-only path (`__ballot(p.live && !fast) == 0`): every level of this trie is full
    branches of sixteen hashed children -- 256 of them at depth 2, four waves of the lane-per-node kernel -- but for ONE node of
    two children, so that one wave hashes from registers next to one that may not.  The root is a full branch too: the path takes
    it unless its bytes are wanted (phant_mpt_root_nodes)."""
    keys = [bytes([a, z << 4]) for a in range(suite.scale(256, 80)) for z in range(16) if a != 0x2a or z in (3, 12)]
    return keys, [_bytes(rng, 40) for _ in keys]


def _embedded(rng, first):
    keys = set()
    alphabet = (0x00, 0x01, 0x10, 0x17, 0x70, 0x71, 0x77)
    while len(keys) < suite.scale(240, 120):
        k = bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), int(rng.integers(1, 4))))
        keys.add(first + k if first else k)
    # ... and under every first byte a pair that parts in its last nibble only: two embedded leaves in a branch of ~22 bytes, which
    # sits inside the extension (nibbles 5, a, 5) above it -- nibble 5 is none of the alphabet's, so nothing else shares that path
    for a in alphabet:
        keys |= {first + bytes([a, 0x5a, 0x50 | x]) for x in (0, 1)}
    keys = sorted(keys)
    return keys, [bytes([int(rng.integers(1, 256))]) for _ in keys]


def embedded(rng):
    """put_branch's embedded children and fits_slot<1|2> (`p.ext_len == 0u || p.total >= 32u`): keys of 1 to 3 bytes over seven
    byte values with 1-byte values -- keys that are prefixes of others (branch values), leaves and branches shorter than 32
    bytes that sit inside their parents, extensions over embedded branches (misfits of the one- and two-block classes)."""
    return _embedded(rng, b"")


def embedded_under_extension(rng):
    """... the same under a common first byte: the root is an extension, every bin lies below depth 0 (the helper stream can run)."""
    return _embedded(rng, b"\x3c")


def embedded_root(rng):
    """branch_emit's root rule (a root shorter than 32 bytes is hashed all the same, mpt.zig:42): two keys, an extension over a
    branch of two embedded leaves -- some twenty bytes."""
    return [b"\x10", b"\x11"], [b"a", b"b"]


LONG_EXT_SHARED = (1, 100, 226, 227, 228, 229, 250)


def long_extensions(rng):
    """BranchPlan::ext_cap (`40 + ext_len / 2 + 4 < 2 * RATE` for `staged`: it changes between 227 and 228 shared bytes;
    fits_slot<1|2> well below): pairs of 255-byte keys that share 1 .. 250 bytes and part in a high nibble (an even depth) or a
    low one (odd)."""
    keys = []
    for p, s in enumerate(LONG_EXT_SHARED):
        for low in (0, 1):
            a = bytearray(_bytes(rng, 255))
            a[0] = 0x10 * p + 8 * low + 1
            b = bytearray(a)
            b[s:] = _bytes(rng, 255 - s)
            a[s], b[s] = (0x20, 0x21) if low else (0x20, 0x90)
            keys += [bytes(a), bytes(b)]
    return keys, [_bytes(rng, rng.integers(1, 41)) for _ in keys]


def mixed_fanout(rng):
    """branch_kernel<1|2>'s misfit list and the fallback pass's grid-stride loop (`first += gridDim.x * LANES`): prefixes of three
    nibbles with 2 .. 16 hashed children each in a fixed pattern -- one bin of several hundred nodes of which only those of up to
    3 (7) children fit a one-(two-)block slot; with trie_fallback_grid = 1 one workgroup of 64 lanes takes the rest in turns."""
    keys = []
    for i in range(suite.scale(720, 136)):
        for c in range(2 + (i * 7) % 15):
            keys.append(bytes([i >> 4, ((i & 15) << 4) | c]) + _bytes(rng, 30))
    return keys, [_bytes(rng, 33) for _ in keys]


def exact_bin(c):
    def build(rng):
        keys = [bytes([i >> 8, i & 255, x]) for i in range(c) for x in (0x00, 0x80)]
        return keys, [_bytes(rng, 33) for _ in keys]
    build.__doc__ = f"""launch_bin's thresholds: {c} prefixes of four nibbles with two leaves each are exactly {c} nodes at depth 4."""
    return build


def _clusters(rng, big_leaf):
    n = suite.scale(400, 150)
    keys = {b"\xc4" + _bytes(rng, 31) for _ in range(n)}
    for shared in range(6, 12):
        stem = b"\xc4" + _bytes(rng, shared - 1)
        keys |= {stem + _bytes(rng, 32 - shared) for _ in range(12)}
    keys = sorted(keys)
    vals = [_bytes(rng, rng.integers(1, 95 if not big_leaf else 131)) for _ in keys]
    if big_leaf:
        vals[len(vals) // 2] = _bytes(rng, 200)
    return keys, vals


def deep_clusters(rng):
    """order_kernel's list of the leaves under the deepest bins (`t.deep_leaves`) and leaf_kernel's two launches: six clusters of a
    dozen keys that share 6 .. 11 bytes, scattered among a few hundred random 32-byte keys; every value below 95 bytes, so no leaf
    can reach a rate block (counters[3] == 0).  order_kernel never gives the helper stream the bin of depth 0 (`s_from > 0`), and
    in a trie this small no bin breaks the run from below: the keys share their first byte, the root is an extension, and every
    bin runs beside the leaves."""
    return _clusters(rng, False)


def deep_clusters_big_leaf(rng):
    """... and with values of up to 130 bytes and one of 200: identify_kernel raises counters[3], order_kernel then refuses the
    helper stream (`t.counters[3] == 0u`) and the launcher adds leaf_big_kernel."""
    return _clusters(rng, True)


LEAF_TOTALS = (135, 136, 137, 543, 544, 545, 2000, 5000)


def leaf_sizes(rng):
    """leaf_kernel (`p.total < RATE`), leaf_big_kernel (`p.total >= RATE && p.total < LEAF_BIG_MAX`) and the scratch path beyond:
    sixteen 32-byte keys under sixteen first nibbles; eight values sized so that the ENCODED leaf -- list header, the hex-prefix
    string of the key's remaining 63 nibbles, the value string -- is 135, 136, 137, 543, 544, 545, 2 000 and 5 000 bytes."""
    keys = [bytes([(x << 4) | x]) + _bytes(rng, 31) for x in range(16)]
    vals = []
    for x, k in enumerate(keys):
        if x % 2:
            vals.append(_bytes(rng, 20 + x))
            continue
        rest = 2 * len(k) - 1  # (the root branch at depth 0 takes one nibble)
        hp = bytes([0x30 | _nibbles(k)[1]]) + k[1:] if rest % 2 else b"\x20" + k[1:]
        want = LEAF_TOTALS[x // 2]
        v = next(n for n in range(1, want) if len(_rlp_list([_rlp_str(hp), _rlp_str(b"\xff" * n)])) == want)
        vals.append(b"\xff" + _bytes(rng, v - 1))
    return keys, vals


def nested_chains(rng):
    """small_climb_kernel's hand-off (`atomicAdd(&t.order2[node], 1u)` between two `__threadfence()`): ~100 spines of 20 .. 60 nested
    two-child nodes on consecutive depths -- a node's other child is a leaf a key order away, hashed by another workgroup, and the
    wave that brings the last child climbs on."""
    keys, first = set(), 0
    total = suite.scale(4000, 240)
    while len(keys) < total:
        spine = bytearray(_bytes(rng, 32))
        spine[0] = first
        first += 1
        keys.add(bytes(spine))
        for j in range(2, 2 + min(int(rng.integers(20, 61)), total - len(keys))):
            k = bytearray(spine)
            k[j // 2] ^= 0x80 >> (4 * (j & 1))
            k[j // 2 + 1:] = _bytes(rng, 31 - j // 2)
            keys.add(bytes(k))
    keys = sorted(keys)[:total]
    return keys, [_bytes(rng, rng.integers(1, 60)) for _ in keys]


def last_two_bytes(rng):
    """... and keys that differ in their last two bytes only: one extension of 60 nibbles over four levels of branches without
    values, every node's children spread over the whole grid."""
    n = suite.scale(4096, 256)
    stem = _bytes(rng, 30)
    tails = sorted(int(x) for x in rng.choice(65536, n, replace=False))
    return [stem + bytes([t >> 8, t & 255]) for t in tails], [_bytes(rng, rng.integers(1, 60)) for _ in tails]


EXACT_BINS = (1, 2, 3, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
EXACT_BINS_EMULATED = (512, 513, 1024, 1025, 2048, 2049)
BUILDERS = {f.__name__: f for f in (value_branches, full_waves, embedded, embedded_under_extension, embedded_root, long_extensions,
                                    mixed_fanout, deep_clusters, deep_clusters_big_leaf, leaf_sizes, nested_chains, last_two_bytes)}
BUILDERS.update({f"exact_bin_{c}": exact_bin(c) for c in EXACT_BINS})
_built = {}


def shape(P, oracle, name):
    key = (name, suite.EMULATED, suite.FULL)
    if key not in _built:
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
        _built[key] = Shape(P, oracle, *BUILDERS[name](np.random.default_rng(seed)))
    return _built[key]


def run_checked(P, ctx, sh, setting, what):
    with forced(ctx, setting) as knobs:
        got = sh.run(P, ctx)
        st = ctx.trie_stats()
    assert got == sh.root, f"{what}: root differs from the oracle's"
    check_stats(st, expect(sh.plan, knobs), what)
    return st


# ---- every shape under every setting ----
MATRIX_SHAPES = ("value_branches", "full_waves", "embedded", "embedded_under_extension", "embedded_root", "long_extensions",
                 "mixed_fanout", "deep_clusters", "deep_clusters_big_leaf", "leaf_sizes")


@pytest.mark.parametrize("name", MATRIX_SHAPES)
def test_shape_under_every_setting(P, oracle, ctx, name):
    """Every shape above under every setting of the table: the oracle's root, and the statistics `expect` derives from the keys."""
    sh = shape(P, oracle, name)
    for setting in settings_for_matrix():
        run_checked(P, ctx, sh, setting, f"{name} under {setting}")


def test_the_shapes_reach_what_they_aim_at(P, oracle, ctx):
    """What `expect` cannot say because it depends on the nodes' sizes, and what the shapes were made for: the fallback lists really
    fill, the helper stream really runs (a trie whose bins start at depth 0 would pass every root comparison with the knob set and
    nothing forced), and leaf_big_kernel runs where a leaf needs it."""
    # full branches never fit one or two blocks: all of them are misfits, and a grid of one workgroup goes round more than once
    sh = shape(P, oracle, "value_branches")
    st = run_checked(P, ctx, sh, "blocks1_grid1", "value_branches")
    assert st["misfits"] >= sh.plan["hist"][2] > 16
    assert run_checked(P, ctx, sh, "blocks4", "value_branches")["misfits"] == 0
    assert run_checked(P, ctx, sh, "default", "value_branches")["misfits"] == 0
    # BranchPlan::staged: with sixteen hashed children a value of up to 6 bytes builds in the LDS slot, one of 7 and more in the scratch
    # blob -- whichever kernel takes the bin; nothing else of this trie goes there (no extension, no leaf of 544 bytes)
    scratch = 0
    for j in range(0, sh.plan["hist"][2], 2):
        v = BRANCH_VALUE_LENS[(j // 2) % len(BRANCH_VALUE_LENS)]
        if v >= 7:
            scratch += (3 + 16 * 33 + (1 if v <= 55 else 2 if v <= 255 else 3) + v + 3) & ~3
    for setting in ("default", "no_wave", "no_coop", "blocks4", "blocks1_grid1", "blocks2"):
        assert run_checked(P, ctx, sh, setting, "value_branches")["scratch_bytes"] == scratch > 0, setting
    # several hundred misfits in ONE bin: nodes of more than 3 children in one-block slots, of more than 7 in two-block slots
    sh = shape(P, oracle, "mixed_fanout")
    fans = [2 + (i * 7) % 15 for i in range(sh.plan["hist"][3])]
    for setting, fit in (("blocks1_grid1", 3), ("blocks2_grid1", 7), ("blocks1", 3), ("side_blocks1_grid1", 3)):
        st = run_checked(P, ctx, sh, setting, "mixed_fanout")
        assert st["misfits"] >= sum(f > fit for f in fans) > 64, (setting, st)
    # extensions over embedded branches are misfits of the small classes
    for name in ("embedded", "embedded_under_extension"):
        assert run_checked(P, ctx, shape(P, oracle, name), "blocks1_grid1", name)["misfits"] > 0
    # the helper stream: every bin beside the leaves, under each way of queueing and joining
    for name in ("deep_clusters", "embedded_under_extension"):
        sh = shape(P, oracle, name)
        for setting in ("side", "side_behind", "side_join", "side_lds0", "side_ldsmax", "side_blocks1_grid1"):
            st = run_checked(P, ctx, sh, setting, name)
            assert st["deep_from"] >= 1 and st["side_bins"] == st["bins"] >= 2 and not st["leaf_big"], (name, setting, st)
            assert st["leaves_ahead"] == (setting != "side_behind")
    assert run_checked(P, ctx, shape(P, oracle, "deep_clusters"), "side_blocks1_grid1", "deep_clusters")["misfits"] > 0
    # a leaf that may reach a rate block: no helper stream, and the kernel for such leaves
    for name in ("deep_clusters_big_leaf", "leaf_sizes", "long_extensions"):
        st = run_checked(P, ctx, shape(P, oracle, name), "side", name)
        assert st["deep_from"] == -1 and st["side_bins"] == 0 and st["leaf_big"], (name, st)
    assert not run_checked(P, ctx, shape(P, oracle, "deep_clusters"), "default", "deep_clusters")["leaf_big"]
    # the small pass where the trie fits it
    for name in ("deep_clusters", "value_branches", "leaf_sizes", "embedded_root", "long_extensions"):
        assert run_checked(P, ctx, shape(P, oracle, name), "small", name)["pass"] == "small"


def exact_bins():
    return EXACT_BINS if suite.FULL or not suite.EMULATED else EXACT_BINS_EMULATED


def test_bins_of_exact_size(P, oracle, ctx):
    """launch_bin at the edges of its kernels: branch_wave_kernel in workgroups of one wave up to 512 nodes and of four beyond, up to
    WAVE_MAX_NODES = 2 048; branch_coop_kernel two nodes a workgroup up to 1 024 and eight beyond, up to COOP_MAX_NODES = 4 096;
    a lane per node from 4 097 -- and with the wave kernel off, and with both off.  The class of the bin of depth 4 is asserted."""
    for c in exact_bins():
        sh = shape(P, oracle, f"exact_bin_{c}")
        assert sh.plan["hist"][4] == c
        for setting, cls in (("default", "wave" if c <= 2048 else "half_wave" if c <= 4096 else "blocks4"),
                             ("no_wave", "half_wave" if c <= 4096 else "blocks4"), ("coop_max0", "blocks4")):
            if suite.EMULATED and not suite.FULL and c < 2048 and setting != "default":
                continue  # (the emulated default suite: the other two settings at WAVE_MAX_NODES and beyond only)
            st = run_checked(P, ctx, sh, setting, f"a bin of {c} nodes under {setting}")
            assert st["max_bin"] == c and st[cls] >= 1, (c, setting, st)
            others = {"wave", "half_wave", "blocks4"} - {cls}
            # (the bins above depth 4 hold c / 16, c / 256 ... nodes: below every threshold, so they share the class unless c > 2 048)
            if c <= 2048 or setting == "coop_max0":
                assert all(st[o] == 0 for o in others), (c, setting, st)


def test_full_branch_waves_with_the_root_node_wanted(P, oracle, ctx):
    """phant_mpt_root_nodes over the trie of full branches: with the root's bytes wanted (`t.root_enc`) the root -- a full branch
    without a value -- is excluded from the register-only path; the 532 bytes that come back hash to the oracle's root."""
    import ctypes as C
    sh = shape(P, oracle, "full_waves")
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for setting in ("no_coop", "blocks4", "default", "small"):
        seg, cap = np.array([0, len(sh.keys)], np.uint32), 600
        roots, enc, ln = np.zeros((1, 32), np.uint8), np.zeros((1, cap), np.uint8), np.zeros(1, np.uint32)
        with forced(ctx, setting) as knobs:
            ctx.check(ctx._lib.phant_mpt_root_nodes(ctx.handle, p(sh.kb), p(sh.ko), p(sh.vb), p(sh.vo), len(sh.keys), p(seg), 1, p(roots),
                                                    p(enc), cap, p(ln)))
            st = ctx.trie_stats()
        assert roots[0].tobytes() == sh.root, setting
        assert oracle.keccak256(enc[0, :int(ln[0])].tobytes()) == sh.root, setting
        assert int(ln[0]) == 532 or len(sh.keys) < 4000, setting  # (the emulated run's smaller trie has no full root)
        check_stats(st, expect(sh.plan, knobs), f"full_waves with the root node, {setting}")


# ---- forests ----
def _items(rng, k):
    return [_bytes(rng, rng.integers(1, 701)) for _ in range(k)]


FOREST_SETTINGS = ("default", "blocks1", "blocks1_grid1", "blocks2", "blocks2_grid1", "side", "side_behind")


def _forest_stats(st, knobs, n, what):
    """the keys of these tries are made inside the call (rlp(index), keccak256(address)): the pass, the forced class and the order of
    queueing are asserted; every one of them has nodes at depth 0 -- the roots --, so the helper stream must stay out"""
    forced_blocks = knobs.get("trie_slot_blocks", 0)
    assert st["pass"] == "general" and st["n"] == n and st["leaves_ahead"] == (knobs.get("trie_ahead_max_keys", -1) != 0), (what, st)
    assert st["deep_from"] == -1 and st["side_bins"] == 0, (what, st)
    if forced_blocks:
        assert st["blocks%d" % forced_blocks] == st["bins"] >= 2 and st["wave"] == st["half_wave"] == 0, (what, st)
    else:
        assert st["wave"] + st["half_wave"] + st["blocks4"] == st["bins"] >= 2 and st["blocks1"] == st["blocks2"] == 0, (what, st)


def test_forests_under_forced_slots_and_the_helper_stream(P, oracle, ctx):
    """phant_block_roots (three lists of 1, 300 and 2 500 items of 1 .. 700 bytes: three tries in one pass), phant_index_root_be32
    and phant_state_root (3 000 accounts with 0 .. 5 slots: thousands of tries of a handful of keys, then the accounts' trie) in
    one- and two-block slots and with the helper stream asked for."""
    rng = np.random.default_rng(2024)
    lists = [_items(rng, k) for k in suite.scale((1, 300, 2500), (1, 40, 200))]
    be32 = _items(rng, suite.scale(300, 60))
    acc = []
    for _ in range(suite.scale(3000, 200)):
        storage = {int(rng.integers(0, 2 ** 62)): int(rng.integers(1, 2 ** 62)) for _ in range(int(rng.integers(0, 6)))}
        acc.append(dict(addr=_bytes(rng, 20), nonce=int(rng.integers(0, 1000)), balance=int(rng.integers(0, 2 ** 62)) ** 2,
                        code=_bytes(rng, rng.integers(0, 300)), storage=storage))
    packed = [P.mpt.pack_items(x) for x in lists]
    want_lists, want_be32, want_state = [oracle.index_root_rlp(x) for x in lists], oracle.index_root_be32(be32), oracle.state_root(acc)
    for setting in FOREST_SETTINGS:
        with forced(ctx, setting) as knobs:
            assert P.mpt.block_roots_packed(packed, ctx=ctx) == want_lists, setting
            st = ctx.trie_stats()
            _forest_stats(st, knobs, sum(len(x) for x in lists), f"block_roots under {setting}")
            assert st["leaf_big"], setting
            if knobs.get("trie_slot_blocks") == 1:
                assert st["misfits"] > 0, (setting, st)  # (the lists' upper branches have up to sixteen children)
            assert P.mpt.index_root_be32(be32, ctx=ctx) == want_be32, setting
            _forest_stats(ctx.trie_stats(), knobs, len(be32), f"index_root_be32 under {setting}")
            assert P.state.state_root(acc, ctx=ctx) == want_state, setting
            _forest_stats(ctx.trie_stats(), knobs, len(acc), f"state_root under {setting}")  # (the last pass: the accounts' trie)


# ---- one context, many calls ----
INTERLEAVED = (("embedded_root", "side"), ("mixed_fanout", "blocks1_grid1"), ("leaf_sizes", "small"), ("deep_clusters", "side_behind"),
               ("exact_bin_2049", "no_wave"), ("embedded", "blocks2_grid1"), ("value_branches", "small"), ("deep_clusters", "side_join"),
               ("full_waves", "no_coop"), ("embedded_root", "small"), ("exact_bin_513", "default"), ("long_extensions", "side"),
               ("deep_clusters_big_leaf", "side"), ("embedded_under_extension", "side_blocks1_grid1"), ("value_branches", "coop_max0"),
               ("nested_chains", {"trie_small_max_keys": 4096}), ("deep_clusters", "side_ldsmax"), ("exact_bin_2", "blocks4_grid1"))


def test_one_context_small_large_small(P, oracle):
    """The shapes in a fixed interleaved order on ONE context, another setting each time, small after large after small: the arenas
    grow and are reused, the mailbox tag counts on, the small pass's persistent words and the helper stream's events are
    shared by everything that comes after."""
    c = new_context(P)
    try:
        for rep in range(suite.scale(2, 1)):
            for name, setting in INTERLEAVED:
                run_checked(P, c, shape(P, oracle, name), setting, f"round {rep}: {name} under {setting}")
    finally:
        c.close()


@pytest.mark.parametrize("setting", ["side", "small"])
def test_the_call_after_refused_keys(P, oracle, setting):
    """Keys that are not strictly increasing are refused by lcp_element while order_kernel, the leaves (general pass, queued ahead,
    the helper stream asked for) or small_climb_kernel are already in the stream: every one of them must do nothing, and the
    next call on that context -- the same arenas, mailbox and small_state -- must be right."""
    c = new_context(P)
    try:
        sh = shape(P, oracle, "deep_clusters")
        keys, vals = list(sh.keys), list(sh.vals)
        k = len(keys) // 3
        keys[k], keys[k + 1] = keys[k + 1], keys[k]
        kb, ko = P.mpt._pack(keys, np.uint32)
        for rep in range(2):
            with forced(c, setting):
                with pytest.raises(P.mpt.UnsortedError):
                    P.mpt.mptize_packed(kb, ko, sh.vb, sh.vo, ctx=c)
                with pytest.raises(P.mpt.UnsortedError):
                    P.mpt.mptize([P.mpt.KeyVal.init(b"\x01", b"a"), P.mpt.KeyVal.init(b"\x01", b"b")], ctx=c)
            st = run_checked(P, c, sh, setting, f"after refused keys, {setting}")
            assert st["pass"] == ("small" if setting == "small" else "general")
            assert setting == "small" or st["deep_from"] >= 1
    finally:
        c.close()


def test_the_call_after_a_refused_device_form_key(P, oracle):
    """A device-resident key longer than 255 bytes (only lcp_element can see it: its nibble depths would index the depth counters
    out of bounds) is refused, in both passes; the next call on the context is right."""
    import torch
    from phant_amd import _lib as L
    c = new_context(P)
    try:
        keys, vals = [b"\x01" * 10, b"\x02" * 300, b"\x03"], [b"a", b"b", b"c"]
        kb, ko = P.mpt._pack(keys, np.int32)
        vb, vo = P.mpt._pack(vals, np.int64)
        dev = [torch.from_numpy(a).cuda() for a in (kb, ko, vb, vo)]
        sh = shape(P, oracle, "deep_clusters")
        for setting in ("side", "small"):
            with forced(c, setting):
                with pytest.raises(L.PhantError) as e:
                    P.mpt.mptize_dev(*dev, ctx=c)
                    torch.cuda.synchronize()
                assert e.value.code == L.E_INVALID_ARG
            run_checked(P, c, sh, setting, f"after a refused device-form key, {setting}")
    finally:
        c.close()


def test_two_threads_small_pass_and_helper_stream(P, oracle):
    """Two host threads with a context each (ctypes releases the GIL for the call): one in the small pass, one in the general pass
    with its bins on the helper stream -- each has its own mailbox, small_state, helper stream and events; every root of both
    against the oracle, and each context's statistics are its own."""
    work = [shape(P, oracle, name) for name in ("deep_clusters", "embedded_under_extension", "deep_clusters", "embedded_under_extension")]
    bad = [[], []]

    def run(t):
        c = new_context(P)
        try:
            with forced(c, "small" if t == 0 else "side"):
                for rep in range(6):
                    for sh in work:
                        got, st = sh.run(P, c), c.trie_stats()
                        if got != sh.root or st["pass"] != ("small" if t == 0 else "general") or (t == 1 and st["deep_from"] < 1):
                            bad[t].append((rep, st))
        except Exception as e:  # noqa: BLE001 (reported by the assertion below)
            bad[t].append(repr(e))
        finally:
            c.close()

    th = [threading.Thread(target=run, args=(t,)) for t in (0, 1)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert bad == [[], []]


# ---- the small pass's hand-off ----
@pytest.mark.parametrize("name", ["nested_chains", "last_two_bytes"])
def test_small_pass_hand_off_repeated(P, oracle, name):
    """ADVICE.md's last item: the small pass's fence / count protocol (small_climb_kernel: a child's reference, a fence, the count,
    a fence, the other children's references; the last workgroup out clears the state for the next call) is only exercised on the
    GPU.  Tries whose nodes get their last child from a far-away workgroup, twenty times on one context, so that every call but
    the first starts from the words its predecessor's last workgroup cleared.  (trie_small_max_keys = 4 096: by its own rule the pass
    takes more than 2 048 keys only where the values are long.)"""
    sh = shape(P, oracle, name)
    c = new_context(P)
    try:
        with forced(c, {"trie_small_max_keys": 4096}):
            for rep in range(suite.scale(20, 3)):
                assert sh.run(P, c) == sh.root, (name, rep)
                assert c.trie_stats()["pass"] == "small"
    finally:
        c.close()
