"""The grids of the per-proof verify pipeline's two hash kernels (mpt_verify_v3.hip) against the oracle, through the C-ABI.

The deep tier's grid covers the depths a batch of all but uniformly long proofs has and no more, and it has no row for the
last one: a proof's last node rides with the wave of its parent when every proof of that wave ends there with a node of one
length below the rate -- in a trip of its own otherwise.  The list role's grid is sized from the queue a well-formed witness
leaves, its waves stride over a longer one.  None of this may change a status, a value range, a verdict or the number of
nodes hashed: every case compares all of them with oracle/verify.c, and the oracle alone says what each proof is.

Small batches take the tier split S = 0 and, below 2 049 nodes, its wave-per-node kernels: the splits are forced here (0, 2
and 5 levels deduplicated), and with 0 the lane-per-node kernel, which shares the deep tier's loop, is forced as well."""
import numpy as np
import pytest
import torch

from tests.test_gpu_verify import _Mode
from tests.witness_util import pack_proofs

pytestmark = pytest.mark.gpu

PRESENT, BAD_HASH, MISSING_NODE = 1, 16, 20  # include/phant_gpu.h
RATE, BRANCH_LEN = 136, 532


@pytest.fixture(scope="module", params=["levels0", "levels2", "levels5"])
def M(request):
    import phant_amd
    ctx = phant_amd.Context(dedup_levels=int(request.param[6:]))
    if request.param == "levels0":
        ctx.diag_set("verify_no_coop", 1)  # hash_deep_kernel<true>, whatever the batch's size
    yield _Mode(phant_amd.mpt, ctx, request.param)
    ctx.close()


_cache = {}


def _witness(n, depth, seed, **kw):
    """(root, keys, proofs) of phant_amd.witness.account_witness(n, depth, seed) without damage, as bytes; built once."""
    import phant_amd
    key = (n, depth, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        b = phant_amd.witness.account_witness(n, depth=depth, seed=seed, corrupt_frac=0.0, **kw).batch
        nodes, off, pfn = b.nodes.cpu().numpy(), b.node_off.cpu().numpy(), b.proof_first_node.cpu().numpy()
        keys = b.keys.cpu().numpy()
        proofs = tuple(tuple(nodes[off[j]:off[j + 1]].tobytes() for j in range(pfn[i], pfn[i + 1])) for i in range(b.n))
        _cache[key] = (b.roots.cpu().numpy().reshape(-1, 32)[0].tobytes(), tuple(keys[i].tobytes() for i in range(b.n)), proofs)
    root, keys, proofs = _cache[key]
    return root, list(keys), [list(p) for p in proofs]


def _verify(M, oracle, roots, ridx, keys, proofs):
    """Statuses, value ranges and the per-root verdict of the library and of the oracle: equal, or the test fails here."""
    nodes, node_off, pfn = pack_proofs(proofs)
    r = np.frombuffer(b"".join(roots), np.uint8)
    k = np.frombuffer(b"".join(keys), np.uint8)
    ri = None if ridx is None else np.asarray(ridx, np.uint32)
    got = M.verify_batch(r, ri, k, 32, nodes, node_off, pfn)
    want = oracle.mpt_verify_batch(r, ri, k, 32, nodes, node_off, pfn)
    assert np.array_equal(got[0], want[0]), (np.flatnonzero(got[0] != want[0])[:8], got[0][:12], want[0][:12])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    blamed = np.zeros(len(proofs), np.int64) if ri is None else ri.astype(np.int64)
    st = torch.from_numpy(got[0].copy()).cuda()
    fails = M.verdict_dev(st, None if ri is None else torch.from_numpy(ri.astype(np.int32)).cuda(), len(roots)).cpu().numpy()
    bad = ~np.isin(want[0], (M.PROOF_PRESENT, M.PROOF_ABSENT))
    assert np.array_equal(fails, np.bincount(blamed[bad], minlength=len(roots)))
    return want[0]


def _hashed_once(M, proofs, ridx):
    """verify_stats of the last launch == every node of the deep tier once, and of the shallow tier (no node of which is
    damaged here) every distinct multi-block node once and every shorter one, which has no group, per copy."""
    shallow = M._ctx.verify_tier_stats()["dedup_levels"]
    assert shallow == int(M.mode[6:])
    want, seen = [0] * 8, set()
    for i, p in enumerate(proofs):
        for d, nd in enumerate(p):
            group = (0 if ridx is None else int(ridx[i]), d, nd)
            if d < shallow and len(nd) >= RATE:
                if group in seen:
                    continue
                seen.add(group)
            want[min(len(nd) // RATE, 7)] += 1
    assert M._ctx.verify_stats() == want


def _rides(proofs):
    """the launcher's criterion for dropping the last depth's row: the mean proof length within an eighth of a node of 8"""
    total, n = sum(len(p) for p in proofs), len(proofs)
    return 8 * n - n // 8 <= total <= 8 * n


@pytest.mark.parametrize("n", [63, 64, 65, 129, 257])
def test_wave_edges(M, oracle, n):
    """depth-8 proofs up to, at and beyond a wave's and a workgroup's edge; a sixteenth of them damaged somewhere"""
    root, keys, proofs = _witness(257, 8, 41)
    keys, proofs = keys[:n], proofs[:n]
    rng = np.random.default_rng(n)
    for i in rng.choice(n, size=max(1, n // 16), replace=False):
        d = int(rng.integers(0, 8))
        nd = bytearray(proofs[i][d])
        nd[int(rng.integers(0, len(nd)))] ^= 0x04
        proofs[i][d] = bytes(nd)
    assert _rides(proofs)
    want = _verify(M, oracle, [root], None, keys, proofs)
    assert (want == BAD_HASH).sum() == max(1, n // 16) and (want == PRESENT).sum() == n - max(1, n // 16)


def test_riding_on_and_off_in_one_batch(M, oracle):
    """130 proofs: the first wave's are of depth 8 with proofs of depth 3, 6, 7 and 9, an empty one and one without its leaf
    (its last node a 532-byte branch) among them -- its lanes do not all end behind the depth-6 node, so its last two depths
    are two trips --, the other two waves' are all of depth 8 and ride.  Every node hashed exactly once."""
    base = _witness(257, 8, 41)
    other = {d: _witness(16, d, 50 + d) for d in (3, 6, 7, 9)}
    roots = [base[0]] + [other[d][0] for d in (3, 6, 7, 9)]
    rid = {3: 1, 6: 2, 7: 3, 9: 4}
    keys, proofs, ridx = base[1][:130], base[2][:130], [0] * 130
    odd = [(1, 3, 0), (5, 6, 0), (6, 9, 0), (17, 7, 0), (30, 3, 1), (31, 6, 1), (32, 7, 1), (33, 6, 2), (40, 7, 2), (63, 9, 1)]
    odd += [(41 + t, 9, 2 + t) for t in range(12)]  # (the longer ones keep the mean at 8)
    for at, d, k in odd:
        keys[at], proofs[at], ridx[at] = other[d][1][k], other[d][2][k], rid[d]
    proofs[0] = []               # only the empty trie is proven without nodes
    proofs[62] = proofs[62][:7]  # the leaf is missing
    assert all(len(p) == 8 for p in proofs[64:]) and len(proofs[62][-1]) == BRANCH_LEN and _rides(proofs)
    want = _verify(M, oracle, roots, ridx, keys, proofs)
    assert want[0] not in (PRESENT, M.PROOF_ABSENT) and want[62] == MISSING_NODE and (np.delete(want, [0, 62]) == PRESENT).all()
    _hashed_once(M, proofs, ridx)


def test_two_leaf_lengths_in_one_wave(M, oracle):
    """depth-8 proofs out of two tries whose leaves differ in length: alternating in the first wave (no common length: two
    trips), the second wave all of the one and the third all of the other (both ride, with their own lengths)"""
    a, b = _witness(257, 8, 41), _witness(64, 8, 43, value=bytes(range(1, 41)))
    assert len(a[2][0][7]) != len(b[2][0][7]) and max(len(a[2][0][7]), len(b[2][0][7])) < RATE
    pick = [(b, t // 2) if t % 2 else (a, t // 2) for t in range(64)] + [(a, 32 + t) for t in range(64)] + [(b, 32), (b, 33)]
    keys, proofs = [w[1][i] for w, i in pick], [w[2][i] for w, i in pick]
    ridx = [0 if w is a else 1 for w, _ in pick]
    assert _rides(proofs)
    want = _verify(M, oracle, [a[0], b[0]], ridx, keys, proofs)
    assert (want == PRESENT).all()
    _hashed_once(M, proofs, ridx)


@pytest.mark.parametrize("where", ["leaf", "slot", "marker"])
def test_damage_at_the_riding_node_and_at_its_parent(M, oracle, where):
    """One byte flipped in the leaf, in the depth-6 branch's slot for the key's nibble (the leaf's reference) and in one of
    that branch's marker bytes, in lanes 0, 31 and 63 of the second wave: exactly those proofs fail."""
    root, keys, proofs = _witness(257, 8, 41)
    keys, proofs = keys[:129], proofs[:129]
    hit = [64, 64 + 31, 64 + 63]
    for t, i in enumerate(hit):
        nib = keys[i][3] >> 4  # the key's nibble at depth 6
        d, at = {"leaf": (7, 5 + 40 * t), "slot": (6, 4 + 33 * nib + 13 * t), "marker": (6, (0, 3 + 33 * nib, BRANCH_LEN - 1)[t])}[where]
        nd = bytearray(proofs[i][d])
        nd[at] ^= 0x10
        proofs[i][d] = bytes(nd)
    want = _verify(M, oracle, [root], None, keys, proofs)
    assert np.flatnonzero(want != PRESENT).tolist() == hit and (want[hit] == BAD_HASH).all()


def test_list_queue_longer_than_its_grid(M, oracle):
    """300 depth-8 proofs in which every copy of a node of the first five levels differs from every other copy by one byte (in
    a slot off the proof's own path): whichever copy a group elects, the others are listed and hashed, and with the list role's
    grid held at one workgroup the queue is several times its four waves.  Only the untouched proof passes, the others fail at
    their root copy, and no proof is verified from scratch."""
    root, keys, proofs = _witness(300, 8, 47)
    for i in range(1, 300):
        for d in range(5):
            nib = (keys[i][d // 2] >> 4) if d % 2 == 0 else (keys[i][d // 2] & 15)
            nd = bytearray(proofs[i][d])
            nd[4 + 33 * ((nib + 1) % 16) + i % 32] ^= 1 + i // 32
            proofs[i][d] = bytes(nd)
    M._ctx.diag_set("verify_list_wgs", 1)
    try:
        want = _verify(M, oracle, [root], None, keys, proofs)
        shallow, listed = int(M.mode[6:]), M._ctx.verify_tier_stats()["list_nodes"]
        assert listed == 300 * shallow  # (0: no shallow tier, nothing listed)
        assert M._ctx.verify_path_stats()[0] == 0
    finally:
        M._ctx.diag_set("verify_list_wgs", 0)
    assert want[0] == PRESENT and (want[1:] == BAD_HASH).all()
    # ... and the grid sized by the library itself
    _verify(M, oracle, [root], None, keys, proofs)
    assert M._ctx.verify_path_stats()[0] == 0


@pytest.fixture
def ctx4():
    import phant_amd
    ctx = phant_amd.Context(dedup_levels=4)
    yield ctx
    ctx.close()


def test_multi_root_block_witness(ctx4, oracle):
    """BASELINE config 4's shape at a twentieth of its size (3 680 proofs of depth 8, 3, 5 and 7 against 100 roots), four
    levels deduplicated: a batch whose proofs are NOT uniformly long keeps a row of waves for every depth."""
    import phant_amd
    w = phant_amd.witness.block_witness(scale=0.05, corrupt_frac=0.05, seed=8)
    b = w.batch
    assert b.n == 1000 + 600 + 880 + 1200 and b.n_roots == 1 + 75 + 22 + 2
    fc = torch.full((b.n_roots,), -3, dtype=torch.int32, device=b.nodes.device)
    vo = torch.empty(b.n, dtype=torch.int64, device=b.nodes.device)
    vl = torch.empty(b.n, dtype=torch.int32, device=b.nodes.device)
    st = phant_amd.mpt.verify_batch_dev(b, value_off=vo, value_len=vl, fail_count=fc, ctx=ctx4)
    torch.cuda.synchronize()
    ridx = b.root_idx.cpu().numpy()
    want = oracle.mpt_verify_batch(b.roots.cpu().numpy().reshape(-1), ridx.astype(np.uint32), b.keys.cpu().numpy().reshape(-1), 32,
                                   b.nodes.cpu().numpy(), b.node_off.cpu().numpy().astype(np.uint64),
                                   b.proof_first_node.cpu().numpy().astype(np.uint32))
    assert np.array_equal(st.cpu().numpy(), want[0])
    assert np.array_equal(vo.cpu().numpy().view(np.uint64), want[1]) and np.array_equal(vl.cpu().numpy().view(np.uint32), want[2])
    bad = ~np.isin(want[0], (phant_amd.mpt.PROOF_PRESENT, phant_amd.mpt.PROOF_ABSENT))
    assert np.array_equal(fc.cpu().numpy(), np.bincount(ridx[bad], minlength=b.n_roots)) and bad.sum() == w.n_invalid > 0
    assert ctx4.verify_tier_stats()["dedup_levels"] == 4 and ctx4.verify_path_stats()[0] == 0
