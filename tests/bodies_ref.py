"""TEST INFRASTRUCTURE: the definition of phant_block_bodies and of phant_bodies_decode_rlp in Python.

The row of transaction i in block b is row i of tests/tx_ref_forks.expected over ALL transactions of the segment with block b's base
fee, gas limit and blob base fee; the roots are oracle.index_root_rlp over the block's raw transactions / withdrawals; the per-block
verdicts follow include/phant_gpu.h.  The splitter is written from the header comment over tests/secp_ref.py's canonical RLP items."""
import numpy as np

from tests import secp_ref as S
from tests import tx_ref as T
from tests import tx_ref_forks as F

BODY_TX, BODY_TXS_ROOT, BODY_WD_ROOT, BODY_BLOB_GAS = 1, 2, 4, 8
SPLIT_OK, SPLIT_BAD_RLP, SPLIT_BAD_TX, SPLIT_UNCLES, SPLIT_BAD_WITHDRAWAL = range(5)
TX_NAMES = tuple(name for name, _, _ in T.OUTPUTS + F.TX_OUTPUTS)
AUTH_NAMES = tuple(name for name, _, _ in F.AUTH_OUTPUTS)
WIDTH = {name: np.dtype(dt).itemsize * k for name, dt, k in T.OUTPUTS + F.TX_OUTPUTS + F.AUTH_OUTPUTS}
WIDTH.update(tx_block=4, block_first_bad=4, block_blob_gas_used=8, transactions_root=32, withdrawals_root=32, block_flags=4)
BLOCK_NAMES = ("tx_block", "block_first_bad", "block_blob_gas_used", "transactions_root", "withdrawals_root", "block_flags")


def _per_block(v, nb):
    return [None] * nb if v is None else list(v)


def expected(oracle, block_txs, chain_id, fork, base_fee=None, gas_limit=None, blob_base_fee=None, recover=True, block_wds=None, exp_txs_root=None,
             exp_wd_root=None, exp_blob_gas=None):
    """block_txs: per block its raw transactions; base_fee / gas_limit / blob_base_fee / the three expectations: None or one value per
    block; block_wds: None or per block its withdrawals' encodings -> ({output name: bytes of the whole array}, first_bad_block, first_bad,
    n_auth, blob_gas_used)"""
    nb = len(block_txs)
    txs = [bytes(t) for b in block_txs for t in b]
    first = np.cumsum([0] + [len(b) for b in block_txs]).tolist()
    bf, gl, bbf = _per_block(base_fee, nb), _per_block(gas_limit, nb), _per_block(blob_base_fee, nb)
    calls = {}
    out = {name: [] for name in TX_NAMES if name != "auth_first"}
    whole = None
    for b in range(nb):
        key = (bf[b], gl[b], bbf[b])
        if first[b + 1] > first[b] and key not in calls:
            calls[key] = F.expected(oracle, txs, chain_id, fork, bf[b], gl[b], bbf[b], recover)
        if first[b + 1] > first[b]:
            whole = calls[key]
            for name in out:
                out[name].append(whole[0][name][first[b] * WIDTH[name]:first[b + 1] * WIDTH[name]])
    out = {name: b"".join(v) for name, v in out.items()}
    if whole is None:
        whole = F.expected(oracle, txs, chain_id, fork, None, None, None, recover)
    for name in AUTH_NAMES + ("auth_first",):  # (no block parameter enters a tuple's row)
        out[name] = whole[0][name]
    n_auth, blob_gas = whole[2], whole[3]
    flags = np.frombuffer(out["flags"], "<u4")
    blobs = np.frombuffer(out["blobs"], "<u4")
    bad = np.flatnonzero(flags & F.ERROR_BITS)
    out["tx_block"] = np.repeat(np.arange(nb), np.diff(first)).astype("<u4").tobytes()
    rel, gas, txr, wdr, bflags = [], [], [], [], []
    for b in range(nb):
        mine = bad[(bad >= first[b]) & (bad < first[b + 1])]
        rel.append(int(mine[0]) - first[b] if len(mine) else first[b + 1] - first[b])
        gas.append(F.GAS_PER_BLOB * int(blobs[first[b]:first[b + 1]].sum()))
        txr.append(oracle.index_root_rlp([bytes(t) for t in block_txs[b]]))
        f = BODY_TX if len(mine) else 0
        if exp_txs_root is not None and bytes(exp_txs_root[b]) != txr[-1]:
            f |= BODY_TXS_ROOT
        if block_wds is not None:
            wdr.append(oracle.index_root_rlp([bytes(w) for w in block_wds[b]]))
            if exp_wd_root is not None and bytes(exp_wd_root[b]) != wdr[-1]:
                f |= BODY_WD_ROOT
        if exp_blob_gas is not None and int(exp_blob_gas[b]) != gas[-1]:
            f |= BODY_BLOB_GAS
        bflags.append(f)
    out["block_first_bad"] = np.asarray(rel, "<u4").tobytes()
    out["block_blob_gas_used"] = np.asarray(gas, "<u8").tobytes()
    out["transactions_root"], out["withdrawals_root"] = b"".join(txr), b"".join(wdr)
    out["block_flags"] = np.asarray(bflags, "<u4").tobytes()
    bad_blocks = [b for b in range(nb) if bflags[b]]
    return out, (bad_blocks[0] if bad_blocks else nb), (int(bad[0]) if len(bad) else len(txs)), n_auth, blob_gas


# ------------------------------------------------------------------------------------------------------------ the splitter
def split(raw, bodies_only=False):
    """one raw block [header, txs, uncles, withdrawals?] (bodies_only: without the header) -> (SPLIT_*, [transaction values], [withdrawal
    values]); a refused block has no values"""
    raw = bytes(raw)
    bad = lambda code: (code, [], [])  # noqa: E731
    top = S.rlp_item(raw, 0, len(raw))
    if top is None or not top[0] or top[3] != len(raw):
        return bad(SPLIT_BAD_RLP)
    parts = S._items(raw, top[1], top[2])
    first = 0 if bodies_only else 1
    if parts is None or len(parts) not in (first + 2, first + 3) or not all(p[0] for p in parts):
        return bad(SPLIT_BAD_RLP)
    items = S._items(raw, parts[first][2], parts[first][3])
    if items is None:
        return bad(SPLIT_BAD_RLP)
    txs = []
    for it in items:
        if it[0]:
            txs.append(raw[it[1]:it[4]])
        elif it[3] > it[2] and raw[it[2]] <= 0x7F:
            txs.append(raw[it[2]:it[3]])
        else:
            return bad(SPLIT_BAD_TX)
    if parts[first + 1][3] != parts[first + 1][2]:
        return bad(SPLIT_UNCLES)
    wds = []
    if len(parts) == first + 3:
        items = S._items(raw, parts[first + 2][2], parts[first + 2][3])
        if items is None:
            return bad(SPLIT_BAD_RLP)
        if not all(it[0] for it in items):
            return bad(SPLIT_BAD_WITHDRAWAL)
        wds = [raw[it[1]:it[4]] for it in items]
    return SPLIT_OK, txs, wds


def split_all(raws, bodies_only=False):
    """-> (status list, per block its transaction values, per block its withdrawal values)"""
    r = [split(x, bodies_only) for x in raws]
    return [x[0] for x in r], [x[1] for x in r], [x[2] for x in r]


def make_block(txs, withdrawals=None, uncles=b"\xc0", header=None):
    """a raw block around raw transactions (typed ones wrapped as strings) and encoded withdrawals; header: its encoding (a list)"""
    body = [S.rlp_list([t if t and t[0] >= 0xC0 else S.rlp_bytes(t) for t in txs]), uncles]
    if withdrawals is not None:
        body.append(S.rlp_list(list(withdrawals)))
    return S.rlp_list(([S.rlp_list([S.rlp_bytes(b"h" * 32)]) if header is None else header]) + body)


def withdrawal(index, validator=7, address=b"\xaa" * 20, amount=1):
    """one withdrawal as it stands in a block: rlp([index, validator_index, address, amount])"""
    return S.rlp_list([S.rlp_int(index), S.rlp_int(validator), S.rlp_bytes(address), S.rlp_int(amount)])
