"""A plain-Python definition of every output of phant_block_receipt_segments and of phant_receipts_decode_rlp, written from the rules
of include/phant_gpu.h (EIP-2718, EIP-658, EIP-7642 for the eth/69 form, the Yellow Paper's RLP) on top of tests/receipts_ref.py
(rlp_decode, bloom_of, the encoders) and the oracle's index_root_rlp -- not from the kernels.

A receipt here is the tuple of tests/receipts_ref.py, (tx_type, succeeded, cumulative_gas_used, logs), except that `succeeded` may be a
32-byte post-state root; a block is a list of raw receipt values in the call's form."""
import numpy as np

from oracle import oracle as O
from tests import receipts_ref as R

CONSENSUS, ETH69 = 0, 1
UNDECODABLE, BLOOM, GAS_ORDER, POST_STATE, ERROR_BITS = 1, 2, 4, 0x100, 7
RB_RECEIPT, RB_ROOT, RB_BLOOM, RB_GAS_USED, RB_COUNT = 1, 2, 4, 8, 16
SPLIT_OK, SPLIT_BAD_RLP, SPLIT_BAD_RECEIPT = 0, 1, 5
WIDTH = {"tx_type": 1, "status": 1, "cum_gas": 8, "gas_used": 8, "log_first": 4, "bloom": 256, "flags": 4, "log_receipt": 4, "address": 20,
         "topic_first": 4, "topics": 32, "data_at": 8, "data_len": 4, "encoded": 1, "encoded_off": 8, "receipts_root": 32, "logs_bloom": 256,
         "block_gas_used": 8, "block_first_bad": 4, "block_flags": 4}
PER_RECEIPT = ("tx_type", "status", "cum_gas", "gas_used", "log_first", "bloom", "flags")
PER_LOG = ("log_receipt", "address", "topic_first", "topics", "data_at", "data_len")
ENCODINGS = ("encoded", "encoded_off")
PER_BLOCK = ("receipts_root", "logs_bloom", "block_gas_used", "block_first_bad", "block_flags")
OUTPUTS = PER_RECEIPT + PER_LOG + ENCODINGS + PER_BLOCK


# ------------------------------------------------------------------------------------------------------------ the two wire forms
def _status_item(ok):
    return R.rlp_str(ok) if isinstance(ok, (bytes, bytearray)) else R.rlp_int(1 if ok else 0)


def _logs_item(logs):
    return R.rlp_list([R.rlp_list([R.rlp_str(a), R.rlp_list([R.rlp_str(t) for t in ts]), R.rlp_str(d)]) for a, ts, d in logs])


def encode_consensus(receipt, bloom=None):
    tx_type, ok, gas, logs = receipt
    body = R.rlp_list([_status_item(ok), R.rlp_int(gas), R.rlp_str(R.bloom_of(logs) if bloom is None else bloom), _logs_item(logs)])
    return (bytes([tx_type]) if tx_type else b"") + body


def encode_eth69(receipt):
    tx_type, ok, gas, logs = receipt
    return R.rlp_list([R.rlp_int(tx_type), _status_item(ok), R.rlp_int(gas), _logs_item(logs)])


def encode(receipt, form):
    return encode_eth69(receipt) if form == ETH69 else encode_consensus(receipt)


# ---------------------------------------------------------------------------------------------------------------- one row
def decode_row(raw, form):
    """-> None (undecodable) or (tx_type, status 0 / 1 / 2, cum_gas, logs, the status item's value, the embedded bloom or None)"""
    raw = bytes(raw)
    try:
        if not raw:
            return None
        tx_type = 0
        if form == CONSENSUS and raw[0] < 0x80:
            if raw[0] == 0:
                return None
            tx_type, raw = raw[0], raw[1:]
        items = R.rlp_decode(raw)
        if not isinstance(items, list) or len(items) != 4 or any(isinstance(x, list) for x in items[:3]) or not isinstance(items[3], list):
            return None
        if form == ETH69:
            t, status, gas, logs = items
            if len(t) > 1 or (len(t) == 1 and not 1 <= t[0] <= 0x7F):
                return None
            tx_type, bloom = (t[0] if t else 0), None
        else:
            status, gas, bloom, logs = items
            if len(bloom) != 256:
                return None
        if status not in (b"", b"\x01") and len(status) != 32:
            return None
        if len(gas) > 8 or gas[:1] == b"\x00":
            return None
        out = []
        for lg in logs:
            if not isinstance(lg, list) or len(lg) != 3 or isinstance(lg[0], list) or not isinstance(lg[1], list) or isinstance(lg[2], list):
                return None
            if len(lg[0]) != 20 or any(isinstance(t, list) or len(t) != 32 for t in lg[1]):
                return None
            out.append((lg[0], list(lg[1]), lg[2]))
        return tx_type, (2 if len(status) == 32 else len(status)), int.from_bytes(gas, "big"), out, status, bloom
    except (ValueError, IndexError):
        return None


def _data_offsets(raw, form, row):
    """where each log's data lies inside a decodable row: the row re-encoded piece by piece (it is canonical, so the pieces are its bytes)"""
    tx_type, _, gas, logs, status, bloom = row
    head = (R.rlp_int(tx_type) if form == ETH69 else b"") + R.rlp_str(status) + R.rlp_int(gas) + (R.rlp_str(bloom) if form == CONSENSUS else b"")
    logs_enc = [R.rlp_list([R.rlp_str(a), R.rlp_list([R.rlp_str(t) for t in ts]), R.rlp_str(d)]) for a, ts, d in logs]
    payload = head + R.rlp_list(logs_enc)
    at = (1 if form == CONSENSUS and tx_type else 0) + len(R.rlp_list([payload])) - len(payload) + len(head)
    at += len(R.rlp_list(logs_enc)) - sum(map(len, logs_enc))
    out = []
    for (a, ts, d), enc in zip(logs, logs_enc):
        out.append(at + len(enc) - len(d))
        at += len(enc)
    assert at == len(raw)
    return out


# ------------------------------------------------------------------------------------------------------------- the call
def expected(blocks, form, exp_root=None, exp_bloom=None, exp_gas=None, exp_count=None):
    """-> ({output: bytes}, first_bad_block, n_logs, n_topics, encoded_len)"""
    rows = {k: [] for k in OUTPUTS}
    n_logs = n_topics = at_byte = 0
    enc_off = [0]
    first_bad_block = len(blocks)
    for b, block in enumerate(blocks):
        prev, values, bloom_or, last_gas, first_bad = None, [], bytearray(256), 0, len(block)
        for j, raw in enumerate(block):
            raw = bytes(raw)
            row = decode_row(raw, form)
            rows["log_first"].append(n_logs)
            if row is None:
                f, fields, bloom, value = UNDECODABLE, (0, 0, 0, 0), bytes(256), raw
            else:
                tx_type, status, gas, logs, status_item, embedded = row
                bloom = R.bloom_of(logs)
                f = POST_STATE if status == 2 else 0
                if form == CONSENSUS and embedded != bloom:
                    f |= BLOOM
                if (gas == 0) if j == 0 else (prev is not None and gas <= prev[2]):
                    f |= GAS_ORDER
                fields = (tx_type, status, gas, (gas - (0 if j == 0 or prev is None else prev[2])) % 2**64)
                value = raw if form == CONSENSUS else encode_consensus((tx_type, status_item if status == 2 else status, gas, logs), bloom)
                for (a, ts, d), data_at in zip(logs, _data_offsets(raw, form, row)):
                    rows["log_receipt"].append(len(rows["flags"]))
                    rows["address"].append(a)
                    rows["topic_first"].append(n_topics)
                    rows["topics"] += ts
                    rows["data_at"].append(at_byte + data_at)
                    rows["data_len"].append(len(d))
                    n_logs, n_topics = n_logs + 1, n_topics + len(ts)
                last_gas = gas
                bloom_or = bytearray(x | y for x, y in zip(bloom_or, bloom))
            if f & ERROR_BITS:
                first_bad = min(first_bad, j)
            for k, v in zip(("tx_type", "status", "cum_gas", "gas_used"), fields):
                rows[k].append(v)
            rows["bloom"].append(bloom)
            rows["flags"].append(f)
            rows["encoded"].append(value)
            enc_off.append(enc_off[-1] + len(value))
            values.append(value)
            prev = row
            at_byte += len(raw)
        root = O.index_root_rlp(values)
        bf = RB_RECEIPT if first_bad < len(block) else 0
        if exp_root is not None and bytes(exp_root[b]) != root:
            bf |= RB_ROOT
        if exp_bloom is not None and bytes(exp_bloom[b]) != bytes(bloom_or):
            bf |= RB_BLOOM
        if exp_gas is not None and exp_gas[b] != last_gas:
            bf |= RB_GAS_USED
        if exp_count is not None and exp_count[b] != len(block):
            bf |= RB_COUNT
        if bf:
            first_bad_block = min(first_bad_block, b)
        for k, v in zip(PER_BLOCK, (root, bytes(bloom_or), last_gas, first_bad, bf)):
            rows[k].append(v)
    rows["log_first"].append(n_logs)
    rows["topic_first"].append(n_topics)
    rows["encoded_off"] = enc_off
    out = {}
    for k, v in rows.items():
        if WIDTH[k] in (4, 8):
            out[k] = np.asarray(v, "<u%d" % WIDTH[k]).tobytes()
        elif k in ("tx_type", "status"):
            out[k] = bytes(v)
        else:
            out[k] = b"".join(bytes(x) for x in v)
    return out, first_bad_block, n_logs, n_topics, enc_off[-1]


# --------------------------------------------------------------------------------------------------------- the splitter
def _item_at(b, at, end):
    """the header of one canonical item in b[at:end] -> (is_list, payload offset, payload length); its content is not looked into"""
    if at >= end:
        raise ValueError("no item")
    t = b[at]
    if t < 0x80:
        return False, at, 1
    short, base = (t < 0xB8, 0x80) if t < 0xC0 else (t < 0xF8, 0xC0)
    if short:
        pay, n = at + 1, t - base
        if base == 0x80 and n == 1 and (pay >= end or b[pay] < 0x80):
            raise ValueError("a single byte below 0x80 with a header")
    else:
        ll = t - base - 55
        if at + 1 + ll > end or b[at + 1] == 0:
            raise ValueError("a length cut short or with a leading zero")
        pay, n = at + 1 + ll, int.from_bytes(b[at + 1:at + 1 + ll], "big")
        if n < 56:
            raise ValueError("the short form was mandatory")
    if pay + n > end:
        raise ValueError("the item runs past the end")
    return t >= 0xC0, pay, n


def split(raw, eth69=False):
    """the per-block element of a Receipts message -> (SPLIT_*, [receipt values]); a refused block has none.  The receipts are not
    looked into: only the block's list and the header of each of its items are read."""
    raw, values = bytes(raw), []
    try:
        is_list, at, n = _item_at(raw, 0, len(raw))
        if not is_list or at + n != len(raw):
            return SPLIT_BAD_RLP, []
        items = []
        while at < len(raw):
            item_is_list, pay, n = _item_at(raw, at, len(raw))
            items.append((item_is_list, at, pay, n))
            at = pay + n
    except ValueError:
        return SPLIT_BAD_RLP, []
    for item_is_list, at, pay, n in items:
        if item_is_list:
            values.append(raw[at:pay + n])
        elif eth69 or n == 0 or raw[pay] > 0x7F:
            return SPLIT_BAD_RECEIPT, []
        else:
            values.append(raw[pay:pay + n])
    return SPLIT_OK, values


def split_all(raws, eth69=False):
    out = [split(r, eth69) for r in raws]
    return [s for s, _ in out], [v for _, v in out]


def message_item(values, eth69=False):
    """a block's receipts as a peer sends them: typed receipts wrapped as strings before eth/69"""
    return R.rlp_list([v if eth69 or v[0] >= 0xC0 else R.rlp_str(v) for v in values])


# ------------------------------------------------------------------------------------------------------------ fixtures
_fixture = None


def fixture_receipts():
    """the 87 fixture blocks' receipts as tests/test_gpu_receipts.py::test_fixture_receipt_tries derives them -> (per block the receipt
    tuples, per block the header's receiptTrie): no receipts for an empty block; for one transaction the status that hits the root; for
    two the receipts tests/golden.py finds.  Computed once."""
    global _fixture
    if _fixture is None:
        from tests import golden
        blocks, roots, found = [], [], {}
        for b in (b for c in golden.fixtures()["cases"] for b in c["blocks"]):
            want = bytes.fromhex(b["receipt_trie"])
            if not b["tx_values"]:
                mine = []
            elif len(b["tx_values"]) == 1:
                hits = [r for r in golden.one_transaction_receipts(b) if O.index_root_rlp([r]) == want]
                assert len(hits) == 1
                mine = [R.decode(hits[0])]
            else:
                key = (b["receipt_trie"], b["gas_used"])
                if key not in found:
                    found[key] = [R.decode(r) for r in golden.two_transaction_receipts(b, O.index_root_rlp)]
                mine = found[key]
            blocks.append(mine), roots.append(want)
        _fixture = (blocks, roots)
    return _fixture
