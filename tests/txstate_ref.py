"""TEST INFRASTRUCTURE: the definition of phant_block_txs_prestate in Python integers.

A block's transactions (the rows phant_block_transactions[_ex] answers) against the pre-state a witness proves (the rows
phant_exec_witness_prestate answers): which witness row every sender, recipient, authority and probe is, the nonce every transaction
must carry, EIP-3607, and an upper bound on what a sender can have spent before each of its transactions.  include/phant_gpu.h restates
this; DESIGN.md section 7k says why each rule is what it is.  Nothing here shares code with the library."""
import numpy as np

M64, M256 = (1 << 64) - 1, (1 << 256) - 1
LONDON, CANCUN, PRAGUE = 0, 1, 2
ROW_NONE = CODE_NONE = 0xFFFFFFFF
SIG_OK, PRESENT, ABSENT = 0, 1, 2
TX_UNDECODABLE, TX_BAD_V, TX_SIGNATURE, TX_COST_OVERFLOW, TX_IS_CREATE = 0x001, 0x002, 0x004, 0x400, 0x800
EMPTY_CODE_HASH = bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")

# PHANT_TXST_*: bit k of state_flags[i]
FLAG_NAMES = ("SenderUnknown", "ToUnknown", "NonceLow", "NonceHigh", "BalanceShort", "NotEOA", "CodeMissing", None, "Skipped", "Undetermined",
              "NeedsInflow", "SpentSaturated")
SENDER_UNKNOWN, TO_UNKNOWN, NONCE_LOW, NONCE_HIGH, BALANCE_SHORT, NOT_EOA, CODE_MISSING = (1 << k for k in range(7))
SKIPPED, UNDETERMINED, NEEDS_INFLOW, SPENT_SATURATED = 0x100, 0x200, 0x400, 0x800
ERROR_BITS = 0x7F
ROLE_SENDER, ROLE_RECIPIENT, ROLE_AUTHORITY, ROLE_PROBE = 1, 2, 4, 8

# the outputs in the order of phant_txstate_out: (name, numpy dtype, elements per row, which count the rows follow)
OUTPUTS = (("sender_row", "u4", 1, "n"), ("to_row", "u4", 1, "n"), ("expected_nonce", "u8", 1, "n"), ("spent_before", "u1", 32, "n"),
           ("state_flags", "u4", 1, "n"), ("sends", "u4", 1, "n_accounts"), ("roles", "u1", 1, "n_accounts"), ("probe_row", "u4", 1, "n_probe"))


def tx(sender, nonce=0, cost=0, to=b"\x00" * 20, sig_status=SIG_OK, flags=0):
    """one transaction row as the transactions call left it: cost is upfront_cost (2^256 and beyond: the row is zero and
    PHANT_TX_COST_OVERFLOW is set, as that call does)"""
    if cost > M256:
        cost, flags = 0, flags | TX_COST_OVERFLOW
    return {"sender": bytes(sender), "nonce": nonce, "cost": cost, "to": bytes(to), "sig_status": sig_status, "flags": flags}


def account(address, nonce=0, balance=0, status=PRESENT, code_hash=EMPTY_CODE_HASH, code_index=CODE_NONE):
    """one pre-state row as phant_exec_witness_prestate left it"""
    return {"address": bytes(address), "nonce": nonce, "balance": balance, "status": status, "code_hash": bytes(code_hash), "code_index": code_index}


def participates(t):
    return t["sig_status"] == SIG_OK and not t["flags"] & (TX_UNDECODABLE | TX_BAD_V | TX_SIGNATURE)


def is_designator(a, codes):
    """EIP-7702: the account's code is 0xef0100 || address"""
    if a["code_hash"] == EMPTY_CODE_HASH or a["code_index"] == CODE_NONE:
        return False
    code = codes[a["code_index"]]
    return len(code) == 23 and code[:3] == b"\xef\x01\x00"


def define(fork, txs, accounts, codes=(), auth_first=None, auths=(), probes=()):
    """-> ({output: list of integers, one per row}, first_bad, n_undetermined).  auths: (authority, auth_status) per tuple;
    auth_first: None or n + 1 offsets into them."""
    n = len(txs)
    row_of = {}
    for j, a in enumerate(accounts):
        row_of.setdefault(a["address"], j)  # the LOWEST row with that address
    proven = lambda j: j != ROW_NONE and accounts[j]["status"] in (PRESENT, ABSENT)  # noqa: E731
    out = {"sender_row": [ROW_NONE] * n, "to_row": [ROW_NONE] * n, "expected_nonce": [0] * n, "spent_before": [0] * n, "state_flags": [0] * n,
           "sends": [0] * len(accounts), "roles": [0] * len(accounts), "probe_row": [row_of.get(bytes(p), ROW_NONE) for p in probes]}
    for j in out["probe_row"]:
        if j != ROW_NONE:
            out["roles"][j] |= ROLE_PROBE
    spent, authorized, n_undetermined = {}, set(), 0  # per sequence: the costs so far; the authorities of the transactions so far
    for i, t in enumerate(txs):
        if not participates(t):
            out["state_flags"][i] = SKIPPED
            continue
        f = 0
        s = out["sender_row"][i] = row_of.get(t["sender"], ROW_NONE)
        if s != ROW_NONE:
            out["roles"][s] |= ROLE_SENDER
        if not proven(s):
            f |= SENDER_UNKNOWN
        else:
            a = accounts[s]
            before = spent.get(s, 0)
            cost = 1 << 256 if t["flags"] & TX_COST_OVERFLOW else t["cost"]
            out["expected_nonce"][i] = expected = min(a["nonce"] + out["sends"][s], M64)
            out["spent_before"][i] = min(before, M256)
            if before > M256:
                f |= SPENT_SATURATED
            if fork >= PRAGUE and (is_designator(a, codes) or t["sender"] in authorized):
                f |= UNDETERMINED
                n_undetermined += 1
            else:
                if t["nonce"] < expected:
                    f |= NONCE_LOW
                if t["nonce"] > expected:
                    f |= NONCE_HIGH
                if a["code_hash"] != EMPTY_CODE_HASH:
                    f |= CODE_MISSING if fork >= PRAGUE and a["code_index"] == CODE_NONE else NOT_EOA
                if a["balance"] < before + cost:
                    f |= NEEDS_INFLOW | (BALANCE_SHORT if i == 0 else 0)
            out["sends"][s] += 1
            spent[s] = before + cost
        if not t["flags"] & TX_IS_CREATE:
            r = out["to_row"][i] = row_of.get(t["to"], ROW_NONE)
            if r != ROW_NONE:
                out["roles"][r] |= ROLE_RECIPIENT
            if not proven(r):
                f |= TO_UNKNOWN
        out["state_flags"][i] = f
        if auth_first is not None:  # this transaction's tuples count from the NEXT transaction on
            for authority, status in auths[auth_first[i]:auth_first[i + 1]]:
                if status == SIG_OK:
                    authorized.add(bytes(authority))
                    if bytes(authority) in row_of:
                        out["roles"][row_of[bytes(authority)]] |= ROLE_AUTHORITY
    first_bad = next((i for i in range(n) if out["state_flags"][i] & ERROR_BITS), n)
    return out, first_bad, n_undetermined


def errors(flags):
    return [name for k, name in enumerate(FLAG_NAMES) if name and (flags & ERROR_BITS) >> k & 1]


# ------------------------------------------------------------------------------------------------ the arrays of the C-ABI
def _rows(values, width):
    return np.frombuffer(b"".join(int(v).to_bytes(width, "big") for v in values), np.uint8).reshape(-1, width).copy() if values else np.zeros((0, width), np.uint8)


def _bytes(values, width):
    return np.frombuffer(b"".join(values), np.uint8).reshape(-1, width).copy() if values else np.zeros((0, width), np.uint8)


def inputs(txs, accounts, codes=(), auth_first=None, auths=(), probes=()):
    """the arrays of phant_txstate_in, by its member names (auth_first: None stays None)"""
    code_off = np.zeros(len(codes) + 1, np.uint64)
    if codes:
        code_off[1:] = np.cumsum([len(c) for c in codes])
    return {"sender": _bytes([t["sender"] for t in txs], 20), "sig_status": np.asarray([t["sig_status"] for t in txs], np.uint8),
            "tx_flags": np.asarray([t["flags"] for t in txs], np.uint32), "nonce": np.asarray([t["nonce"] for t in txs], np.uint64),
            "upfront_cost": _rows([t["cost"] for t in txs], 32), "to": _bytes([t["to"] for t in txs], 20),
            "auth_first": None if auth_first is None else np.asarray(auth_first, np.uint32),
            "authority": _bytes([bytes(a) for a, _ in auths], 20), "auth_status": np.asarray([s for _, s in auths], np.uint8),
            "addresses": _bytes([a["address"] for a in accounts], 20), "account_status": np.asarray([a["status"] for a in accounts], np.uint8),
            "nonces": np.asarray([a["nonce"] for a in accounts], np.uint64), "balances": _rows([a["balance"] for a in accounts], 32),
            "code_hashes": _bytes([a["code_hash"] for a in accounts], 32), "code_index": np.asarray([a["code_index"] for a in accounts], np.uint32),
            "code_off": code_off, "codes": np.frombuffer(b"".join(codes), np.uint8).copy(), "probe": _bytes([bytes(p) for p in probes], 20)}


def expected(fork, txs, accounts, codes=(), auth_first=None, auths=(), probes=()):
    """-> ({output: its bytes as the call writes them}, first_bad, n_undetermined)"""
    out, first_bad, n_undetermined = define(fork, txs, accounts, codes, auth_first, auths, probes)
    exp = {}
    for name, dtype, k, _ in OUTPUTS:
        exp[name] = _rows(out[name], 32).tobytes() if k == 32 else np.asarray(out[name], dtype).tobytes()
    return exp, first_bad, n_undetermined


# ------------------------------------------------------------------------------------ the fixtures' blocks as a known answer
def walk_fixtures(oracle, rows_of, answer):
    """Every case of tests/golden/fixture_roots.json.gz, its blocks in order over `pre`: the nonces advance by `sends` from block to
    block, a block's withdrawals are credited behind it (the fixtures state them: one case funds its only sender that way), and every
    `to` that `pre` lacks is added as an ABSENT row, as a witness would prove it.  rows_of(raw transactions) -> the
    tx() rows; answer(txs, accounts, codes) -> (define()'s lists, first_bad).  -> the counts the fixtures fix, which owe nothing to
    either: transactions whose sender was found, whose nonce is the expected one, distinct recipients `pre` lacks, senders whose nonce
    in `post` is their nonce in `pre` plus their transactions, and the error bits seen."""
    from tests import golden
    fx = golden.fixtures()
    found = nonce_ok = post_ok = error_bits = 0
    missing = set()
    for case in fx["cases"]:
        codes = sorted({a["code"] for a in case["pre"] if fx["codes"][a["code"]]})
        blobs = [bytes.fromhex(fx["codes"][c]) for c in codes]
        accounts = [account(bytes.fromhex(a["addr"]), a["nonce"], int(a["balance"] or "0", 16), PRESENT,
                            oracle.keccak256(bytes.fromhex(fx["codes"][a["code"]])), codes.index(a["code"]) if a["code"] in codes else CODE_NONE)
                    for a in case["pre"]]
        sent = {}
        for block in case["blocks"]:
            txs = rows_of([bytes.fromhex(t) for t in block["tx_values"]])
            for t in txs:
                if not t["flags"] & TX_IS_CREATE and all(a["address"] != t["to"] for a in accounts):
                    missing.add(t["to"])
                    accounts.append(account(t["to"], status=ABSENT))
            out, first_bad = answer(txs, accounts, blobs)
            assert first_bad == len(txs), (case["name"], first_bad)
            for i, t in enumerate(txs):
                found += out["sender_row"][i] != ROW_NONE
                nonce_ok += out["expected_nonce"][i] == t["nonce"]
                error_bits |= out["state_flags"][i] & ERROR_BITS
            for j, k in enumerate(out["sends"]):
                accounts[j]["nonce"] += k
                if k:
                    sent[accounts[j]["address"]] = sent.get(accounts[j]["address"], 0) + k
            for w in block.get("withdrawal_values", ()):
                _, _, address, gwei = _flat_rlp_list(bytes.fromhex(w))
                for a in accounts:
                    if a["address"] == address:
                        a["balance"] += int.from_bytes(gwei, "big") * 10**9
        if "post" in case:
            before = {bytes.fromhex(a["addr"]): a["nonce"] for a in case["pre"]}
            after = {bytes.fromhex(a["addr"]): a["nonce"] for a in case["post"]}
            post_ok += sum(1 for addr, k in sent.items() if addr in after and before[addr] + k == after[addr])
    return {"found": found, "nonce_ok": nonce_ok, "recipients_missing": len(missing), "post_ok": post_ok, "error_bits": error_bits}


def _flat_rlp_list(b):
    """the items of a short list of short strings (a withdrawal: [index, validator, address, amount])"""
    assert 0xC0 <= b[0] <= 0xF7 and len(b) == 1 + b[0] - 0xC0
    items, at = [], 1
    while at < len(b):
        if b[at] < 0x80:
            items.append(b[at:at + 1])
            at += 1
        else:
            assert b[at] <= 0xB7
            items.append(b[at + 1:at + 1 + b[at] - 0x80])
            at += 1 + b[at] - 0x80
    return items


FIXTURE_ANSWER = {"found": 70, "nonce_ok": 70, "recipients_missing": 1, "post_ok": 65, "error_bits": 0}


def rows_from_analysis(oracle, raws, chain_id=1):
    """tests/tx_ref.py's analysis of raw transactions as tx() rows"""
    from tests import tx_ref as T
    rows = []
    for raw in raws:
        o = T.analyse(oracle, raw, chain_id)
        rows.append({"sender": o["sender"], "nonce": o["nonce"], "cost": int.from_bytes(o["upfront_cost"], "big"), "to": o["to"],
                     "sig_status": o["sig_status"], "flags": o["flags"]})
    return rows
