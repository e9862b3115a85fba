"""TEST INFRASTRUCTURE: the definition of phant_block_settle in Python integers.

A block of plain transfers settled without an EVM: the rows phant_block_transactions[_ex] and phant_block_txs_prestate answer, the
pre-state rows a witness proves and the block's withdrawals -> per transaction the gas it uses, the cumulative gas and the sender's
exact balance before it, per pre-state row the account_op / nonces / balances / code_hashes that phant_exec_witness_poststate reads
(src/blockchain/blockchain.zig:155-205 `applyBody`, :262-343 `processTransaction`, for the blocks in which no transaction meets code).
include/phant_gpu.h restates this; DESIGN.md section 7n says why each rule is what it is.  Nothing here shares code with the library."""
import numpy as np

M64, M256 = (1 << 64) - 1, (1 << 256) - 1
LONDON, CANCUN, PRAGUE = 0, 1, 2
ROW_NONE = 0xFFFFFFFF
PRESENT, ABSENT = 1, 2
POST_KEEP, POST_SET, POST_DELETE = 0, 1, 2
EMPTY_CODE_HASH = bytes.fromhex("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470")
GWEI = 10**9

# what the call reads of the earlier calls' flags
TX_ERROR_BITS = 0x7FF | 0x7F000         # every error bit of phant_block_transactions[_ex]
TX_COST_OVERFLOW, TX_IS_CREATE = 0x400, 0x800
TXST_ERROR_BITS, TXST_SKIPPED, TXST_UNDETERMINED = 0x7F, 0x100, 0x200

# PHANT_SETTLE_*: settle_flags[i]
UPSTREAM, GAS_LIMIT, BALANCE_SHORT, NOT_PLAIN = 0x001, 0x002, 0x004, 0x100
ERROR_BITS = 0x007
FLAG_NAMES = ("Upstream", "GasLimit", "BalanceShort", None, None, None, None, None, "NotPlain")
COINBASE_UNKNOWN = 1                    # block_flags
WD_UNKNOWN = 1                          # wd_flags[j]
ACCT_OVERFLOW, ACCT_NEGATIVE = 1, 2     # account_flags[j]
LAST_PRECOMPILE = {LONDON: 0x09, CANCUN: 0x0A, PRAGUE: 0x11}

# the inputs in the order of phant_settle_in: (name, numpy dtype, elements per row, which count the rows follow)
INPUTS = (("base_fee", "u1", 32, "one"), ("type", "u1", 1, "n"), ("tx_flags", "u4", 1, "n"), ("gas_limit", "u8", 1, "n"), ("intrinsic_gas", "u8", 1, "n"),
          ("floor_gas", "u8", 1, "n"), ("value", "u1", 32, "n"), ("effective_gas_price", "u1", 32, "n"), ("upfront_cost", "u1", 32, "n"),
          ("to", "u1", 20, "n"), ("sender_row", "u4", 1, "n"), ("to_row", "u4", 1, "n"), ("state_flags", "u4", 1, "n"),
          ("account_status", "u1", 1, "n_accounts"), ("nonces", "u8", 1, "n_accounts"), ("balances", "u1", 32, "n_accounts"),
          ("code_hashes", "u1", 32, "n_accounts"), ("wd_row", "u4", 1, "n_wd"), ("wd_amount_gwei", "u8", 1, "n_wd"))
# the outputs in the order of phant_settle_out
OUTPUTS = (("settle_flags", "u4", 1, "n"), ("cumulative_gas_used", "u8", 1, "n"), ("balance_before", "u1", 32, "n"),
           ("account_op", "u1", 1, "n_accounts"), ("nonces_after", "u8", 1, "n_accounts"), ("balances_after", "u1", 32, "n_accounts"),
           ("code_hashes_after", "u1", 32, "n_accounts"), ("account_flags", "u1", 1, "n_accounts"), ("wd_flags", "u1", 1, "n_wd"))
SCALARS = ("first_bad", "n_not_plain", "first_not_plain", "block_flags", "n_wd_unknown", "gas_used")


def tx(sender_row, to_row, value=0, price=10, gas_limit=21000, intrinsic=21000, floor=0, to=b"\x22" * 20, type=0, tx_flags=0, state_flags=0, cost=None):
    """one transaction row as the transactions call and the pre-state call left it; cost None: gas_limit x price + value"""
    return {"sender_row": sender_row, "to_row": to_row, "value": value, "price": price, "gas_limit": gas_limit, "intrinsic": intrinsic, "floor": floor,
            "to": bytes(to), "type": type, "tx_flags": tx_flags, "state_flags": state_flags, "cost": gas_limit * price + value if cost is None else cost}


def account(nonce=0, balance=0, status=PRESENT, code_hash=EMPTY_CODE_HASH):
    """one pre-state row as phant_exec_witness_prestate left it"""
    return {"nonce": nonce, "balance": balance, "status": status, "code_hash": bytes(code_hash)}


def is_precompile(fork, to):
    return to[:19] == bytes(19) and 1 <= to[19] <= LAST_PRECOMPILE[fork]


def classify(fork, base_fee, t, accounts):
    """-> UPSTREAM, NOT_PLAIN or 0 (plain): from the row's own inputs alone"""
    gas = max(t["intrinsic"], t["floor"])
    if t["tx_flags"] & TX_ERROR_BITS or t["state_flags"] & (TXST_SKIPPED | TXST_ERROR_BITS) or t["price"] < base_fee:
        return UPSTREAM
    # what cannot happen behind calls that raised no error bit: a row without its rows, a charge beyond 256 bits
    if t["sender_row"] == ROW_NONE or (t["to_row"] == ROW_NONE and not t["tx_flags"] & TX_IS_CREATE) or gas * t["price"] + t["value"] > M256:
        return UPSTREAM
    if t["type"] in (3, 4) or t["tx_flags"] & TX_IS_CREATE or t["state_flags"] & TXST_UNDETERMINED:
        return NOT_PLAIN
    if accounts[t["to_row"]]["code_hash"] != EMPTY_CODE_HASH or is_precompile(fork, t["to"]):
        return NOT_PLAIN
    return 0


def define(fork, block_gas_limit, base_fee, coinbase_row, txs, accounts, withdrawals=()):
    """withdrawals: (row, amount in gwei) -> ({output: list of integers, one per row}, {scalar: value}).  The loop applyBody runs,
    over the plain rows alone."""
    n, na = len(txs), len(accounts)
    proven = lambda j: j != ROW_NONE and accounts[j]["status"] in (PRESENT, ABSENT)  # noqa: E731
    out = {"settle_flags": [0] * n, "cumulative_gas_used": [0] * n, "balance_before": [0] * n, "account_op": [POST_KEEP] * na,
           "nonces_after": [a["nonce"] for a in accounts], "balances_after": [a["balance"] for a in accounts],
           "code_hashes_after": [a["code_hash"] for a in accounts], "account_flags": [0] * na, "wd_flags": [0] * len(withdrawals)}
    balance = [a["balance"] for a in accounts]  # exact and signed
    sends, touched = [0] * na, set()
    coinbase_known = proven(coinbase_row)
    cum = n_not_plain = block_flags = n_wd_unknown = 0
    first_not_plain = n
    for i, t in enumerate(txs):
        cls = classify(fork, base_fee, t, accounts)
        out["settle_flags"][i] = f = cls
        if cls == NOT_PLAIN:
            n_not_plain += 1
            first_not_plain = min(first_not_plain, i)
        if cls:
            continue
        gas = max(t["intrinsic"], t["floor"])
        s, r = t["sender_row"], t["to_row"]
        if t["gas_limit"] + cum > block_gas_limit:
            f |= GAS_LIMIT
        if balance[s] < t["cost"]:
            f |= BALANCE_SHORT
        out["balance_before"][i] = min(max(balance[s], 0), M256)
        cum += gas
        out["cumulative_gas_used"][i] = min(cum, M64)
        out["settle_flags"][i] = f
        balance[s] -= gas * t["price"] + t["value"]
        sends[s] += 1
        balance[r] += t["value"]
        touched |= {s, r}
        if coinbase_known:
            balance[coinbase_row] += gas * (t["price"] - base_fee)
            touched.add(coinbase_row)
        else:
            block_flags |= COINBASE_UNKNOWN
    for j, (row, gwei) in enumerate(withdrawals):
        if not proven(row):
            out["wd_flags"][j] = WD_UNKNOWN
            n_wd_unknown += 1
            continue
        balance[row] += gwei * GWEI
        touched.add(row)
    for j in touched:
        a = accounts[j]
        nonce = out["nonces_after"][j] = min(a["nonce"] + sends[j], M64)
        if balance[j] > M256:
            out["account_flags"][j] |= ACCT_OVERFLOW
        if balance[j] < 0:
            out["account_flags"][j] |= ACCT_NEGATIVE
        bal = out["balances_after"][j] = min(max(balance[j], 0), M256)
        if nonce == 0 and bal == 0 and a["code_hash"] == EMPTY_CODE_HASH:  # EIP-161: a touched empty account does not stay
            out["account_op"][j] = POST_DELETE if a["status"] == PRESENT else POST_KEEP
        else:
            out["account_op"][j] = POST_SET
    first_bad = next((i for i in range(n) if out["settle_flags"][i] & ERROR_BITS), n)
    return out, {"first_bad": first_bad, "n_not_plain": n_not_plain, "first_not_plain": first_not_plain, "block_flags": block_flags,
                 "n_wd_unknown": n_wd_unknown, "gas_used": min(cum, M64)}


def settled(out, scalars, n):
    return scalars["first_bad"] == n and scalars["n_not_plain"] == 0 and scalars["block_flags"] == 0 and scalars["n_wd_unknown"] == 0 and \
        not any(out["account_flags"])


def errors(flags):
    return [name for k, name in enumerate(FLAG_NAMES) if name and (flags & ERROR_BITS) >> k & 1]


# ------------------------------------------------------------------------------------------------ the arrays of the C-ABI
def _rows(values, width):
    return np.frombuffer(b"".join(int(v).to_bytes(width, "big") for v in values), np.uint8).reshape(-1, width).copy() if len(values) else np.zeros((0, width), np.uint8)


def _bytes(values, width):
    return np.frombuffer(b"".join(values), np.uint8).reshape(-1, width).copy() if len(values) else np.zeros((0, width), np.uint8)


def inputs(base_fee, txs, accounts, withdrawals=(), floor=True):
    """the arrays of phant_settle_in, by its member names (floor False: floor_gas is None, which the call reads as zeros)"""
    col = lambda k, dt: np.asarray([t[k] for t in txs], dt)  # noqa: E731
    return {"base_fee": _rows([base_fee], 32), "type": col("type", np.uint8), "tx_flags": col("tx_flags", np.uint32), "gas_limit": col("gas_limit", np.uint64),
            "intrinsic_gas": col("intrinsic", np.uint64), "floor_gas": col("floor", np.uint64) if floor else None, "value": _rows([t["value"] for t in txs], 32),
            "effective_gas_price": _rows([t["price"] for t in txs], 32), "upfront_cost": _rows([t["cost"] for t in txs], 32),
            "to": _bytes([t["to"] for t in txs], 20), "sender_row": col("sender_row", np.uint32), "to_row": col("to_row", np.uint32),
            "state_flags": col("state_flags", np.uint32), "account_status": np.asarray([a["status"] for a in accounts], np.uint8),
            "nonces": np.asarray([a["nonce"] for a in accounts], np.uint64), "balances": _rows([a["balance"] for a in accounts], 32),
            "code_hashes": _bytes([a["code_hash"] for a in accounts], 32), "wd_row": np.asarray([w[0] for w in withdrawals], np.uint32),
            "wd_amount_gwei": np.asarray([w[1] for w in withdrawals], np.uint64)}


def expected(fork, block_gas_limit, base_fee, coinbase_row, txs, accounts, withdrawals=()):
    """-> ({output: its bytes as the call writes them}, {scalar: value})"""
    out, scalars = define(fork, block_gas_limit, base_fee, coinbase_row, txs, accounts, withdrawals)
    exp = {}
    for name, dtype, k, _ in OUTPUTS:
        if name == "code_hashes_after":
            exp[name] = b"".join(out[name])
        else:
            exp[name] = _rows(out[name], 32).tobytes() if k == 32 else np.asarray(out[name], dtype).tobytes()
    return exp, scalars


# ------------------------------------------------------------------------------------ the fixtures' blocks as a known answer
def fixture_accounts(fx, case, oracle):
    """a case's `pre` as (addresses, account() rows)"""
    addrs = [bytes.fromhex(a["addr"]) for a in case["pre"]]
    rows = [account(a["nonce"], int(a["balance"] or "0", 16), PRESENT, oracle.keccak256(bytes.fromhex(fx["codes"][a["code"]]))) for a in case["pre"]]
    return addrs, rows


def withdrawals_of(block):
    """a fixture block's withdrawals as (address, amount in gwei)"""
    from tests.txstate_ref import _flat_rlp_list
    out = []
    for w in block.get("withdrawal_values", ()):
        _, _, address, gwei = _flat_rlp_list(bytes.fromhex(w))
        out.append((address, int.from_bytes(gwei, "big")))
    return out


def apply(addrs, rows, out):
    """the rows after a block: what account_op / nonces_after / balances_after say -> [(address, row)] of the accounts that exist"""
    after = []
    for j, (addr, a) in enumerate(zip(addrs, rows)):
        op = out["account_op"][j]
        if op == POST_DELETE or (op == POST_KEEP and a["status"] == ABSENT):
            continue
        after.append((addr, a if op == POST_KEEP else dict(a, nonce=out["nonces_after"][j], balance=out["balances_after"][j], status=PRESENT)))
    return after
