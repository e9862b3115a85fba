"""TEST INFRASTRUCTURE: the definition of phant_block_fee_history (include/phant_gpu.h) in Python integers -- per block the priority fee at
chosen percentiles of its gas used, eth_feeHistory's `reward`: tips against the block's base fee, `sorted` with a (tip, index) key, and
geth's loop taken literally with the threshold in integers.  And the two host rules phant_amd.types.block.fee_history adds around it,
restated from their EIPs: the next block's base fee (EIP-1559) and excess blob gas (EIP-4844)."""
import numpy as np

FEE_BELOW_BASE = 1
OUTPUTS = ("reward", "tip", "order", "block_gas_used", "block_flags")
M64 = (1 << 64) - 1


def reaches(S, G, p):
    """the division-free form of S >= floor(G p / 10000) the kernels use"""
    return 10000 * (S + 1) > G * p


def block_rewards(tips, gas, percentiles_bp):
    """one block: -> (order within the block, rewards, G)"""
    order = sorted(range(len(tips)), key=lambda i: (tips[i], i))
    G = sum(gas)
    rewards = []
    for p in percentiles_bp:
        if not order:
            rewards.append(0)
            continue
        threshold = G * p // 10000
        r, s = 0, gas[order[0]]
        while s < threshold and r < len(order) - 1:  # geth: for sumGasUsed < thresholdGasUsed && txIndex < len(txs) - 1
            r += 1
            s += gas[order[r]]
        rewards.append(tips[order[r]])
    return order, rewards, G


def expected(block_first, price, gas_used, percentiles_bp, base_fee=None):
    """block_first: n_blocks + 1 integers; price: n integers; gas_used: n integers; base_fee: n_blocks integers or None
    -> ({output: bytes as the C-ABI lays it out}, first_bad_block)"""
    nb = len(block_first) - 1
    tip_b, order_b, reward_b, gas_b, flags = [], [], [], [], []
    for b in range(nb):
        s, e = int(block_first[b]), int(block_first[b + 1])
        base = 0 if base_fee is None else int(base_fee[b])
        f = 0
        tips = []
        for i in range(s, e):
            if int(price[i]) < base:
                tips.append(0)
                f |= FEE_BELOW_BASE
            else:
                tips.append(int(price[i]) - base)
        order, rewards, G = block_rewards(tips, [int(g) for g in gas_used[s:e]], percentiles_bp)
        tip_b += tips
        order_b += [s + r for r in order]
        reward_b += rewards
        gas_b.append(min(G, M64))
        flags.append(f)
    bad = [b for b in range(nb) if flags[b]]
    out = {"reward": b"".join(r.to_bytes(32, "big") for r in reward_b), "tip": b"".join(t.to_bytes(32, "big") for t in tip_b),
           "order": np.asarray(order_b, "<u4").tobytes(), "block_gas_used": np.asarray(gas_b, "<u8").tobytes(),
           "block_flags": np.asarray(flags, "<u4").tobytes()}
    return out, (bad[0] if bad else nb)


def next_base_fee(base_fee, gas_used, gas_limit):
    """EIP-1559 as include/phant_gpu.h states it for PHANT_HDR_BASE_FEE: t = gas_limit / 2, all divisions floor"""
    t = gas_limit // 2
    if gas_used == t:
        return base_fee
    if gas_used > t:
        return base_fee + max(base_fee * (gas_used - t) // t // 8, 1)
    return base_fee - base_fee * (t - gas_used) // t // 8


def next_excess_blob_gas(excess, blob_gas_used, target):
    """EIP-4844's calc_excess_blob_gas"""
    return max(excess + blob_gas_used - target, 0)
