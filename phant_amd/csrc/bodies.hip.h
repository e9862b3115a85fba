// bodies.hip.h -- the bodies of a chain segment in one call (included by bulk_keccak.hip behind transactions.hip.h; DESIGN.md section
// 7o): the transactions of n_blocks blocks through the steps of phant_block_transactions_ex (transactions.hip.h: tx::Call), the
// rules under each block's own base fee, gas limit and blob base fee, the per-block verdicts, and the transactions and withdrawals
// tries of all blocks as ONE forest pass.
//
//   body_check_kernel     device form only: tx_off, wd_off, block_first and wd_first as the caller states them, a lane per entry; the
//                         host reads the verdict before any other kernel indexes with them
//   body_tx_block_kernel  a lane per transaction: its block, by bisecting block_first (an upper bound: empty blocks are skipped)
//   (tx_decode_kernel, tx_hash_kernel, the tuples' kernels, ecrecover_kernel: transactions.hip.h's, over the whole segment)
//   body_rules_kernel     a lane per transaction: tx::rules_row under the parameters of its block; then per distinct block of the wave ONE
//                         lane lowers the block's first bad transaction and adds the block's versioned hashes
//   (seg::launch_forest)  segment_lists.hip.h's lengths, scan and pairs over body::Src: a WAVE per value copies its bytes from index
//                         order into trie order
//   (trie_forest_dev)     all lists of the segment, tries 0 .. n_blocks - 1 the transactions, the withdrawals behind them
//   body_verdict_kernel   a lane per block: roots and blob gas against what the header says, block_flags, the least bad block
//
// Plain C++ plus the cross-lane builtins keyed_table.hip.h uses: tests/emu.py compiles this file for the host.
#pragma once
#include "segment_lists.hip.h"
#include "transactions.hip.h"

namespace phant {
namespace body {

// the call's own control word next to transactions.hip.h's: [3] = n_blocks - (the least flagged block) or 0
constexpr uint32_t CTL_BAD_BLOCK = 3;

// the segment in device memory
struct Seg {
    const uint32_t* block_first;
    const uint64_t* wd_off;
    const uint32_t* wd_first;
    const uint8_t* wd;
    const uint8_t *base_fee, *blob_base_fee;  // n_blocks x 32 big-endian, or null
    const uint64_t* gas_limit;                // n_blocks, or null
    const uint8_t *exp_txs_root, *exp_wd_root;
    const uint64_t* exp_blob_gas;
    uint32_t n_blocks, n, n_wd, fork;
    uint32_t* tx_block;
    uint8_t* roots;  // tx_tries x 32, then wd_tries x 32
    uint32_t* block_flags;
    uint32_t* first_bad;                 // zeroed: count - (the least flagged transaction of the block); the verdict turns it round
    unsigned long long* blob_gas;        // zeroed: the block's versioned hashes; the verdict multiplies
};

__global__ void __launch_bounds__(256) body_check_kernel(const uint64_t* __restrict__ tx_off, uint64_t tx_bytes, const uint64_t* __restrict__ wd_off,
                                                         uint64_t wd_bytes, const uint32_t* __restrict__ block_first,
                                                         const uint32_t* __restrict__ wd_first, uint32_t n, uint32_t n_wd, uint32_t n_blocks,
                                                         uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t f = 0;
    if (i < n) f |= seg::off_flags(tx_off, i, n, tx_bytes);
    if (i < n_wd) f |= seg::off_flags(wd_off, i, n_wd, wd_bytes);
    if (i < n_blocks) f |= seg::first_flags(block_first, i, n_blocks, n);
    if (i < n_blocks && wd_first) f |= seg::first_flags(wd_first, i, n_blocks, n_wd);
    if (f) atomicOr(ctl, f);
}

__global__ void __launch_bounds__(256) body_tx_block_kernel(const uint32_t* __restrict__ block_first, uint32_t n_blocks, uint32_t n,
                                                            uint32_t* __restrict__ tx_block) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) tx_block[i] = seg::block_of(block_first, n_blocks, i);
}

// The rules with the parameters read through tx_block.  The lanes of a wave hold consecutive transactions, so the lanes of one block
// are neighbours: per distinct block of the wave its lowest lane speaks for all of them (keyed_table.hip.h's wave_first_of, with the
// block's sums taken from one scan of the wave) -- a block of 10 000 transactions sends 157 atomics to its words, not 10 000.
__global__ void __launch_bounds__(64) body_rules_kernel(uint32_t n, Seg sg, tx::Dev dv, const uint8_t* __restrict__ sig_status) {
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    const bool has = i < n;
    uint32_t f = 0, b = 0;
    unsigned long long blobs = 0;
    if (has) {
        b = sg.tx_block[i];
        tx::Rules ru;
        for (int k = 0; k < 8; ++k) ru.base_fee[k] = ru.blob_base_fee[k] = 0u;
        ru.have_base_fee = sg.base_fee ? 1u : 0u, ru.have_blob_base_fee = sg.blob_base_fee ? 1u : 0u, ru.have_gas_limit = sg.gas_limit ? 1u : 0u;
        ru.fork = sg.fork;
        if (sg.base_fee) tx::load_u256(sg.base_fee + 32ull * b, ru.base_fee);
        if (sg.blob_base_fee) tx::load_u256(sg.blob_base_fee + 32ull * b, ru.blob_base_fee);
        ru.block_gas_limit = sg.gas_limit ? sg.gas_limit[b] : 0ull;
        f = tx::rules_row(i, ru, dv, sig_status);
        blobs = dv.x.blobs[i];
    }
    const bool flagged = has && (f & tx::ERROR_BITS) != 0u, say = flagged || blobs != 0ull;
    const unsigned long long all_bad = __ballot(flagged);
    unsigned long long todo = __ballot(say);
    if (!todo) return;
    unsigned long long incl = blobs;  // the wave's inclusive scan of the hashes (a transaction has fewer than 2^27)
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t theirs = (uint32_t)__shfl((int)b, (int)leader);
        const unsigned long long same = __ballot(say && b == theirs), bad = all_bad & same;
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(same);
        const unsigned long long sum = __shfl(incl, (int)last) - __shfl(incl - blobs, (int)leader);
        if (lane == leader) {
            if (bad) {
                const uint32_t first = sg.block_first[theirs], count = sg.block_first[theirs + 1u] - first;
                atomicMax(sg.first_bad + theirs, count - (blockIdx.x * 64u + (uint32_t)__builtin_ctzll(bad) - first));
            }
            if (sum) atomicAdd(sg.blob_gas + theirs, sum);
        }
        todo &= ~same;
    }
    if (all_bad && lane == (uint32_t)__builtin_ctzll(all_bad)) atomicMax(dv.ctl + 1, n - i);  // the segment's least flagged index
}

// ---- the lists of the forest (segment_lists.hip.h): values 0 .. n_tx - 1 are the transactions (tries 0 .. tx_tries - 1), the
// withdrawals follow.  n_tx / tx_tries (n_wd / wd_tries) are 0 when nobody asks for that root.
struct Src {
    const uint8_t *txs, *wd;
    const uint64_t *tx_off, *wd_off;
    const uint32_t *block_first, *wd_first, *tx_block;
    uint32_t n_blocks, n_tx, n_wd, tx_tries, wd_tries;
    struct Item {
        uint32_t trie, pos, index;
        const uint8_t* src;
        uint64_t len;
    };
    // value g: its trie by bisection (a transaction's is its block, which body_tx_block_kernel has found), its position and index there
    PHANT_DEV Item item(uint32_t g) const {
        Item it;
        const bool is_tx = g < n_tx;
        const uint32_t w = is_tx ? g : g - n_tx;
        const uint32_t* const first = is_tx ? block_first : wd_first;
        const uint32_t b = is_tx ? tx_block[g] : seg::block_of(first, n_blocks, w);
        const uint32_t begin = first[b], count = first[b + 1u] - begin;
        it.trie = is_tx ? b : tx_tries + b;
        it.pos = w - begin;
        it.index = seg::index_of_pos(it.pos, count);
        const uint64_t* const off = is_tx ? tx_off : wd_off;
        const uint64_t at = off[begin + it.index];
        it.src = (is_tx ? txs : wd) + at;
        it.len = off[begin + it.index + 1u] - at;
        return it;
    }
    PHANT_DEV uint32_t trie(uint32_t t, uint32_t& count) const {
        const bool is_tx = t < tx_tries;
        const uint32_t* const first = is_tx ? block_first + t : wd_first + (t - tx_tries);
        count = first[1] - first[0];
        return (is_tx ? 0u : n_tx) + first[0];
    }
    PHANT_DEV void write(uint8_t* out, const Item& it, uint32_t lane) const { wave_copy(out, it.src, it.len, lane); }
};

__global__ void __launch_bounds__(256) body_verdict_kernel(Seg sg, uint32_t tx_tries, uint32_t wd_tries, uint32_t* __restrict__ ctl) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= sg.n_blocks) return;
    const uint32_t count = sg.block_first[b + 1u] - sg.block_first[b], rel = sg.first_bad[b];
    const unsigned long long gas = tx::GAS_PER_BLOB * sg.blob_gas[b];
    uint32_t f = rel ? (uint32_t)PHANT_BODY_TX : 0u;
    if (sg.exp_txs_root && tx_tries && seg::bytes_differ(sg.exp_txs_root + 32ull * b, sg.roots + 32ull * b, 32u)) f |= PHANT_BODY_TXS_ROOT;
    if (sg.exp_wd_root && wd_tries && seg::bytes_differ(sg.exp_wd_root + 32ull * b, sg.roots + 32ull * (tx_tries + b), 32u)) f |= PHANT_BODY_WD_ROOT;
    if (sg.exp_blob_gas && sg.exp_blob_gas[b] != gas) f |= PHANT_BODY_BLOB_GAS;
    sg.first_bad[b] = count - rel;
    sg.blob_gas[b] = gas;
    sg.block_flags[b] = f;
    if (f) atomicMax(ctl + CTL_BAD_BLOCK, sg.n_blocks - b);
}

// what the host form refuses before anything is copied (tx_off: tx::check_host)
inline int32_t check_host(const phant_bodies_in& in, std::string& err) {
    if (const int32_t rc = seg::check_firsts_host("block_bodies", "block_first", "n", in.block_first, in.n_blocks, in.n, err)) return rc;
    if (!in.wd_first) return PHANT_OK;
    if (const int32_t rc = seg::check_firsts_host("block_bodies", "wd_first", "n_wd", in.wd_first, in.n_blocks, in.n_wd, err)) return rc;
    return in.n_wd ? seg::check_offsets_host("block_bodies", "wd_off", "withdrawal", in.wd_off, in.n_wd, err) : PHANT_OK;
}

}  // namespace body

int32_t block_bodies(Workspaces& ws, hipStream_t st, const phant_bodies_in& in, phant_bodies_out& out, bool dev, const uint32_t* gtable,
                     std::string& err) {
    using namespace body;
    const uint32_t n = in.n, nb = in.n_blocks, n_wd = in.wd_first ? in.n_wd : 0u, fork = in.fork;
    const bool recover = !(in.flags & PHANT_TXS_NO_RECOVERY);
    CALL_TRY("block_bodies", ws.ensure_mailbox());
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_TXS;
    // ---- the transactions' part of the call, as phant_block_transactions_ex begins it
    phant_txs_in tin;
    std::memset(&tin, 0, sizeof tin);
    tin.n = n, tin.flags = in.flags, tin.txs = in.txs, tin.tx_off = in.tx_off, tin.tx_bytes = in.tx_bytes, tin.chain_id = in.chain_id;
    tx::Call c;
    std::memset(&c, 0, sizeof c);  // (a segment without a transaction still has its blocks' roots and flags)
    if (n)
        if (const int32_t rc = tx::call_begin(c, tin, fork, dev, err)) return rc;
    uint64_t wd_bytes = n_wd ? in.wd_bytes : 0u;
    if (!dev) {
        if (const int32_t rc = check_host(in, err)) return rc;
        wd_bytes = n_wd ? in.wd_off[n_wd] : 0u;
    }
    // which tries: a root somebody asks for or expects
    const bool want_txr = out.transactions_root || in.transactions_root, want_wdr = in.wd_first && (out.withdrawals_root || in.withdrawals_root);
    Src src;
    std::memset(&src, 0, sizeof src);
    src.n_blocks = nb, src.n_tx = want_txr ? n : 0u, src.n_wd = want_wdr ? n_wd : 0u, src.tx_tries = want_txr ? nb : 0u, src.wd_tries = want_wdr ? nb : 0u;
    const uint64_t total64 = (uint64_t)src.n_tx + src.n_wd, val_bytes = (want_txr ? c.bytes : 0u) + (want_wdr ? wd_bytes : 0u);
    if (total64 + 2ull * nb + 2u >= 0x7fffffffull) return err = "block_bodies: more than 2^31 - 2 items in one call", PHANT_E_UNSUPPORTED;
    if (val_bytes > 0xffffffffull) return err = "block_bodies: more than 4 GiB of trie values in one call", PHANT_E_UNSUPPORTED;
    seg::IndexForest p{};
    p.size((uint32_t)total64, src.tx_tries + src.wd_tries, val_bytes);

    // ---- the arena: the per-block outputs, the words to zero and the transactions' control words and outputs in front (one span goes
    // back), the internal arrays, (host form) every input in one piece, the forest's pairs last
    Seg sg;
    std::memset(&sg, 0, sizeof sg);
    sg.n_blocks = nb, sg.n = n, sg.n_wd = n_wd, sg.fork = fork;
    sg.block_first = in.block_first, sg.wd_off = in.wd_off, sg.wd_first = in.wd_first, sg.wd = in.withdrawals;
    sg.base_fee = in.base_fee, sg.blob_base_fee = in.blob_base_fee, sg.gas_limit = (in.flags & PHANT_TXS_HAVE_GAS_LIMIT) ? in.gas_limit : nullptr;
    sg.exp_txs_root = in.transactions_root, sg.exp_wd_root = in.wd_first ? in.withdrawals_root : nullptr, sg.exp_blob_gas = in.blob_gas_used;
    // (the carve runs twice, and its first run leaves null pointers behind: what is wanted is decided from `in` alone)
    const bool have_gas_limit = (in.flags & PHANT_TXS_HAVE_GAS_LIMIT) != 0u, have_exp_wd = in.wd_first && in.withdrawals_root;
    const void* inputs_end = nullptr;
    auto carve = [&](auto& io) {
        sg.tx_block = io.template take<uint32_t>((size_t)n);
        sg.roots = io.template take<uint8_t>(32 * (size_t)p.tries);
        sg.block_flags = io.template take<uint32_t>((size_t)nb);
        sg.first_bad = io.template take<uint32_t>((size_t)nb);
        sg.blob_gas = io.template take<unsigned long long>((size_t)nb);
        tx::call_carve(io, c, dev || !n);
        if (!dev) {
            take_input(io, sg.block_first, (size_t)nb + 1, true);
            take_input(io, sg.wd_first, (size_t)nb + 1, in.wd_first != nullptr);
            take_input(io, sg.wd_off, (size_t)n_wd + 1, n_wd != 0u);
            take_input(io, sg.wd, (size_t)wd_bytes, n_wd != 0u);
            take_input(io, sg.base_fee, 32 * (size_t)nb, in.base_fee != nullptr);
            take_input(io, sg.blob_base_fee, 32 * (size_t)nb, in.blob_base_fee != nullptr);
            take_input(io, sg.gas_limit, (size_t)nb, have_gas_limit);
            take_input(io, sg.exp_txs_root, 32 * (size_t)nb, in.transactions_root != nullptr);
            take_input(io, sg.exp_wd_root, 32 * (size_t)nb, have_exp_wd);
            take_input(io, sg.exp_blob_gas, (size_t)nb, in.blob_gas_used != nullptr);
            inputs_end = io.template take<uint8_t>(0);
        }
        if (p.tries) p.carve(io);
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_bodies", "workspace", err)) return rc;
    tx::Dev& d = c.d;
    CALL_TRY("block_bodies", hipMemsetAsync(sg.first_bad, 0, (size_t)(reinterpret_cast<uint8_t*>(d.ctl + tx::CTL_WORDS) - reinterpret_cast<uint8_t*>(sg.first_bad)), st));
    if (!n) CALL_TRY("block_bodies", hipMemsetAsync(d.x.auth_first, 0, 4, st));  // (its one entry; tx_decode_kernel writes it otherwise)

    // ---- in: (host form) every input in ONE copy through the pinned stage where they fit it; (device form) the offsets' check
    if (!dev) {
        StagedInputs ins(ws, st, n ? static_cast<const void*>(c.d_off) : sg.block_first, inputs_end);
        if (n) ins.put(c.d_off, in.tx_off, 8 * ((size_t)n + 1));
        if (n) ins.put(c.d_txs, in.txs, (size_t)c.bytes);
        ins.put(sg.block_first, in.block_first, 4 * ((size_t)nb + 1));
        if (in.wd_first) ins.put(sg.wd_first, in.wd_first, 4 * ((size_t)nb + 1));
        if (n_wd) ins.put(sg.wd_off, in.wd_off, 8 * ((size_t)n_wd + 1));
        if (n_wd) ins.put(sg.wd, in.withdrawals, (size_t)wd_bytes);
        ins.put(sg.base_fee, in.base_fee, 32 * (size_t)nb);
        ins.put(sg.blob_base_fee, in.blob_base_fee, 32 * (size_t)nb);
        if (have_gas_limit) ins.put(sg.gas_limit, in.gas_limit, 8 * (size_t)nb);
        ins.put(sg.exp_txs_root, in.transactions_root, 32 * (size_t)nb);
        if (have_exp_wd) ins.put(sg.exp_wd_root, in.withdrawals_root, 32 * (size_t)nb);
        ins.put(sg.exp_blob_gas, in.blob_gas_used, 8 * (size_t)nb);
        CALL_TRY("block_bodies", ins.finish());
    } else {
        const uint32_t most = std::max(std::max(n, n_wd), nb);
        hipLaunchKernelGGL(body_check_kernel, dim3(blocks_of(most, 256)), dim3(256), 0, st, c.d_off, c.bytes, sg.wd_off, wd_bytes, sg.block_first, sg.wd_first, n,
                           n_wd, nb, d.ctl);
        CALL_TRY("block_bodies", hipGetLastError());
        CALL_TRY("block_bodies", ws.read_words(Workspaces::MAILBOX_TXS, d.ctl, tx::CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID)
            return err = "block_bodies_dev: tx_off, wd_off, block_first or wd_first does not run from 0 to its total, or goes backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & seg::F_TOO_LONG) return err = "block_bodies_dev: a transaction or a withdrawal of 4 GiB or more", PHANT_E_UNSUPPORTED;
    }

    // ---- the transactions: their blocks, decode, hash, (the tuples,) ONE recovery over the segment, the rules per block
    if (n) {
        hipLaunchKernelGGL(body_tx_block_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, sg.block_first, nb, n, sg.tx_block);
        CALL_TRY("block_bodies", hipGetLastError());
        if (const int32_t rc = tx::call_kernels(ws, st, c, in.chain_id, fork, recover, gtable, err)) return rc;
        hipLaunchKernelGGL(body_rules_kernel, dim3(blocks_of(n, 64)), dim3(64), 0, st, n, sg, d, recover ? d.o.sig_status : nullptr);
        CALL_TRY("block_bodies", hipGetLastError());
    }

    // ---- the tries of all blocks: lengths, one scan, pairs, one forest pass
    if (p.tries) {
        src.txs = c.d_txs, src.tx_off = c.d_off, src.wd = sg.wd, src.wd_off = sg.wd_off;
        src.block_first = sg.block_first, src.wd_first = sg.wd_first, src.tx_block = sg.tx_block;
        CALL_TRY("block_bodies", seg::launch_forest(src, p, st));
        if (const int32_t rc = trie_forest_dev(ws, st, p.trie_pairs(sg.roots), err)) return rc;
    }
    hipLaunchKernelGGL(body_verdict_kernel, dim3(blocks_of(nb, 256)), dim3(256), 0, st, sg, src.tx_tries, src.wd_tries, d.ctl);
    CALL_TRY("block_bodies", hipGetLastError());

    // ---- out: one span from the per-block outputs through the control words up to the last wanted output
    CallOutputs outs(ws, st, dev, sg.tx_block, d.ctl, Workspaces::MAILBOX_TXS, tx::CTL_WORDS);
    static_assert(tx::CALL_OUTPUTS + 6 <= CallOutputs::CAP, "the outputs of a segment fit");
    outs.add(out.tx_block, sg.tx_block, 4 * (size_t)n);
    if (want_txr) outs.add(out.transactions_root, sg.roots, 32 * (size_t)nb);
    if (want_wdr) outs.add(out.withdrawals_root, sg.roots + 32 * (size_t)src.tx_tries, 32 * (size_t)nb);
    outs.add(out.block_flags, sg.block_flags, 4 * (size_t)nb);
    outs.add(out.block_first_bad, sg.first_bad, 4 * (size_t)nb);
    outs.add(out.block_blob_gas_used, sg.blob_gas, 8 * (size_t)nb);
    if (n) tx::call_outputs(outs, c, out.txs, in.auth_cap);
    else outs.add(out.txs.auth_first, d.x.auth_first, 4);  // (its one entry)
    CALL_TRY("block_bodies", outs.deliver());
    const volatile uint32_t* const ctl = outs.ctl();
    out.first_bad_block = nb - ctl[CTL_BAD_BLOCK];
    out.txs.base.first_bad = n - ctl[1];
    out.txs.n_auth = ctl[2];
    out.txs.blob_gas_used = tx::GAS_PER_BLOB * ((uint64_t)ctl[4] | (uint64_t)ctl[5] << 32);
    return PHANT_OK;
}

}  // namespace phant
