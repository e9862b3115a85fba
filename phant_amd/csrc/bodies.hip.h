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
//   body_len_kernel       a lane per trie value (its length, in trie order) and per trie (its keys' bytes, its first value)
//   (exclusive scan)      radix_sort.hip's, over both at once
//   body_pairs_kernel     a WAVE per value: its offset, its key rlp(index) and that key's offset, its bytes from index order into
//                         trie order (receipts.hip.h's position functions)
//   (trie_forest_dev)     all lists of the segment, tries 0 .. n_blocks - 1 the transactions, the withdrawals behind them
//   body_verdict_kernel   a lane per block: roots and blob gas against what the header says, block_flags, the least bad block
//
// Plain C++ plus the cross-lane builtins keyed_table.hip.h uses: tests/emu.py compiles this file for the host.
#pragma once
#include <type_traits>

#include "receipts.hip.h"
#include "transactions.hip.h"
#include "trie_build.h"
#include "wave_util.hip.h"

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

// 64-bit offsets from 0 to `bytes`, never backwards, no item of 4 GiB; 32-bit firsts from 0 to `total`, never backwards
PHANT_DEV uint32_t off_flags(const uint64_t* __restrict__ off, uint32_t i, uint32_t n, uint64_t bytes) {
    const uint64_t b = off[i], e = off[i + 1u];
    if (e < b || (i == 0u && b != 0u) || (i + 1u == n && e != bytes)) return tx::F_INVALID;
    return e - b > 0xffffffffull ? (uint32_t)tx::F_TOO_LONG : 0u;
}
PHANT_DEV uint32_t first_flags(const uint32_t* __restrict__ first, uint32_t i, uint32_t n, uint32_t total) {
    const uint32_t b = first[i], e = first[i + 1u];
    return e < b || (i == 0u && b != 0u) || (i + 1u == n && e != total) ? (uint32_t)tx::F_INVALID : 0u;
}

__global__ void __launch_bounds__(256) body_check_kernel(const uint64_t* __restrict__ tx_off, uint64_t tx_bytes, const uint64_t* __restrict__ wd_off,
                                                         uint64_t wd_bytes, const uint32_t* __restrict__ block_first,
                                                         const uint32_t* __restrict__ wd_first, uint32_t n, uint32_t n_wd, uint32_t n_blocks,
                                                         uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t f = 0;
    if (i < n) f |= off_flags(tx_off, i, n, tx_bytes);
    if (i < n_wd) f |= off_flags(wd_off, i, n_wd, wd_bytes);
    if (i < n_blocks) f |= first_flags(block_first, i, n_blocks, n);
    if (i < n_blocks && wd_first) f |= first_flags(wd_first, i, n_blocks, n_wd);
    if (f) atomicOr(ctl, f);
}

__global__ void __launch_bounds__(256) body_tx_block_kernel(const uint32_t* __restrict__ block_first, uint32_t n_blocks, uint32_t n,
                                                            uint32_t* __restrict__ tx_block) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) tx_block[i] = upper_bound(block_first, n_blocks + 1u, i) - 1u;  // (block_first[n_blocks] = n > i)
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

// ---- the index-keyed pairs of the forest: values 0 .. n_tx - 1 are the transactions (tries 0 .. tx_tries - 1), the withdrawals
// follow; each list in trie order.  n_tx / tx_tries (n_wd / wd_tries) are 0 when nobody asks for that root.
struct Pairs {
    const uint8_t *txs, *wd;
    const uint64_t *tx_off, *wd_off;
    const uint32_t *block_first, *wd_first, *tx_block;
    uint32_t n_blocks, n_tx, n_wd, tx_tries, wd_tries;
    uint32_t total, tries;  // n_tx + n_wd, tx_tries + wd_tries
    uint32_t* len;          // total + 1 lengths of values, then tries + 1 of the tries' keys; scanned in place
    uint32_t* seg_first;    // tries + 1
    uint32_t* key_off;
    uint64_t* val_off;
    uint8_t *keys, *vals;
    uint64_t key_cap, val_cap;
};
struct Item {
    uint32_t trie, pos, index;
    const uint8_t* src;
    uint64_t len;
};
// value g: its trie by bisection (a transaction's is its block, which body_tx_block_kernel has found), its position and index there
PHANT_DEV Item item_of(const Pairs& a, uint32_t g) {
    Item it;
    const bool is_tx = g < a.n_tx;
    const uint32_t w = is_tx ? g : g - a.n_tx;
    const uint32_t* const first = is_tx ? a.block_first : a.wd_first;
    const uint32_t b = is_tx ? a.tx_block[g] : upper_bound(first, a.n_blocks + 1u, w) - 1u;
    const uint32_t begin = first[b], count = first[b + 1u] - begin;
    it.trie = is_tx ? b : a.tx_tries + b;
    it.pos = w - begin;
    it.index = rc::index_of_pos(it.pos, count);
    const uint64_t* const off = is_tx ? a.tx_off : a.wd_off;
    const uint64_t at = off[begin + it.index];
    it.src = (is_tx ? a.txs : a.wd) + at;
    it.len = off[begin + it.index + 1u] - at;
    return it;
}

__global__ void __launch_bounds__(256) body_len_kernel(Pairs a) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > a.total + 1u + a.tries) return;
    uint32_t v = 0;
    if (g < a.total) {
        v = (uint32_t)item_of(a, g).len;  // (checked: below 4 GiB)
    } else if (g > a.total) {
        const uint32_t t = g - a.total - 1u;
        if (t == a.tries) {
            a.seg_first[t] = a.total;
        } else {
            const bool is_tx = t < a.tx_tries;
            const uint32_t* const first = is_tx ? a.block_first : a.wd_first;
            const uint32_t b = is_tx ? t : t - a.tx_tries;
            a.seg_first[t] = (is_tx ? 0u : a.n_tx) + first[b];
            v = rc::key_bytes_before(first[b + 1u] - first[b]);
        }
    }
    a.len[g] = v;
}

// len scanned: S[g] = the bytes of the values in front of g; S[total] = S[total + 1] = all of them; S[total + 1 + t] - S[total] = the bytes
// of the keys of the tries in front of t (modulo 2^32, which the difference undoes)
__global__ void __launch_bounds__(256) body_pairs_kernel(Pairs a) {
    const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (g > a.total) return;
    const uint32_t all = a.len[a.total];
    if (g == a.total) {
        if (lane == 0u) a.val_off[g] = all, a.key_off[g] = a.len[a.total + 1u + a.tries] - all;
        return;
    }
    const Item it = item_of(a, g);
    const uint32_t at = a.len[g], ko = a.len[a.total + 1u + it.trie] - all + rc::key_bytes_before(it.pos);
    if ((uint64_t)ko + 5u > a.key_cap || (uint64_t)at + it.len > a.val_cap) return;  // (cannot happen: both arrays are sized from the same rules)
    if (lane == 0u) {
        a.val_off[g] = at, a.key_off[g] = ko;
        (void)put_uint(a.keys + ko, it.index);
    }
    wave_copy(a.vals + at, it.src, it.len, lane);
}

__global__ void __launch_bounds__(256) body_verdict_kernel(Seg sg, uint32_t tx_tries, uint32_t wd_tries, uint32_t* __restrict__ ctl) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= sg.n_blocks) return;
    const uint32_t count = sg.block_first[b + 1u] - sg.block_first[b], rel = sg.first_bad[b];
    const unsigned long long gas = tx::GAS_PER_BLOB * sg.blob_gas[b];
    uint32_t f = rel ? (uint32_t)PHANT_BODY_TX : 0u;
    auto differs = [](const uint8_t* x, const uint8_t* y) {
        uint32_t d = 0;
        for (uint32_t k = 0; k < 32u; ++k) d |= (uint32_t)(x[k] ^ y[k]);
        return d != 0u;
    };
    if (sg.exp_txs_root && tx_tries && differs(sg.exp_txs_root + 32ull * b, sg.roots + 32ull * b)) f |= PHANT_BODY_TXS_ROOT;
    if (sg.exp_wd_root && wd_tries && differs(sg.exp_wd_root + 32ull * b, sg.roots + 32ull * (tx_tries + b))) f |= PHANT_BODY_WD_ROOT;
    if (sg.exp_blob_gas && sg.exp_blob_gas[b] != gas) f |= PHANT_BODY_BLOB_GAS;
    sg.first_bad[b] = count - rel;
    sg.blob_gas[b] = gas;
    sg.block_flags[b] = f;
    if (f) atomicMax(ctl + CTL_BAD_BLOCK, sg.n_blocks - b);
}

// what the host form refuses before anything is copied (tx_off: tx::check_host)
inline int32_t check_host(const phant_bodies_in& in, std::string& err) {
    const uint32_t nb = in.n_blocks;
    if (in.block_first[0] != 0u || in.block_first[nb] != in.n) return err = "block_bodies: block_first does not run from 0 to n", PHANT_E_INVALID_ARG;
    for (uint32_t b = 0; b < nb; ++b)
        if (in.block_first[b + 1u] < in.block_first[b]) return err = "block_bodies: block_first goes backwards", PHANT_E_INVALID_ARG;
    if (!in.wd_first) return PHANT_OK;
    if (in.wd_first[0] != 0u || in.wd_first[nb] != in.n_wd) return err = "block_bodies: wd_first does not run from 0 to n_wd", PHANT_E_INVALID_ARG;
    for (uint32_t b = 0; b < nb; ++b)
        if (in.wd_first[b + 1u] < in.wd_first[b]) return err = "block_bodies: wd_first goes backwards", PHANT_E_INVALID_ARG;
    if (!in.n_wd) return PHANT_OK;
    if (in.wd_off[0] != 0u) return err = "block_bodies: wd_off does not run from 0", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < in.n_wd; ++i)
        if (in.wd_off[i + 1u] < in.wd_off[i]) return err = "block_bodies: wd_off goes backwards", PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < in.n_wd; ++i)
        if (in.wd_off[i + 1u] - in.wd_off[i] > 0xffffffffull) return err = "block_bodies: a withdrawal of 4 GiB or more", PHANT_E_UNSUPPORTED;
    return PHANT_OK;
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
    Pairs p;
    std::memset(&p, 0, sizeof p);
    p.n_blocks = nb, p.n_tx = want_txr ? n : 0u, p.n_wd = want_wdr ? n_wd : 0u, p.tx_tries = want_txr ? nb : 0u, p.wd_tries = want_wdr ? nb : 0u;
    const uint64_t total64 = (uint64_t)p.n_tx + p.n_wd, val_bytes = (want_txr ? c.bytes : 0u) + (want_wdr ? wd_bytes : 0u);
    if (total64 + 2ull * nb + 2u >= 0x7fffffffull) return err = "block_bodies: more than 2^31 - 2 items in one call", PHANT_E_UNSUPPORTED;
    if (val_bytes > 0xffffffffull) return err = "block_bodies: more than 4 GiB of trie values in one call", PHANT_E_UNSUPPORTED;
    p.total = (uint32_t)total64, p.tries = p.tx_tries + p.wd_tries;
    p.key_cap = (uint64_t)rc::key_bytes_before(p.total) + 16u, p.val_cap = val_bytes;
    const uint32_t scan_n = p.total + 1u + p.tries + 1u;

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
    uint32_t* d_scan = nullptr;
    const void* inputs_end = nullptr;
    auto input = [&](auto& io, auto*& member, size_t count, bool wanted) {
        using T = std::remove_cv_t<std::remove_pointer_t<std::remove_reference_t<decltype(member)>>>;
        if (wanted) member = io.template take<T>(count + (sizeof(T) == 1 ? 16 : 0));
    };
    auto carve = [&](auto& io) {
        sg.tx_block = io.template take<uint32_t>((size_t)n);
        sg.roots = io.template take<uint8_t>(32 * (size_t)p.tries);
        sg.block_flags = io.template take<uint32_t>((size_t)nb);
        sg.first_bad = io.template take<uint32_t>((size_t)nb);
        sg.blob_gas = io.template take<unsigned long long>((size_t)nb);
        tx::call_carve(io, c, dev || !n);
        if (!dev) {
            input(io, sg.block_first, (size_t)nb + 1, true);
            input(io, sg.wd_first, (size_t)nb + 1, in.wd_first != nullptr);
            input(io, sg.wd_off, (size_t)n_wd + 1, n_wd != 0u);
            input(io, sg.wd, (size_t)wd_bytes, n_wd != 0u);
            input(io, sg.base_fee, 32 * (size_t)nb, in.base_fee != nullptr);
            input(io, sg.blob_base_fee, 32 * (size_t)nb, in.blob_base_fee != nullptr);
            input(io, sg.gas_limit, (size_t)nb, have_gas_limit);
            input(io, sg.exp_txs_root, 32 * (size_t)nb, in.transactions_root != nullptr);
            input(io, sg.exp_wd_root, 32 * (size_t)nb, have_exp_wd);
            input(io, sg.exp_blob_gas, (size_t)nb, in.blob_gas_used != nullptr);
            inputs_end = io.template take<uint8_t>(0);
        }
        if (p.tries) {
            p.len = io.template take<uint32_t>((size_t)scan_n + 4);
            d_scan = io.template take<uint32_t>(scan_scratch_entries(scan_n));
            p.seg_first = io.template take<uint32_t>((size_t)p.tries + 1);
            p.key_off = io.template take<uint32_t>((size_t)p.total + 1);
            p.val_off = io.template take<uint64_t>((size_t)p.total + 1);
            p.keys = io.template take<uint8_t>((size_t)p.key_cap);
            p.vals = io.template take<uint8_t>((size_t)p.val_cap + 16);
        }
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
        if (mb[0] & tx::F_INVALID)
            return err = "block_bodies_dev: tx_off, wd_off, block_first or wd_first does not run from 0 to its total, or goes backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & tx::F_TOO_LONG) return err = "block_bodies_dev: a transaction or a withdrawal of 4 GiB or more", PHANT_E_UNSUPPORTED;
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
        p.txs = c.d_txs, p.tx_off = c.d_off, p.wd = sg.wd, p.wd_off = sg.wd_off;
        p.block_first = sg.block_first, p.wd_first = sg.wd_first, p.tx_block = sg.tx_block;
        hipLaunchKernelGGL(body_len_kernel, dim3(blocks_of(scan_n, 256)), dim3(256), 0, st, p);
        CALL_TRY("block_bodies", hipGetLastError());
        CALL_TRY("block_bodies", launch_exclusive_scan_u32(p.len, scan_n, d_scan, st));
        hipLaunchKernelGGL(body_pairs_kernel, dim3(blocks_of((uint64_t)p.total + 1, 4)), dim3(256), 0, st, p);
        CALL_TRY("block_bodies", hipGetLastError());
        const int32_t rc = trie_forest_dev(ws, st, TriePairs{p.keys, p.key_off, p.key_cap, p.vals, p.val_off, p.val_cap, p.total, p.seg_first, p.tries, sg.roots}, err);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(body_verdict_kernel, dim3(blocks_of(nb, 256)), dim3(256), 0, st, sg, p.tx_tries, p.wd_tries, d.ctl);
    CALL_TRY("block_bodies", hipGetLastError());

    // ---- out: one span from the per-block outputs through the control words up to the last wanted output
    CallOutputs outs(ws, st, dev, sg.tx_block, d.ctl, Workspaces::MAILBOX_TXS, tx::CTL_WORDS);
    static_assert(tx::CALL_OUTPUTS + 6 <= CallOutputs::CAP, "the outputs of a segment fit");
    outs.add(out.tx_block, sg.tx_block, 4 * (size_t)n);
    if (want_txr) outs.add(out.transactions_root, sg.roots, 32 * (size_t)nb);
    if (want_wdr) outs.add(out.withdrawals_root, sg.roots + 32 * (size_t)p.tx_tries, 32 * (size_t)nb);
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
