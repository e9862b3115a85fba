// receipt_segments.hip.h -- the receipts of a chain segment from raw messages in one call (included by bulk_keccak.hip behind
// receipts.hip.h): a strict RLP decode of every receipt and of its logs, the logs' blooms, the consensus encodings
// an eth/69 peer no longer sends, the per-block verdicts, and the receipts tries of all blocks as ONE forest pass.
//
//   rseg_check_kernel    device form only: rc_off and block_first as the caller states them, a lane per entry (segment_lists.hip.h's rules); the
//                        host reads the verdict before any other kernel indexes with them
//   rseg_decode_kernel   a lane per receipt: the head's items and the headers of its logs, never a payload; shapes validated, logs and
//                        topics counted
//   (exclusive scan)     radix_sort.hip's, over both counts at once
//   rseg_logs_kernel     a lane per receipt walks its logs again: each log's receipt, the place of its address, its first topic, its data
//   rseg_items_kernel    a lane per bloom item (an address or a topic): its bytes out, hashed, bloom_add_digest into its receipt's row
//   rseg_rows_kernel     a WAVE per receipt: the embedded bloom against the computed one (64 dwords), the gas rule, the block's bloom and
//                        its first bad row
//   (seg::launch_forest) segment_lists.hip.h's lengths, scan and pairs over rseg::Seg: a WAVE per value, copied (consensus form, or a
//                        row nobody could decode) or built (ETH69) in trie order
//   rseg_gather_kernel   ETH69, a wave per receipt: the built encoding back in index order for the caller who stores it
//   (trie_forest_dev)    one trie per block
//   rseg_verdict_kernel  a lane per block: the last gas, root, bloom, gas and count against what the header says
//
// Every offset inside a receipt is 32 bits and relative to the receipt's first byte; rlp.h's reader compares each declared length with
// what is left of the ROW before anything is added to it, so no lane reads outside [rc_off[i], rc_off[i + 1]).
// Plain C++ plus the cross-lane builtins segment_lists.hip.h uses: tests/emu.py compiles this file for the host.
#pragma once
#include "receipts.hip.h"
#include "segment_lists.hip.h"

namespace phant {
namespace rseg {

// the call's control words (device memory, zeroed): [0] = seg::F_INVALID / F_TOO_LONG of the check, [1] = n_blocks - (the least flagged
// block) or 0, [2] = n_logs, [3] = n_topics, [4] = the bytes of the consensus encodings (ETH69; below 2^32 like the call's values)
constexpr uint32_t CTL_WORDS = 8, CTL_BAD_BLOCK = 1, CTL_LOGS = 2, CTL_TOPICS = 3, CTL_ENC = 4;
// what an ETH69 receipt grows by at most when its consensus encoding is built: a type byte, 0xb9 0x01 0x00 and the bloom, a longer list header
constexpr uint64_t BUILT_GROWTH = 1u + rc::BLOOM_FIELD + 8u;
// the shortest log: 0xd7 0x94 address 0xc0 0x80; the shortest topic: 0xa0 and its 32 bytes
constexpr uint64_t MIN_LOG_BYTES = 24, TOPIC_BYTES = 33;

struct Seg {
    const uint8_t* receipts;
    const uint64_t* rc_off;
    const uint32_t* block_first;
    const uint8_t *exp_root, *exp_bloom;
    const uint64_t* exp_gas;
    const uint32_t* exp_count;
    uint32_t n_blocks, n, eth69, log_cap, topic_cap;
    // per receipt
    uint8_t *tx_type, *status;
    uint64_t *cum_gas, *gas_used;
    uint32_t* counts;   // 2 n + 2: the logs of every receipt, a zero, the topics, a zero; scanned in place: [0, n] = log_first
    uint32_t* rows;     // n x 64 dwords, zeroed: the computed blooms; null when nobody needs one
    uint32_t *dflags, *flags, *head_at, *logs_at;
    // per log
    uint32_t *log_receipt, *addr_at, *topic_first;
    uint8_t *address, *topics;
    uint64_t* data_at;
    uint32_t* data_len;
    // per block
    uint8_t* roots;
    uint32_t* block_bloom;  // n_blocks x 64 dwords, zeroed
    uint64_t* block_gas;
    uint32_t* first_bad;    // zeroed: count - (the least flagged row of the block); the verdict turns it round
    uint32_t* block_flags;
    uint32_t* ctl;
    uint8_t* enc;  // ETH69: the built encodings in index order, or null
    uint64_t* enc_off;
    uint64_t enc_cap;

    // the lists of the forest (segment_lists.hip.h; defined below): one trie per block
    struct Item {
        uint32_t trie, pos, index, row, len;
        bool built;
    };
    PHANT_DEV Item item(uint32_t g) const;
    PHANT_DEV uint32_t trie(uint32_t t, uint32_t& count) const {
        count = block_first[t + 1u] - block_first[t];
        return block_first[t];
    }
    PHANT_DEV void write(uint8_t* out, const Item& it, uint32_t lane) const;
};

// ---- the strict decode of one receipt: m = its bytes, len of them
struct Head {
    uint32_t type, status, head_at, logs_at, logs_pay, logs_len;
    uint64_t gas;
};

// the logs list's payload [at, end): every log [address(20), [topic(32) ...], data] and nothing else; each(address_at, topics, data_at,
// data_len) per log; false: malformed
template <class Each>
PHANT_DEV bool walk_logs(const MemBytes& m, uint32_t at, uint32_t end, Each&& each) {
    RlpItem lg, it;
    while (at < end) {
        if (!rlp_decode(m, at, end - at, lg) || !lg.is_list) return false;
        const uint32_t lend = lg.pay + lg.len;
        if (!rlp_decode(m, lg.pay, lg.len, it) || it.is_list || it.len != 20u) return false;
        const uint32_t addr = it.pay;
        uint32_t q = addr + 20u;
        if (!rlp_decode(m, q, lend - q, it) || !it.is_list || it.len % (uint32_t)TOPIC_BYTES) return false;
        const uint32_t topics = it.len / (uint32_t)TOPIC_BYTES;
        for (uint32_t k = 0; k < topics; ++k)  // (a 32-byte string has the one header 0xa0: the items fill the payload exactly)
            if (m.byte(it.pay + (uint32_t)TOPIC_BYTES * k) != 0xa0u) return false;
        q = it.pay + it.len;
        if (!rlp_decode(m, q, lend - q, it) || it.is_list || q + it.total != lend) return false;
        each(addr, topics, it.pay, it.len);
        at = lend;
    }
    return true;
}

PHANT_DEV bool parse_head(const MemBytes& m, uint32_t len, bool eth69, Head& h) {
    uint32_t at = 0;
    h.type = 0;
    if (!len) return false;
    if (!eth69 && m.byte(0) < 0x80u) {  // EIP-2718: a type byte 0x01 .. 0x7f in front
        if (!(h.type = m.byte(0))) return false;
        at = 1;
    }
    RlpItem o, it;
    if (!rlp_decode(m, at, len - at, o) || !o.is_list || at + o.total != len) return false;
    uint32_t q = o.pay;
    if (eth69) {  // tx_type: a canonical integer 0 .. 0x7f
        if (!rlp_decode(m, q, len - q, it) || it.is_list || it.len > 1u) return false;
        if (it.len && ((h.type = m.byte(it.pay)) == 0u || h.type > 0x7fu)) return false;
        q += it.total;
    }
    h.head_at = q;
    // status_or_root: the empty string, 0x01, or a pre-Byzantium post-state root
    if (!rlp_decode(m, q, len - q, it) || it.is_list) return false;
    if (it.len == 0u) h.status = 0;
    else if (it.len == 1u && m.byte(it.pay) == 1u) h.status = 1;
    else if (it.len == 32u) h.status = 2;
    else return false;
    q += it.total;
    // cum_gas: a canonical integer of at most 8 bytes
    if (!rlp_decode(m, q, len - q, it) || it.is_list || it.len > 8u || (it.len && m.byte(it.pay) == 0u)) return false;
    h.gas = 0;
    for (uint32_t k = 0; k < it.len; ++k) h.gas = h.gas << 8 | m.byte(it.pay + k);
    q += it.total;
    if (!eth69) {  // the bloom: 256 bytes, not read here
        if (!rlp_decode(m, q, len - q, it) || it.is_list || it.len != 256u) return false;
        q += it.total;
    }
    h.logs_at = q;
    if (!rlp_decode(m, q, len - q, it) || !it.is_list || q + it.total != len) return false;
    h.logs_pay = it.pay, h.logs_len = it.len;
    return true;
}

// bytes of the consensus encoding built from a decodable ETH69 receipt of `len` bytes: the items from the status on, the bloom between
PHANT_DEV uint64_t built_len(uint32_t type, uint32_t head_at, uint32_t len) {
    const uint64_t payload = (uint64_t)(len - head_at) + rc::BLOOM_FIELD;
    return (type ? 1u : 0u) + hdr_len(payload) + payload;
}

__global__ void __launch_bounds__(256) rseg_check_kernel(const uint64_t* __restrict__ rc_off, uint64_t rc_bytes, const uint32_t* __restrict__ block_first,
                                                         uint32_t n, uint32_t n_blocks, uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t f = 0;
    if (i < n) f |= seg::off_flags(rc_off, i, n, rc_bytes);
    if (i < n_blocks) f |= seg::first_flags(block_first, i, n_blocks, n);
    if (f) atomicOr(ctl, f);
}

__global__ void __launch_bounds__(256) rseg_decode_kernel(Seg sg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= sg.n) return;
    const uint64_t b = sg.rc_off[i];
    const uint32_t len = (uint32_t)(sg.rc_off[i + 1u] - b);  // (checked: below 4 GiB)
    const MemBytes m{sg.receipts + b};
    Head h;
    uint32_t logs = 0, topics = 0;
    const bool ok = parse_head(m, len, sg.eth69 != 0u, h) &&
                    walk_logs(m, h.logs_pay, h.logs_pay + h.logs_len, [&](uint32_t, uint32_t t, uint32_t, uint32_t) { ++logs, topics += t; });
    sg.tx_type[i] = ok ? (uint8_t)h.type : (uint8_t)0u;
    sg.status[i] = ok ? (uint8_t)h.status : (uint8_t)0u;
    sg.cum_gas[i] = ok ? h.gas : 0ull;
    sg.head_at[i] = ok ? h.head_at : 0u;
    sg.logs_at[i] = ok ? h.logs_at : 0u;
    sg.counts[i] = ok ? logs : 0u;
    sg.counts[sg.n + 1u + i] = ok ? topics : 0u;
    sg.dflags[i] = !ok ? (uint32_t)PHANT_RCPT_UNDECODABLE : h.status == 2u ? (uint32_t)PHANT_RCPT_POST_STATE : 0u;
}

// counts scanned: S[i] = the logs in front of receipt i, S[n] = S[n + 1] = all of them, S[n + 1 + i] - S[n] = the topics in front of it
PHANT_DEV uint32_t n_logs_of(const Seg& sg) { return sg.counts[sg.n]; }
PHANT_DEV uint32_t n_topics_of(const Seg& sg) { return sg.counts[2u * sg.n + 1u] - sg.counts[sg.n]; }
PHANT_DEV bool caps_hold(const Seg& sg) { return n_logs_of(sg) <= sg.log_cap && n_topics_of(sg) <= sg.topic_cap; }

__global__ void __launch_bounds__(256) rseg_logs_kernel(Seg sg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > sg.n) return;
    const uint32_t nl = n_logs_of(sg), nt = n_topics_of(sg);
    if (i == sg.n) {
        sg.ctl[CTL_LOGS] = nl, sg.ctl[CTL_TOPICS] = nt;
        if (sg.topic_first) sg.topic_first[nl] = nt;
        return;
    }
    if (!sg.topic_first || sg.counts[i + 1u] == sg.counts[i]) return;  // (nobody needs the logs; an undecodable receipt has none)
    const uint64_t b = sg.rc_off[i];
    const MemBytes m{sg.receipts + b};
    const bool rows_out = caps_hold(sg);
    const uint32_t lp = sg.logs_at[i], end = (uint32_t)(sg.rc_off[i + 1u] - b);
    RlpItem it;
    (void)rlp_decode(m, lp, end - lp, it);  // (decodable: rseg_decode_kernel has walked all of it)
    uint32_t l = sg.counts[i], t = sg.counts[sg.n + 1u + i] - nl;
    (void)walk_logs(m, it.pay, it.pay + it.len, [&](uint32_t addr, uint32_t topics, uint32_t data, uint32_t data_len) {
        sg.log_receipt[l] = i;
        sg.addr_at[l] = (uint32_t)b + addr;  // (the call's bytes are fewer than 2^32)
        sg.topic_first[l] = t;
        if (rows_out && sg.data_at) sg.data_at[l] = b + data;
        if (rows_out && sg.data_len) sg.data_len[l] = data_len;
        ++l, t += topics;
    });
}

// bloom item k < n_logs: log k's address; the others: topic k - n_logs, 33 bytes apart behind the topics list's header
__global__ void __launch_bounds__(256) rseg_items_kernel(Seg sg) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, nl = n_logs_of(sg), nt = n_topics_of(sg);
    if (k >= nl + nt) return;
    const bool is_addr = k < nl;
    const uint32_t t = is_addr ? 0u : k - nl;
    const uint32_t l = is_addr ? k : upper_bound(sg.topic_first, nl + 1u, t) - 1u;
    const uint32_t len = is_addr ? 20u : 32u;
    const uint8_t* p = sg.receipts + sg.addr_at[l];
    if (!is_addr) p += 20u + hdr_len(TOPIC_BYTES * (sg.topic_first[l + 1u] - sg.topic_first[l])) + (uint32_t)TOPIC_BYTES * (t - sg.topic_first[l]) + 1u;
    uint8_t* const out = is_addr ? sg.address : sg.topics;
    if (out && caps_hold(sg))
        for (uint32_t j = 0; j < len; ++j) out[(uint64_t)len * (is_addr ? l : t) + j] = p[j];
    if (!sg.rows) return;
    Sponge s;
    keccak256_global(s, p, len);
    bloom_add_digest(s, sg.rows + 64ull * sg.log_receipt[l]);
}

__global__ void __launch_bounds__(256) rseg_rows_kernel(Seg sg) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= sg.n) return;
    const uint32_t b = seg::block_of(sg.block_first, sg.n_blocks, i), first = sg.block_first[b];
    const uint32_t df = sg.dflags[i];
    const bool ok = !(df & PHANT_RCPT_UNDECODABLE);
    uint32_t f = df;
    if (sg.rows) {
        const uint32_t w = sg.rows[64ull * i + lane];
        if (w) atomicOr(&sg.block_bloom[64ull * b + lane], w);
        bool differs = false;
        if (ok && !sg.eth69) {  // the embedded bloom: the 256 bytes in front of the logs
            const uint8_t* const e = sg.receipts + sg.rc_off[i] + sg.logs_at[i] - 256u + 4u * lane;
            differs = w != ((uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24);
        }
        if (__ballot(differs)) f |= PHANT_RCPT_BLOOM;
    }
    if (lane != 0u) return;
    const bool has_prev = i > first;
    const uint64_t gas = sg.cum_gas[i], prev = has_prev ? sg.cum_gas[i - 1u] : 0ull;  // (an undecodable row's is 0)
    if (ok && (has_prev ? !(sg.dflags[i - 1u] & PHANT_RCPT_UNDECODABLE) && gas <= prev : gas == 0ull)) f |= PHANT_RCPT_GAS_ORDER;
    sg.gas_used[i] = ok ? gas - prev : 0ull;
    sg.flags[i] = f;
    if (sg.eth69) {  // the bytes the caller's `encoded` must hold: known whether or not a value is built
        const uint32_t raw = (uint32_t)(sg.rc_off[i + 1u] - sg.rc_off[i]);
        atomicAdd(sg.ctl + CTL_ENC, ok ? (uint32_t)built_len(sg.tx_type[i], sg.head_at[i], raw) : raw);
    }
    if (f & PHANT_RCPT_ERROR_BITS) atomicMax(sg.first_bad + b, sg.block_first[b + 1u] - i);  // = count - (i - first)
}

// ---- value g of the forest: its block, its position and index there, copied or built
PHANT_DEV Seg::Item Seg::item(uint32_t g) const {
    Item it;
    it.trie = seg::block_of(block_first, n_blocks, g);
    const uint32_t begin = block_first[it.trie], count = block_first[it.trie + 1u] - begin;
    it.pos = g - begin;
    it.index = seg::index_of_pos(it.pos, count);
    it.row = begin + it.index;
    const uint32_t raw = (uint32_t)(rc_off[it.row + 1u] - rc_off[it.row]);
    it.built = eth69 && !(dflags[it.row] & PHANT_RCPT_UNDECODABLE);
    it.len = it.built ? (uint32_t)built_len(tx_type[it.row], head_at[it.row], raw) : raw;  // (the call's values were bounded below 2^32)
    return it;
}

PHANT_DEV void Seg::write(uint8_t* out, const Item& it, uint32_t lane) const {
    const uint8_t* const src = receipts + rc_off[it.row];
    const uint32_t raw = (uint32_t)(rc_off[it.row + 1u] - rc_off[it.row]);
    if (!it.built) return wave_copy(out, src, raw, lane);
    // [tx_type, when != 0] ++ list header ++ status and gas as they stand ++ 0xb9 0x01 0x00 ++ bloom ++ the logs as they stand
    const uint32_t type = tx_type[it.row], head = head_at[it.row], logs = logs_at[it.row];
    const uint64_t payload = (uint64_t)(raw - head) + rc::BLOOM_FIELD;
    const uint32_t at_head = (type ? 1u : 0u) + hdr_len(payload), at_bloom = at_head + (logs - head) + 3u;
    if (lane == 0u) {
        if (type) out[0] = (uint8_t)type;
        (void)put_hdr(out + (type ? 1u : 0u), 0xc0u, payload);
        out[at_bloom - 3u] = 0xb9u, out[at_bloom - 2u] = 0x01u, out[at_bloom - 1u] = 0x00u;
    }
    wave_copy(out + at_head, src + head, logs - head, lane);
    const uint32_t w = rows[64ull * it.row + lane];
    uint8_t* const bl = out + at_bloom + 4u * lane;
    bl[0] = (uint8_t)w, bl[1] = (uint8_t)(w >> 8), bl[2] = (uint8_t)(w >> 16), bl[3] = (uint8_t)(w >> 24);
    wave_copy(out + at_bloom + 256u, src + logs, raw - logs, lane);
}

// the values back in index order (receipts.hip.h's rc_gather_kernel per block): nothing is written when they exceed enc_cap
__global__ void __launch_bounds__(256) rseg_gather_kernel(Seg sg, seg::IndexForest a) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i > sg.n || a.val_off[sg.n] > sg.enc_cap) return;
    if (i == sg.n) {
        if (lane == 0u && sg.enc_off) sg.enc_off[i] = a.val_off[i];
        return;
    }
    const uint32_t b = seg::block_of(sg.block_first, sg.n_blocks, i), first = sg.block_first[b], count = sg.block_first[b + 1u] - first;
    const uint32_t k = count < 128u ? count : 128u, j = i - first;
    const uint64_t* const vo = a.val_off + first;
    const uint64_t base = vo[0], len0 = vo[k] - vo[k - 1u];  // index 0 sits at position k - 1
    const uint64_t at = j == 0u ? base : j < k ? vo[j - 1u] + len0 : vo[j];
    const uint32_t p = seg::pos_of_index(j, count);
    if (sg.enc_off && lane == 0u) sg.enc_off[i] = at;
    if (sg.enc) wave_copy(sg.enc + at, a.vals + vo[p], vo[p + 1u] - vo[p], lane);
}

__global__ void __launch_bounds__(256) rseg_verdict_kernel(Seg sg, uint32_t have_roots) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= sg.n_blocks) return;
    const uint32_t first = sg.block_first[b], count = sg.block_first[b + 1u] - first, rel = sg.first_bad[b];
    uint64_t gas = 0;  // the last decodable row's
    for (uint32_t i = first + count; i > first; --i)
        if (!(sg.dflags[i - 1u] & PHANT_RCPT_UNDECODABLE)) {
            gas = sg.cum_gas[i - 1u];
            break;
        }
    uint32_t f = rel ? (uint32_t)PHANT_RBLOCK_RECEIPT : 0u;
    if (sg.exp_root && have_roots && seg::bytes_differ(sg.exp_root + 32ull * b, sg.roots + 32ull * b, 32u)) f |= PHANT_RBLOCK_ROOT;
    if (sg.exp_bloom && seg::bytes_differ(sg.exp_bloom + 256ull * b, reinterpret_cast<const uint8_t*>(sg.block_bloom + 64ull * b), 256u)) f |= PHANT_RBLOCK_BLOOM;
    if (sg.exp_gas && sg.exp_gas[b] != gas) f |= PHANT_RBLOCK_GAS_USED;
    if (sg.exp_count && sg.exp_count[b] != count) f |= PHANT_RBLOCK_COUNT;
    sg.first_bad[b] = count - rel;
    sg.block_gas[b] = gas;
    sg.block_flags[b] = f;
    if (f) atomicMax(sg.ctl + CTL_BAD_BLOCK, sg.n_blocks - b);
}

// what the host form refuses before anything is copied
inline int32_t check_host(const phant_rcpt_segs_in& in, std::string& err) {
    if (const int32_t rc = seg::check_firsts_host("block_receipt_segments", "block_first", "n", in.block_first, in.n_blocks, in.n, err)) return rc;
    return in.n ? seg::check_offsets_host("block_receipt_segments", "rc_off", "receipt", in.rc_off, in.n, err) : PHANT_OK;
}

}  // namespace rseg

int32_t block_receipt_segments(Workspaces& ws, hipStream_t st, const phant_rcpt_segs_in& in, phant_rcpt_segs_out& out, bool dev, std::string& err) {
    using namespace rseg;
    const uint32_t n = in.n, nb = in.n_blocks;
    const bool eth69 = in.form == PHANT_RCPTS_ETH69;
    CALL_TRY("block_receipt_segments", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_RSEG_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_RSEG;
    uint64_t bytes = n ? in.rc_bytes : 0u;
    if (!dev) {
        if (const int32_t rc = check_host(in, err)) return rc;
        bytes = n ? in.rc_off[n] : 0u;
    }
    // ---- what is wanted: a trie for a root somebody asks for or expects; values also for the encodings an ETH69 caller stores; a bloom for
    // PHANT_RCPT_BLOOM (consensus form: always), for a built value and for the bloom outputs; the logs for a bloom and for their own rows
    const bool want_root = out.receipts_root || in.receipts_root, want_enc = out.encoded || out.encoded_off;
    const bool want_vals = want_root || (eth69 && want_enc);
    const bool want_bloom = !eth69 || want_vals || out.bloom || out.logs_bloom || in.logs_bloom;
    const bool want_log_rows = out.log_receipt || out.address || out.topic_first || out.topics || out.data_at || out.data_len;
    const bool want_logs = want_bloom || want_log_rows;
    const uint64_t val_bytes = bytes + (eth69 ? BUILT_GROWTH * n : 0u);
    if (2ull * n + 2ull * nb + 4u >= 0x7fffffffull) return err = "block_receipt_segments: more than 2^31 - 2 items in one call", PHANT_E_UNSUPPORTED;
    if (val_bytes > 0xffffffffull) return err = "block_receipt_segments: more than 4 GiB of receipts or trie values in one call", PHANT_E_UNSUPPORTED;
    const size_t log_bound = want_logs ? (size_t)(bytes / MIN_LOG_BYTES) : 0u, topic_bound = want_logs ? (size_t)(bytes / TOPIC_BYTES) : 0u;
    const size_t log_rows = std::min<size_t>(log_bound, in.log_cap), topic_rows = std::min<size_t>(topic_bound, in.topic_cap);
    seg::IndexForest p{};
    p.size(want_vals ? n : 0u, want_vals ? nb : 0u, val_bytes);
    const uint32_t count_n = 2u * n + 2u;
    const bool gather = eth69 && want_enc;

    // ---- the arena: the control words and everything to zero in front, the outputs behind them (one span goes back), the internal
    // arrays, (host form) every input in one piece, the forest's pairs last
    Seg sg;
    std::memset(&sg, 0, sizeof sg);
    sg.n_blocks = nb, sg.n = n, sg.eth69 = eth69 ? 1u : 0u, sg.log_cap = in.log_cap, sg.topic_cap = in.topic_cap;
    sg.receipts = in.receipts, sg.rc_off = in.rc_off, sg.block_first = in.block_first;
    sg.exp_root = in.receipts_root, sg.exp_bloom = in.logs_bloom, sg.exp_gas = in.gas_used, sg.exp_count = in.tx_count;
    sg.enc_cap = out.encoded ? out.encoded_cap : ~0ull;
    uint32_t* d_scan = nullptr;
    const void *zero_end = nullptr, *outputs_end = nullptr, *inputs_begin = nullptr, *inputs_end = nullptr;
    auto carve = [&](auto& io) {
        sg.ctl = io.template take<uint32_t>(CTL_WORDS);
        sg.first_bad = io.template take<uint32_t>((size_t)nb);
        sg.block_bloom = io.template take<uint32_t>(64 * (size_t)nb);
        sg.counts = io.template take<uint32_t>((size_t)count_n + 4);
        if (want_bloom) sg.rows = io.template take<uint32_t>(64 * (size_t)n);
        zero_end = io.template take<uint8_t>(0);
        sg.roots = io.template take<uint8_t>(32 * (size_t)p.tries);
        sg.block_gas = io.template take<uint64_t>((size_t)nb);
        sg.block_flags = io.template take<uint32_t>((size_t)nb);
        sg.tx_type = io.template take<uint8_t>((size_t)n);
        sg.status = io.template take<uint8_t>((size_t)n);
        sg.cum_gas = io.template take<uint64_t>((size_t)n);
        sg.gas_used = io.template take<uint64_t>((size_t)n);
        sg.flags = io.template take<uint32_t>((size_t)n);
        if (want_logs) {
            sg.log_receipt = io.template take<uint32_t>(log_bound + 1);
            sg.topic_first = io.template take<uint32_t>(log_bound + 1);
            if (out.address) sg.address = io.template take<uint8_t>(20 * log_rows);
            if (out.topics) sg.topics = io.template take<uint8_t>(32 * topic_rows);
            if (out.data_at) sg.data_at = io.template take<uint64_t>(log_rows);
            if (out.data_len) sg.data_len = io.template take<uint32_t>(log_rows);
        }
        if (gather) {
            sg.enc_off = io.template take<uint64_t>((size_t)n + 1);
            if (out.encoded) sg.enc = io.template take<uint8_t>((size_t)std::min<uint64_t>(val_bytes, out.encoded_cap) + 16);
        }
        outputs_end = io.template take<uint8_t>(0);
        sg.dflags = io.template take<uint32_t>((size_t)n);
        sg.head_at = io.template take<uint32_t>((size_t)n);
        sg.logs_at = io.template take<uint32_t>((size_t)n);
        d_scan = io.template take<uint32_t>(scan_scratch_entries(count_n));
        if (want_logs) sg.addr_at = io.template take<uint32_t>(log_bound + 1);
        if (!dev) {
            inputs_begin = io.template take<uint8_t>(0);
            take_input(io, sg.rc_off, (size_t)n + 1, n != 0u);
            take_input(io, sg.receipts, (size_t)bytes, n != 0u);
            take_input(io, sg.block_first, (size_t)nb + 1, true);
            take_input(io, sg.exp_root, 32 * (size_t)nb, in.receipts_root != nullptr);
            take_input(io, sg.exp_bloom, 256 * (size_t)nb, in.logs_bloom != nullptr);
            take_input(io, sg.exp_gas, (size_t)nb, in.gas_used != nullptr);
            take_input(io, sg.exp_count, (size_t)nb, in.tx_count != nullptr);
            inputs_end = io.template take<uint8_t>(0);
        }
        if (want_vals) p.carve(io);
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_receipt_segments", "workspace", err)) return rc;
    CALL_TRY("block_receipt_segments", hipMemsetAsync(sg.ctl, 0, (size_t)(static_cast<const uint8_t*>(zero_end) - reinterpret_cast<uint8_t*>(sg.ctl)), st));

    // ---- in: (host form) every input in ONE copy through the pinned stage where they fit it; (device form) the offsets' check
    if (!dev) {
        StagedInputs ins(ws, st, inputs_begin, inputs_end);
        if (n) ins.put(sg.rc_off, in.rc_off, 8 * ((size_t)n + 1));
        if (n) ins.put(sg.receipts, in.receipts, (size_t)bytes);
        ins.put(sg.block_first, in.block_first, 4 * ((size_t)nb + 1));
        ins.put(sg.exp_root, in.receipts_root, 32 * (size_t)nb);
        ins.put(sg.exp_bloom, in.logs_bloom, 256 * (size_t)nb);
        ins.put(sg.exp_gas, in.gas_used, 8 * (size_t)nb);
        ins.put(sg.exp_count, in.tx_count, 4 * (size_t)nb);
        CALL_TRY("block_receipt_segments", ins.finish());
    } else {
        hipLaunchKernelGGL(rseg_check_kernel, dim3(blocks_of(std::max(n, nb), 256)), dim3(256), 0, st, sg.rc_off, bytes, sg.block_first, n, nb, sg.ctl);
        CALL_TRY("block_receipt_segments", hipGetLastError());
        CALL_TRY("block_receipt_segments", ws.read_words(Workspaces::MAILBOX_RSEG, sg.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID)
            return err = "block_receipt_segments_dev: rc_off or block_first does not run from 0 to its total, or goes backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & seg::F_TOO_LONG) return err = "block_receipt_segments_dev: a receipt of 4 GiB or more", PHANT_E_UNSUPPORTED;
    }

    // ---- the receipts: decode, one scan over both counts, the logs' rows, the bloom items, the rows
    if (n) {
        hipLaunchKernelGGL(rseg_decode_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, sg);
        CALL_TRY("block_receipt_segments", hipGetLastError());
        CALL_TRY("block_receipt_segments", launch_exclusive_scan_u32(sg.counts, count_n, d_scan, st));
        hipLaunchKernelGGL(rseg_logs_kernel, dim3(blocks_of((uint64_t)n + 1, 256)), dim3(256), 0, st, sg);
        // (a lane per item the segment CAN hold at most would be a grid sized by the bytes; the items are counted on the device, so the
        // grid covers what the caps or the bytes allow and the kernel's own bound does the rest)
        if (want_logs) hipLaunchKernelGGL(rseg_items_kernel, dim3(blocks_of((uint64_t)log_bound + topic_bound + 1, 256)), dim3(256), 0, st, sg);
        hipLaunchKernelGGL(rseg_rows_kernel, dim3(blocks_of(n, 4)), dim3(256), 0, st, sg);
        CALL_TRY("block_receipt_segments", hipGetLastError());
    }

    // ---- the tries of all blocks: lengths, one scan, pairs, one forest pass; the built encodings back in index order
    if (want_vals) {
        CALL_TRY("block_receipt_segments", seg::launch_forest(sg, p, st));
        if (gather) hipLaunchKernelGGL(rseg_gather_kernel, dim3(blocks_of((uint64_t)n + 1, 4)), dim3(256), 0, st, sg, p);
        CALL_TRY("block_receipt_segments", hipGetLastError());
        if (want_root)
            if (const int32_t rc = trie_forest_dev(ws, st, p.trie_pairs(sg.roots), err)) return rc;
    }
    hipLaunchKernelGGL(rseg_verdict_kernel, dim3(blocks_of(nb, 256)), dim3(256), 0, st, sg, want_root ? 1u : 0u);
    CALL_TRY("block_receipt_segments", hipGetLastError());

    // ---- out: one span from the control words to the last output; the rows whose count only the control words tell follow them
    CallOutputs outs(ws, st, dev, sg.ctl, sg.ctl, Workspaces::MAILBOX_RSEG, CTL_WORDS);
    if (!dev) outs.cover(outputs_end);
    outs.add(out.block_first_bad, sg.first_bad, 4 * (size_t)nb);
    outs.add(out.logs_bloom, sg.block_bloom, 256 * (size_t)nb);
    outs.add(out.log_first, sg.counts, 4 * ((size_t)n + 1));
    if (want_bloom) outs.add(out.bloom, sg.rows, 256 * (size_t)n);
    if (want_root) outs.add(out.receipts_root, sg.roots, 32 * (size_t)nb);
    outs.add(out.block_gas_used, sg.block_gas, 8 * (size_t)nb);
    outs.add(out.block_flags, sg.block_flags, 4 * (size_t)nb);
    outs.add(out.tx_type, sg.tx_type, (size_t)n);
    outs.add(out.status, sg.status, (size_t)n);
    outs.add(out.cum_gas, sg.cum_gas, 8 * (size_t)n);
    outs.add(out.gas_used, sg.gas_used, 8 * (size_t)n);
    outs.add(out.flags, sg.flags, 4 * (size_t)n);
    CALL_TRY("block_receipt_segments", outs.deliver());
    const volatile uint32_t* const ctl = outs.ctl();
    const uint32_t nl = ctl[CTL_LOGS], nt = ctl[CTL_TOPICS];
    out.first_bad_block = nb - ctl[CTL_BAD_BLOCK];
    out.n_logs = nl, out.n_topics = nt;
    out.encoded_len = eth69 ? ctl[CTL_ENC] : bytes;
    if (want_log_rows && nl <= in.log_cap && nt <= in.topic_cap) {
        outs.add(out.log_receipt, sg.log_receipt, 4 * (size_t)nl);
        outs.add(out.topic_first, sg.topic_first, 4 * ((size_t)nl + 1));
        outs.add(out.address, sg.address, 20 * (size_t)nl);
        outs.add(out.topics, sg.topics, 32 * (size_t)nt);
        outs.add(out.data_at, sg.data_at, 8 * (size_t)nl);
        outs.add(out.data_len, sg.data_len, 4 * (size_t)nl);
    }
    if (want_enc && out.encoded_len <= sg.enc_cap) {
        if (gather) {
            outs.add(out.encoded, sg.enc, (size_t)out.encoded_len);
            outs.add(out.encoded_off, sg.enc_off, 8 * ((size_t)n + 1));
        } else if (dev) {  // the consensus form's encodings are the input
            outs.add(out.encoded, const_cast<uint8_t*>(in.receipts), (size_t)bytes);
            outs.add(out.encoded_off, const_cast<uint64_t*>(in.rc_off), 8 * ((size_t)n + 1));
        } else {
            if (out.encoded && bytes) std::memcpy(out.encoded, in.receipts, (size_t)bytes);
            if (out.encoded_off && n) std::memcpy(out.encoded_off, in.rc_off, 8 * ((size_t)n + 1));
            else if (out.encoded_off) out.encoded_off[0] = 0;
        }
    }
    CALL_TRY("block_receipt_segments", outs.deliver());
    return PHANT_OK;
}

}  // namespace phant
