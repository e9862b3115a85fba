// requests.hip.h -- the execution requests of a chain segment in one call (included by bulk_keccak.hip behind receipt_segments.hip.h;
// DESIGN.md section 7s): the deposit requests (EIP-6110) rebuilt from the logs block_receipt_segments leaves decoded, and every block's
// requests_hash (EIP-7685) computed with SHA-256 (sha256.hip.h) and held against its header's.
//
// Definitions (include/phant_gpu.h has the contract, tests/requests_ref.py the same in Python):
//   candidate     a log of an active block whose address is deposit_contract (20 bytes), with at least one topic, the first of them
//                 649bbc62...38c5 = keccak256("DepositEvent(bytes,bytes,bytes,bytes,bytes)")
//   well-formed   data_len == 576, [data_at, data_at + 576) inside [0, rc_bytes), the 32-byte big-endian words at 0, 32, 64, 96, 128 exactly
//                 160, 256, 320, 384, 512 and those at 160, 256, 320, 384, 512 exactly 48, 32, 8, 96, 8
//   row           192 bytes: data[192:240] ++ data[288:320] ++ data[352:360] ++ data[416:512] ++ data[544:552]
//   a candidate that is not well-formed: no row, PHANT_QBLOCK_DEPOSIT_LAYOUT on its block
//   a block's requests   type 0 = its rows in log order when it has one, then the caller's rows with data in the order given
//   requests_hash        sha256(sha256(type_0 ++ data_0) ++ sha256(type_1 ++ data_1) ++ ...); nothing at all: sha256("")
//
//   qreq_check_kernel     device form only: the firsts and offsets as the caller states them, a lane per entry (segment_lists.hip.h's
//                         rules); the host reads the verdict before any other kernel indexes with them
//   qreq_classify_kernel  a lane per log: its block, the address and the first topic, the layout; a good bit per log, the block's flag
//                         by atomic OR
//   (exclusive scan)      radix_sort.hip's over the good bits: each good log's row
//   qreq_gather_kernel    16 lanes per log, 12 of them move 16 bytes of the row each (unaligned 16-byte loads -- data_at has no
//                         alignment --, aligned stores), one writes deposit_log; behind the logs a lane per block: deposit_first
//   qreq_inner_kernel     a lane per (block, type 0) and per caller's row: sha256_stream over the type byte and the rows or the caller's
//                         bytes into the block's slots
//   qreq_outer_kernel     a lane per block: its present digests moved together and hashed, the types' order, the verdict
//
// Five launches, the scan's among them (the device form's check is a sixth), whatever n_blocks and n_logs are.  A call is as long as its longest message: a deposit is 192 bytes = three
// compressions, serial in the one lane that hashes its block's type-0 request.
// Plain C++ plus the builtins sha256.hip.h uses: tests/emu.py compiles this file for the host.
#pragma once
#include "requests_check.h"
#include "segment_lists.hip.h"
#include "sha256.hip.h"
#include "staging.h"

namespace phant {
namespace qreq {

// the call's control words (device memory, zeroed): [0] = seg::F_INVALID / F_TOO_LONG of the check, [1] = n_blocks - (the least flagged
// block) or 0, [2] = n_deposits
constexpr uint32_t CTL_WORDS = 4, CTL_BAD_BLOCK = 1, CTL_DEPOSITS = 2;
constexpr uint32_t EVENT_BYTES = 576, ROW_BYTES = 192;

__constant__ uint8_t DEPOSIT_EVENT_TOPIC[32] = {0x64, 0x9b, 0xbc, 0x62, 0xd0, 0xe3, 0x13, 0x42, 0xaf, 0xea, 0x4e, 0x5c, 0xd8, 0x2d, 0x40, 0x49,
                                                0xe7, 0xe1, 0xee, 0x91, 0x2f, 0xc0, 0x88, 0x9a, 0xa7, 0x90, 0x80, 0x3b, 0xe3, 0x90, 0x38, 0xc5};

struct Req {
    const uint8_t* receipts;
    uint64_t rc_bytes, req_total;
    const uint32_t *block_first, *log_first, *topic_first, *data_len, *req_block_first;
    const uint8_t *address, *topics, *req_type, *req_bytes, *active, *exp_hash;
    const uint64_t *data_at, *req_off;
    uint32_t n_blocks, n, n_logs, n_topics, n_req;
    uint8_t contract[20];
    uint32_t* ctl;
    uint32_t* block_flags;  // zeroed
    uint32_t* good;         // n_logs + 1, zeroed: 1 for a well-formed candidate; scanned in place: a log's row, [n_logs] = n_deposits
    uint32_t *deposit_first, *deposit_log;
    uint8_t *rows, *hashes;
    uint8_t* inner;    // (n_blocks + n_req) x 32: block b's digests from slot b + req_block_first[b] on, type 0 first
    uint8_t* present;  // a byte per slot

    PHANT_DEV bool is_active(uint32_t b) const { return !active || active[b] != 0u; }
    PHANT_DEV uint32_t req_first(uint32_t b) const { return n_req ? req_block_first[b] : 0u; }
};

// the 32-byte big-endian word at p is exactly v < 2^16
PHANT_DEV bool word_is(const uint8_t* p, uint32_t v) {
    const PackedU32x4 a = *reinterpret_cast<const PackedU32x4*>(p), b = *reinterpret_cast<const PackedU32x4*>(p + 16);
    return (a.x | a.y | a.z | a.w | b.x | b.y | b.z) == 0u && b.w == __builtin_bswap32(v);
}

PHANT_DEV bool well_formed(const Req& q, uint32_t l) {
    const uint64_t at = q.data_at[l];
    if (q.data_len[l] != EVENT_BYTES || at > q.rc_bytes || q.rc_bytes - at < EVENT_BYTES) return false;
    const uint8_t* const d = q.receipts + at;
    return word_is(d, 160u) && word_is(d + 32, 256u) && word_is(d + 64, 320u) && word_is(d + 96, 384u) && word_is(d + 128, 512u) &&
           word_is(d + 160, 48u) && word_is(d + 256, 32u) && word_is(d + 320, 8u) && word_is(d + 384, 96u) && word_is(d + 512, 8u);
}

__global__ void __launch_bounds__(256) qreq_check_kernel(Req q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t f = 0;
    if (i < q.n_blocks) f |= seg::first_flags(q.block_first, i, q.n_blocks, q.n);
    if (i < q.n) f |= seg::first_flags(q.log_first, i, q.n, q.n_logs);
    if (i < q.n_logs) f |= seg::first_flags(q.topic_first, i, q.n_logs, q.n_topics);
    if (q.n_req && i < q.n_blocks) f |= seg::first_flags(q.req_block_first, i, q.n_blocks, q.n_req);
    if (i < q.n_req) f |= seg::off_flags(q.req_off, i, q.n_req, q.req_total);
    if (f) atomicOr(q.ctl, f);
}

__global__ void __launch_bounds__(256) qreq_classify_kernel(Req q) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= q.n_logs) return;
    const uint32_t b = seg::block_of(q.block_first, q.n_blocks, upper_bound(q.log_first, q.n + 1u, l) - 1u);
    if (!q.is_active(b)) return;
    if (seg::bytes_differ(q.address + 20ull * l, q.contract, 20u)) return;
    const uint32_t t = q.topic_first[l];
    if (q.topic_first[l + 1u] == t || seg::bytes_differ(q.topics + 32ull * t, DEPOSIT_EVENT_TOPIC, 32u)) return;
    if (well_formed(q, l)) q.good[l] = 1u;
    else atomicOr(q.block_flags + b, (uint32_t)PHANT_QBLOCK_DEPOSIT_LAYOUT);
}

// where the 8 bytes at 8 u of a row come from in the event's data: pubkey (6 of them), credentials (4), amount, signature (12), index
PHANT_DEV uint32_t unit_source(uint32_t u) { return u < 6u ? 192u + 8u * u : u < 10u ? 288u + 8u * (u - 6u) : u == 10u ? 352u : u < 23u ? 416u + 8u * (u - 11u) : 544u; }

__global__ void __launch_bounds__(256) qreq_gather_kernel(Req q) {
    const uint64_t t = blockIdx.x * 256ull + threadIdx.x, per_log = 16ull * q.n_logs;
    if (t >= per_log) {  // a lane per block and one more: deposit_first
        const uint64_t b = t - per_log;
        if (b <= q.n_blocks) q.deposit_first[b] = q.good[q.n ? q.log_first[q.block_first[b]] : 0u];
        if (b == q.n_blocks) q.ctl[CTL_DEPOSITS] = q.good[q.n_logs];
        return;
    }
    const uint32_t l = (uint32_t)(t >> 4), c = (uint32_t)t & 15u, row = q.good[l];
    if (q.good[l + 1u] == row || c > 12u) return;
    if (c == 12u) {
        q.deposit_log[row] = l;
        return;
    }
    const uint8_t* const d = q.receipts + q.data_at[l];
    const uint32_t s0 = unit_source(2u * c), s1 = unit_source(2u * c + 1u);
    uint4 v;
    if (s1 == s0 + 8u) {
        const PackedU32x4 x = *reinterpret_cast<const PackedU32x4*>(d + s0);
        v = make_uint4(x.x, x.y, x.z, x.w);
    } else {  // (the chunks that straddle amount | signature and signature | index)
        const PackedU32x2 x = *reinterpret_cast<const PackedU32x2*>(d + s0), y = *reinterpret_cast<const PackedU32x2*>(d + s1);
        v = make_uint4(x.x, x.y, y.x, y.y);
    }
    *reinterpret_cast<uint4*>(q.rows + (uint64_t)ROW_BYTES * row + 16u * c) = v;  // (the arena's rows: 16-byte aligned)
}

__global__ void __launch_bounds__(256) qreq_inner_kernel(Req q) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= q.n_blocks + q.n_req) return;
    uint32_t slot, type;
    const uint8_t *p, *end;
    uint64_t len;
    bool there;
    if (g < q.n_blocks) {  // the block's deposits
        const uint32_t first = q.deposit_first[g];
        slot = g + q.req_first(g), type = 0u;
        len = (uint64_t)ROW_BYTES * (q.deposit_first[g + 1u] - first);
        p = q.rows + (uint64_t)ROW_BYTES * first, end = q.rows + (uint64_t)ROW_BYTES * q.good[q.n_logs];
        there = len != 0u;  // (an inactive block has no rows)
    } else {  // a caller's row
        const uint32_t r = g - q.n_blocks, b = seg::block_of(q.req_block_first, q.n_blocks, r);
        const uint64_t at = q.req_off[r];
        slot = b + 1u + r, type = q.req_type[r];
        len = q.req_off[r + 1u] - at;
        p = q.req_bytes + at, end = q.req_bytes + q.req_off[q.n_req];
        there = len != 0u && q.is_active(b);
    }
    q.present[slot] = there ? 1u : 0u;
    if (!there) return;
    uint32_t h[8];
    sha::sha256_stream(true, type, p, len, end, h);
    sha::store_bytes(h, q.inner + 32ull * slot);
}

__global__ void __launch_bounds__(256) qreq_outer_kernel(Req q) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= q.n_blocks) return;
    uint8_t* const out = q.hashes + 32ull * b;
    if (!q.is_active(b)) {  // before the fork: a zero hash, no flags
        for (uint32_t k = 0; k < 32u; ++k) out[k] = 0u;
        return;
    }
    const uint32_t r0 = q.req_first(b), r1 = q.req_first(b + 1u), s0 = b + r0, s1 = b + 1u + r1;
    uint32_t w = s0;  // the present digests moved together, in place
    for (uint32_t s = s0; s < s1; ++s) {
        if (!q.present[s]) continue;
        if (s != w)
            for (uint32_t k = 0; k < 32u; ++k) q.inner[32ull * w + k] = q.inner[32ull * s + k];
        ++w;
    }
    uint32_t h[8];
    sha::sha256_stream(false, 0u, q.inner + 32ull * s0, 32ull * (w - s0), q.inner + 32ull * (q.n_blocks + q.n_req), h);
    sha::store_bytes(h, out);
    uint32_t f = q.block_flags[b], prev = 0u;  // (the classify kernel's OR is complete: it ran before)
    for (uint32_t r = r0; r < r1; ++r) {      // 1 .. 255, strictly ascending: a type 0 is not above its predecessor either
        const uint32_t t = q.req_type[r];
        if (t <= prev) f |= PHANT_QBLOCK_ORDER;
        prev = t;
    }
    if (q.exp_hash && seg::bytes_differ(q.exp_hash + 32ull * b, out, 32u)) f |= PHANT_QBLOCK_HASH;
    q.block_flags[b] = f;
    if (f) atomicMax(q.ctl + CTL_BAD_BLOCK, q.n_blocks - b);
}

}  // namespace qreq

int32_t block_requests(Workspaces& ws, hipStream_t st, const phant_requests_in& in, phant_requests_out& out, bool dev, std::string& err) {
    using namespace qreq;
    const uint32_t nb = in.n_blocks, n = in.n, nl = in.n_logs, nt = in.n_topics, nr = in.n_req;
    CALL_TRY("block_requests", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_QREQ_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_QREQ;
    if (!dev)
        if (const int32_t rc = check_host(in, err)) return rc;
    const uint64_t req_bytes = !nr ? 0u : dev ? in.req_total : in.req_off[nr];
    if ((uint64_t)nb + nr + 1u >= 0x7fffffffull || (uint64_t)nl + 1u >= 0x7fffffffull / 16u)
        return err = "block_requests: more than 2^31 - 2 blocks and rows, or 2^27 - 2 logs, in one call", PHANT_E_UNSUPPORTED;
    // (a row per log at most: hand-made logs may state the same data more than once, so the bytes do not bound the rows)
    const size_t row_cap = nl, slots = (size_t)nb + nr;

    // ---- the arena: the control words and everything to zero in front, the outputs behind them (one span goes back), the internal
    // arrays, (host form) every input in one piece
    Req q;
    std::memset(&q, 0, sizeof q);
    q.n_blocks = nb, q.n = n, q.n_logs = nl, q.n_topics = nt, q.n_req = nr, q.rc_bytes = in.rc_bytes, q.req_total = req_bytes;
    q.receipts = in.receipts, q.block_first = in.block_first, q.log_first = in.log_first, q.address = in.address, q.topic_first = in.topic_first;
    q.topics = in.topics, q.data_at = in.data_at, q.data_len = in.data_len, q.req_block_first = in.req_block_first, q.req_type = in.req_type;
    q.req_bytes = in.req_bytes, q.req_off = in.req_off, q.active = in.active, q.exp_hash = in.requests_hash;
    std::memcpy(q.contract, in.deposit_contract, 20);
    uint32_t* d_scan = nullptr;
    const void *zero_end = nullptr, *outputs_end = nullptr, *inputs_begin = nullptr, *inputs_end = nullptr;
    auto carve = [&](auto& io) {
        q.ctl = io.template take<uint32_t>(CTL_WORDS);
        q.block_flags = io.template take<uint32_t>((size_t)nb);
        q.good = io.template take<uint32_t>((size_t)nl + 1 + 4);
        zero_end = io.template take<uint8_t>(0);
        q.deposit_first = io.template take<uint32_t>((size_t)nb + 1);
        q.hashes = io.template take<uint8_t>(32 * (size_t)nb);
        q.deposit_log = io.template take<uint32_t>(row_cap);
        q.rows = io.template take<uint8_t>(ROW_BYTES * row_cap + 16);
        outputs_end = io.template take<uint8_t>(0);
        q.inner = io.template take<uint8_t>(32 * slots + 16);
        q.present = io.template take<uint8_t>(slots);
        d_scan = io.template take<uint32_t>(scan_scratch_entries(nl + 1u));
        if (!dev) {
            inputs_begin = io.template take<uint8_t>(0);
            take_input(io, q.receipts, (size_t)in.rc_bytes, in.rc_bytes != 0u);
            take_input(io, q.block_first, (size_t)nb + 1, true);
            take_input(io, q.log_first, (size_t)n + 1, n != 0u);
            take_input(io, q.address, 20 * (size_t)nl, nl != 0u);
            take_input(io, q.topic_first, (size_t)nl + 1, nl != 0u);
            take_input(io, q.topics, 32 * (size_t)nt, nt != 0u);
            take_input(io, q.data_at, (size_t)nl, nl != 0u);
            take_input(io, q.data_len, (size_t)nl, nl != 0u);
            take_input(io, q.req_block_first, (size_t)nb + 1, nr != 0u);
            take_input(io, q.req_type, (size_t)nr, nr != 0u);
            take_input(io, q.req_bytes, (size_t)req_bytes, req_bytes != 0u);
            take_input(io, q.req_off, (size_t)nr + 1, nr != 0u);
            take_input(io, q.active, (size_t)nb, in.active != nullptr);
            take_input(io, q.exp_hash, 32 * (size_t)nb, in.requests_hash != nullptr);
            inputs_end = io.template take<uint8_t>(0);
        }
    };
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, carve), "block_requests", "workspace", err)) return rc;
    CALL_TRY("block_requests", hipMemsetAsync(q.ctl, 0, (size_t)(static_cast<const uint8_t*>(zero_end) - reinterpret_cast<uint8_t*>(q.ctl)), st));

    // ---- in: (host form) every input in ONE copy through the pinned stage where they fit it; (device form) the check
    if (!dev) {
        StagedInputs ins(ws, st, inputs_begin, inputs_end);
        ins.put(q.receipts, in.receipts, (size_t)in.rc_bytes);
        ins.put(q.block_first, in.block_first, 4 * ((size_t)nb + 1));
        if (n) ins.put(q.log_first, in.log_first, 4 * ((size_t)n + 1));
        if (nl) {
            ins.put(q.address, in.address, 20 * (size_t)nl);
            ins.put(q.topic_first, in.topic_first, 4 * ((size_t)nl + 1));
            ins.put(q.topics, in.topics, 32 * (size_t)nt);
            ins.put(q.data_at, in.data_at, 8 * (size_t)nl);
            ins.put(q.data_len, in.data_len, 4 * (size_t)nl);
        }
        if (nr) {
            ins.put(q.req_block_first, in.req_block_first, 4 * ((size_t)nb + 1));
            ins.put(q.req_type, in.req_type, (size_t)nr);
            ins.put(q.req_bytes, in.req_bytes, (size_t)req_bytes);
            ins.put(q.req_off, in.req_off, 8 * ((size_t)nr + 1));
        }
        ins.put(q.active, in.active, (size_t)nb);
        ins.put(q.exp_hash, in.requests_hash, 32 * (size_t)nb);
        CALL_TRY("block_requests", ins.finish());
    } else {
        hipLaunchKernelGGL(qreq_check_kernel, dim3(blocks_of(std::max(std::max(nb, n), std::max(nl, nr)), 256)), dim3(256), 0, st, q);
        CALL_TRY("block_requests", hipGetLastError());
        CALL_TRY("block_requests", ws.read_words(Workspaces::MAILBOX_QREQ, q.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID)
            return err = "block_requests_dev: block_first, log_first, topic_first, req_block_first or req_off does not run from 0 to its total, or goes backwards",
                   PHANT_E_INVALID_ARG;
        if (mb[0] & seg::F_TOO_LONG) return err = "block_requests_dev: a request of 4 GiB or more", PHANT_E_UNSUPPORTED;
    }

    // ---- the deposits: classify, one scan, the rows; then the hashes.  Every kernel is launched whatever the counts are.
    hipLaunchKernelGGL(qreq_classify_kernel, dim3(blocks_of((uint64_t)nl + 1, 256)), dim3(256), 0, st, q);
    CALL_TRY("block_requests", hipGetLastError());
    CALL_TRY("block_requests", launch_exclusive_scan_u32(q.good, nl + 1u, d_scan, st));
    hipLaunchKernelGGL(qreq_gather_kernel, dim3(blocks_of(16ull * nl + nb + 1u, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(qreq_inner_kernel, dim3(blocks_of(slots, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(qreq_outer_kernel, dim3(blocks_of(nb, 256)), dim3(256), 0, st, q);
    CALL_TRY("block_requests", hipGetLastError());

    // ---- out: one span from the control words to the last output; the rows whose count only the control words tell follow them
    CallOutputs outs(ws, st, dev, q.ctl, q.ctl, Workspaces::MAILBOX_QREQ, CTL_WORDS);
    if (!dev) outs.cover(outputs_end);
    outs.add(out.block_flags, q.block_flags, 4 * (size_t)nb);
    outs.add(out.deposit_first, q.deposit_first, 4 * ((size_t)nb + 1));
    outs.add(out.requests_hash, q.hashes, 32 * (size_t)nb);
    CALL_TRY("block_requests", outs.deliver());
    const volatile uint32_t* const ctl = outs.ctl();
    out.n_deposits = ctl[CTL_DEPOSITS];
    out.first_bad_block = nb - ctl[CTL_BAD_BLOCK];
    if (out.n_deposits <= in.deposit_cap) {
        outs.add(out.deposit_log, q.deposit_log, 4 * (size_t)out.n_deposits);
        outs.add(out.deposit, q.rows, ROW_BYTES * (size_t)out.n_deposits);
    }
    CALL_TRY("block_requests", outs.deliver());
    return PHANT_OK;
}

}  // namespace phant
