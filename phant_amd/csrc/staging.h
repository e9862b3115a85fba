// staging.h -- how a call crosses the bus, once, for the drivers that keep their arrays in the ctx's `io` arena:
// block_receipts, block_receipt_segments, header_chain, block_transactions, block_txs_prestate, block_settle, and the host forms of the trie hasher and of its prover.  Plain
// host C++ on top of arena.h.
//
//   lay_out_arena an arena sized by, then carved by, one list of take<T>() calls
//   take_input    one of those takes: a host-form input array, where it is wanted
//   StagedInputs  the host form's arrays on their way in: ONE copy through the pinned stage, or a copy each
//   stage_pairs   a forest's sorted pairs in host memory: validated, laid out, rebased and sent in through StagedInputs
//   CallOutputs   every output named once; deliver() hands them back as the call's form asks
//   CALL_TRY      a HIP call of a block-level driver: its failure is the driver's PHANT_E_DEVICE with the call's text in err
//
// The pinned stage mirrors the first STAGE_BYTES of `io`.  It is used when the bytes in question END within it and the arena does not
// poison its padding (a copy of a span crosses the padding between sub-allocations; a sanitizer build therefore copies array by array,
// exact bytes only), and only by calls that end in a stream synchronisation: the next call overwrites it.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "../../include/phant_gpu.h"
#include "arena.h"
#include "trie_build.h"

// a HIP call inside the driver `name`, which has `std::string& err` and returns a PHANT_E_* code: "<name>: <call text>: <hip error string>"
#define CALL_TRY(name, call)                                                    \
    do {                                                                        \
        const hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                                 \
            err = std::string(name ": " #call ": ") + hipGetErrorString(e_);    \
            return PHANT_E_DEVICE;                                              \
        }                                                                       \
    } while (0)

namespace phant {

// ---- layout
struct LaidOut {
    enum What { OK, SYNC_FAILED, OOM, UNDERSIZED } what = OK;
    hipError_t e = hipSuccess;
};
// `carve(arena)` makes the call's take<T>() calls: once against a counter, which sizes the arena, then against the arena itself, whose
// previous contents are dropped.  The stream is synchronised before the arena grows (a kernel may still read the one that is about to
// go) unless the caller knows it to be idle.  UNDERSIZED is a sizing bug upstream: never a kernel or a copy on memory behind the
// allocation.
template <class Carve>
LaidOut lay_out_arena(DevArena& arena, hipStream_t st, Carve&& carve, bool stream_idle = false) {
    ArenaSizer size;
    carve(size);
    if (size.bytes > arena.cap && !stream_idle) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return {LaidOut::SYNC_FAILED, e};
    }
    const hipError_t e = arena.reset(size.bytes);
    if (e != hipSuccess) return {LaidOut::OOM, e};
    carve(arena);
    return {arena.overflowed ? LaidOut::UNDERSIZED : LaidOut::OK, hipSuccess};
}
// ... as the drivers report it: PHANT_OK, or the code with `call`: ... in err (`what`: the arena's name in the out-of-memory text)
inline int32_t lay_out_status(const LaidOut& r, const char* call, const char* what, std::string& err) {
    if (r.what == LaidOut::OK) return PHANT_OK;
    if (r.what == LaidOut::UNDERSIZED) return err = std::string(call) + ": arena sized too small (internal)", PHANT_E_DEVICE;
    err = std::string(call) + (r.what == LaidOut::OOM ? ": hipMalloc(" + std::string(what) + "): " : ": hipStreamSynchronize(st): ") + hipGetErrorString(r.e);
    return r.what == LaidOut::OOM ? PHANT_E_OOM : PHANT_E_DEVICE;
}

// a host-form input's place in the arena, when `wanted`: count elements, and behind bytes the 16 spare ones their readers may touch
template <class IO, class T>
void take_input(IO& io, const T*& member, size_t count, bool wanted) {
    if (wanted) member = io.template take<T>(count + (sizeof(T) == 1 ? 16 : 0));
}

// ---- in, host form: the inputs lie in [begin, end) of ws.io.  Whether the caller must synchronise after finish() is the caller's
// decision: an unstaged put() reads `src` when the stream gets there, so a source that does not outlive the call (block_receipts' host
// vectors) needs it, the caller's own arrays do not.
struct StagedInputs {
    Workspaces& ws;
    const hipStream_t st;
    uint8_t *const begin, *const end;
    const bool staged;
    hipError_t e;  // the first error; nothing is copied behind it

    StagedInputs(Workspaces& w, hipStream_t s, const void* b, const void* en)
        : ws(w), st(s), begin(static_cast<uint8_t*>(const_cast<void*>(b))), end(static_cast<uint8_t*>(const_cast<void*>(en))),
          staged(!PHANT_ARENA_POISONS && (size_t)(end - w.io.base) <= Workspaces::STAGE_BYTES), e(staged ? w.ensure_stage() : hipSuccess) {}
    void put(const void* dst, const void* src, size_t bytes) {
        if (!bytes || !src || e != hipSuccess) return;
        uint8_t* const d = static_cast<uint8_t*>(const_cast<void*>(dst));
        if (staged) memcpy(ws.staged(d), src, bytes);
        else e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st);
    }
    // where to WRITE an array that no host array holds yet (offsets rebased on the way): the pinned twin of dst, or nullptr when the
    // call is not staged -- the caller then makes the array and put()s it
    template <class T>
    T* twin(T* dst) const {
        return staged && e == hipSuccess ? ws.staged(dst) : nullptr;
    }
    hipError_t finish() {
        if (e == hipSuccess && staged && end > begin) e = hipMemcpyAsync(begin, ws.staged(begin), (size_t)(end - begin), hipMemcpyHostToDevice, st);
        return e;
    }
};

// ---- in, host-form pairs: the one way in for trie_forest_host and the prover's prove_host.  Validates `h` (then `check_more()`: the
// caller's further inputs; nothing is laid out or copied behind a refusal), lays ws.io out as the five input arrays followed by
// whatever `carve_more(arena)` takes -- it returns the end of the caller's further INPUTS, which it takes first, or nullptr --, writes
// the pairs with their offsets rebased to 0 (in place in the pinned mirror when staged: no host allocation), lets `put_more(ins)` add
// the caller's inputs and sends everything in.  -> the device view to launch on (roots left to the caller) and whether it was staged.
struct StagedPairs {
    int32_t rc = PHANT_OK;
    bool staged = false;
    TriePairs pairs;
};
template <class Check, class Carve, class Put>
StagedPairs stage_pairs(Workspaces& ws, hipStream_t st, const HostPairs& h, const char* call, std::string& err, Check&& check_more, Carve&& carve_more,
                        Put&& put_more) {
    auto refuse = [&](int32_t rc, const char* why) { return err = why, StagedPairs{rc, false, TriePairs{}}; };
    const uint32_t n = h.n, one[2] = {0, n};
    const uint32_t* const seg = h.seg_first || h.n_tries != 1 ? h.seg_first : one;
    for (uint32_t i = 0; i < n; ++i) {
        if (h.key_off[i + 1] < h.key_off[i] || h.val_off[i + 1] < h.val_off[i]) return refuse(PHANT_E_INVALID_ARG, "offsets not monotone");
        if (h.key_off[i + 1] - h.key_off[i] > 255) return refuse(PHANT_E_UNSUPPORTED, "key longer than 255 bytes");
    }
    for (uint32_t s = 0; s < h.n_tries; ++s)
        if (seg[s] > seg[s + 1] || seg[s + 1] > n) return refuse(PHANT_E_INVALID_ARG, "seg_first not monotone");
    if (seg[0] != 0 || seg[h.n_tries] != n) return refuse(PHANT_E_INVALID_ARG, "seg_first must span [0, n]");
    StagedPairs r;
    if ((r.rc = check_more()) != PHANT_OK) return r;
    const uint32_t k0 = n ? h.key_off[0] : 0u;
    const uint64_t v0 = n ? h.val_off[0] : 0u, kb = n ? h.key_off[n] - k0 : 0u, vb = n ? h.val_off[n] - v0 : 0u;
    uint8_t *d_keys = nullptr, *d_vals = nullptr;
    const void* end = nullptr;
    uint32_t *d_koff = nullptr, *d_seg = nullptr;
    uint64_t* d_voff = nullptr;
    r.rc = lay_out_status(lay_out_arena(ws.io, st, [&](auto& io) {
        d_keys = io.template take<uint8_t>(kb + 16);
        d_koff = io.template take<uint32_t>((size_t)n + 1);
        d_vals = io.template take<uint8_t>(vb + 16);
        d_voff = io.template take<uint64_t>((size_t)n + 1);
        d_seg = io.template take<uint32_t>((size_t)h.n_tries + 1);
        end = carve_more(io);
    }), call, "io", err);
    if (r.rc != PHANT_OK) return r;
    StagedInputs ins(ws, st, d_keys, end ? end : d_seg + h.n_tries + 1);
    ins.put(d_keys, kb ? h.keys + k0 : nullptr, kb);
    ins.put(d_vals, vb ? h.vals + v0 : nullptr, vb);
    std::vector<uint32_t> ko;
    std::vector<uint64_t> vo;
    uint32_t* rel_k = ins.twin(d_koff);
    uint64_t* rel_v = ins.twin(d_voff);
    if (!ins.staged) {  // (pageable sources: hipMemcpyAsync has taken its copy of them when put() returns)
        ko.resize((size_t)n + 1);
        vo.resize((size_t)n + 1);
        rel_k = ko.data(), rel_v = vo.data();
    }
    if (rel_k && rel_v) {
        rel_k[0] = 0, rel_v[0] = 0;
        for (uint32_t i = 0; i <= n && n; ++i) rel_k[i] = h.key_off[i] - k0, rel_v[i] = h.val_off[i] - v0;
    }
    if (!ins.staged) ins.put(d_koff, rel_k, ((size_t)n + 1) * 4), ins.put(d_voff, rel_v, ((size_t)n + 1) * 8);
    ins.put(d_seg, seg, ((size_t)h.n_tries + 1) * 4);
    put_more(ins);
    const hipError_t e = ins.finish();
    if (e != hipSuccess) {
        err = std::string(call) + ": staging the pairs: " + hipGetErrorString(e);
        r.rc = e == hipErrorOutOfMemory ? PHANT_E_OOM : PHANT_E_DEVICE;
        return r;
    }
    r.staged = ins.staged;
    r.pairs = TriePairs{d_keys, d_koff, kb, d_vals, d_voff, vb, n, d_seg, h.n_tries, nullptr};
    return r;
}

// ---- out: add() names an output once (a NULL caller pointer or no bytes: nobody wants it), deliver() hands back what was added since
// the last deliver():
//   device form        a device-to-device copy each, then the control words into the mailbox (one copy, one synchronisation)
//   host form, staged  ONE copy of [span, the end of the last output inside `io`) into the pinned stage, a synchronisation, memcpys
//   host form, plain   a copy each, then the control words into the mailbox (without control words: the synchronisation alone)
// An output outside the fetched span -- in another arena, or added after the first deliver() and behind the span, like encodings whose
// size only the control words tell -- gets a copy of its own in every form; a later deliver() synchronises the host form when it made one.
// A call without control words leaves mailbox_words at 0; ctl() is valid after the first deliver().
struct CallOutputs {
    static constexpr int CAP = 48;  // block_transactions names 35, block_bodies 41, block_receipt_segments 20
    struct Item {
        void* dst;
        const uint8_t* src;
        size_t bytes;
    };
    Workspaces& ws;
    const hipStream_t st;
    const bool dev;
    const uint8_t* const span;  // where the one copy back begins: the control words, or the first output
    const uint8_t* span_end;
    const uint32_t* const d_ctl;
    const size_t mailbox_at, mailbox_words;
    Item item[CAP];
    int n = 0, done = 0;
    bool overflow = false, delivered = false, staged = false;

    CallOutputs(Workspaces& w, hipStream_t s, bool device_form, const void* span_begin, const uint32_t* ctl = nullptr, size_t mb_at = 0, size_t mb_words = 0)
        : ws(w), st(s), dev(device_form), span(static_cast<const uint8_t*>(span_begin)), span_end(span), d_ctl(ctl), mailbox_at(mb_at),
          mailbox_words(mb_words) {
        if (mb_words && !dev) cover(ctl + mb_words);
    }
    // the span reaches at least up to here (bytes the kernels wrote: they cross the bus whether anybody wants them or not)
    void cover(const void* end) {
        if (!delivered && static_cast<const uint8_t*>(end) > span_end) span_end = static_cast<const uint8_t*>(end);
    }
    void add(void* dst, const void* src, size_t bytes) {
        if (!dst || !bytes) return;
        if (n == CAP) {
            overflow = true;
            return;
        }
        const uint8_t* const s = static_cast<const uint8_t*>(src);
        item[n++] = Item{dst, s, bytes};
        if (s >= ws.io.base && s < ws.io.base + ws.io.used) cover(s + bytes);
    }
    const volatile uint32_t* ctl() const { return staged ? ws.staged(d_ctl) : ws.mailbox + mailbox_at; }
    hipError_t deliver() {
        if (overflow) return hipErrorInvalidValue;
        const bool first = !delivered;
        delivered = true;
        hipError_t e = hipSuccess;
        if (dev) {
            for (; done < n && e == hipSuccess; ++done) e = hipMemcpyAsync(item[done].dst, item[done].src, item[done].bytes, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && first && mailbox_words) e = ws.read_words(mailbox_at, d_ctl, mailbox_words, st);
            return e;
        }
        if (first) {
            staged = !PHANT_ARENA_POISONS && (size_t)(span_end - ws.io.base) <= Workspaces::STAGE_BYTES;
            if (staged) e = ws.ensure_stage();
        }
        auto in_stage = [&](const Item& it) { return staged && it.src >= span && it.src + it.bytes <= span_end; };
        bool copied = false;
        for (int k = done; k < n && e == hipSuccess; ++k)
            if (!in_stage(item[k])) e = hipMemcpyAsync(item[k].dst, item[k].src, item[k].bytes, hipMemcpyDeviceToHost, st), copied = true;
        if (e != hipSuccess) return e;
        if (first && staged) e = hipMemcpyAsync(ws.staged(const_cast<uint8_t*>(span)), span, (size_t)(span_end - span), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
        if (first && !staged && mailbox_words) e = ws.read_words(mailbox_at, d_ctl, mailbox_words, st);
        else if (first || copied) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        for (; done < n; ++done)
            if (in_stage(item[done])) memcpy(item[done].dst, ws.staged(item[done].src), item[done].bytes);
        return hipSuccess;
    }
};

}  // namespace phant
