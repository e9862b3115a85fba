// staging.h -- how a block-level call crosses the bus, once, for the drivers that keep their arrays in the ctx's
// `io` arena: block_receipts, header_chain, block_transactions, block_txs_prestate.  Plain host C++ on top of arena.h.
//
//   lay_out_arena an arena sized by, then carved by, one list of take<T>() calls
//   StagedInputs  the host form's arrays on their way in: ONE copy through the pinned stage, or a copy each
//   CallOutputs   every output named once; deliver() hands them back as the call's form asks
//
// The pinned stage mirrors the first STAGE_BYTES of `io`.  It is used when the bytes in question END within it and the arena does not
// poison its padding (a copy of a span crosses the padding between sub-allocations; a sanitizer build therefore copies array by array,
// exact bytes only), and only by calls that end in a stream synchronisation: the next call overwrites it.
#pragma once
#include <string.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

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
    hipError_t finish() {
        if (e == hipSuccess && staged && end > begin) e = hipMemcpyAsync(begin, ws.staged(begin), (size_t)(end - begin), hipMemcpyHostToDevice, st);
        return e;
    }
};

// ---- out: add() names an output once (a NULL caller pointer or no bytes: nobody wants it), deliver() hands back what was added since
// the last deliver():
//   device form        a device-to-device copy each, then the control words into the mailbox (one copy, one synchronisation)
//   host form, staged  ONE copy of [span, the end of the last output inside `io`) into the pinned stage, a synchronisation, memcpys
//   host form, plain   a copy each, then the control words into the mailbox (without control words: the synchronisation alone)
// An output outside the fetched span -- in another arena, or added after the first deliver() and behind the span, like encodings whose
// size only the control words tell -- gets a copy of its own in every form; a later deliver() synchronises the host form when it made one.
// A call without control words leaves mailbox_words at 0; ctl() is valid after the first deliver().
struct CallOutputs {
    static constexpr int CAP = 40;  // block_transactions names 35
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
