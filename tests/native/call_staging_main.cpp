// call_staging_main.cpp -- phant_amd/csrc/staging.h alone, over the emulated runtime (tests/native/shim): synthetic calls laid out the
// way the block-level drivers lay theirs out, a host "kernel" that copies every input to its output, and every delivered byte compared
// with what was put in.  tests/test_call_staging_native.py builds it twice: with AddressSanitizer the arena poisons the padding behind
// every sub-allocation, so the helper must never stage and no copy may touch padding (ASan stops the program if one does); without it
// the pinned stage is used wherever the span ends within it.  In both builds the copies, memsets and synchronisations of every call are
// counted and held against what the protocol promises for the call's form.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../phant_amd/csrc/staging.h"

using namespace phant;

static int g_cases = 0, g_staged_in = 0, g_staged_out = 0;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: %s (case %d)\n", __FILE__, __LINE__, #cond, g_cases); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

constexpr size_t CTL_WORDS = 8, MAILBOX_AT = Workspaces::MAILBOX_TXST, STAGE = Workspaces::STAGE_BYTES;
enum Form { HOST, DEVICE };

struct Array {
    size_t bytes;
    bool null_in = false;  // the caller passes no input (the output then keeps the arena's fill)
    bool wanted = true;    // the caller passes an output buffer
};

struct Call {
    std::vector<Array> arrays;
    bool inputs_first = false;  // the arena holds the inputs in front of the control words (header_chain) or behind the outputs
    size_t late_bytes = 0;      // an output behind the span whose size only the control words tell
    bool late_wanted = true;
};

static uint8_t pattern(size_t k, size_t i) { return (uint8_t)(i * 7 + k * 31 + (i >> 8) + 1); }

struct Counters {
    unsigned long long h2d, d2h, d2d, memsets, syncs;
};
static Counters now() { return {hipemu::M.h2d, hipemu::M.d2h, hipemu::M.d2d, hipemu::M.memsets, hipemu::M.stream_syncs}; }

// one call through lay_out_arena, StagedInputs, the "kernel", CallOutputs -> checks every byte and every count
static void run(Workspaces& ws, hipStream_t st, Form form, const Call& c) {
    ++g_cases;
    const size_t k_n = c.arrays.size();
    const bool dev = form == DEVICE;
    // the caller's side: inputs (pageable host arrays, or "device" arrays in the device form) and output buffers with guards
    std::vector<uint8_t*> in(k_n, nullptr), outb(k_n, nullptr);
    for (size_t k = 0; k < k_n; ++k) {
        const Array& a = c.arrays[k];
        if (!a.null_in && a.bytes) {
            CHECK(hipMalloc(&in[k], a.bytes) == hipSuccess);
            for (size_t i = 0; i < a.bytes; ++i) in[k][i] = pattern(k, i);
        }
        if (a.wanted) {
            CHECK(hipMalloc(&outb[k], a.bytes + 16) == hipSuccess);
            std::memset(outb[k], 0xEE, a.bytes + 16);
        }
    }
    uint8_t* late_buf = nullptr;
    if (c.late_wanted && c.late_bytes) {
        CHECK(hipMalloc(&late_buf, c.late_bytes + 16) == hipSuccess);
        std::memset(late_buf, 0xEE, c.late_bytes + 16);
    }

    // ---- layout
    uint32_t* d_ctl = nullptr;
    std::vector<uint8_t*> d_in(k_n, nullptr), d_out(k_n, nullptr);
    uint8_t *d_late = nullptr, *in_end = nullptr;
    auto carve_in = [&](auto& io) {
        for (size_t k = 0; k < k_n && !dev; ++k) d_in[k] = io.template take<uint8_t>(c.arrays[k].bytes);
        in_end = io.template take<uint8_t>(0);
    };
    auto carve = [&](auto& io) {
        if (c.inputs_first) carve_in(io);
        d_ctl = io.template take<uint32_t>(CTL_WORDS);
        for (size_t k = 0; k < k_n; ++k) d_out[k] = io.template take<uint8_t>(c.arrays[k].bytes);
        d_late = io.template take<uint8_t>(c.late_bytes);
        if (!c.inputs_first) carve_in(io);
    };
    const size_t cap_before = ws.io.cap;
    const Counters t0 = now();
    const LaidOut laid = lay_out_arena(ws.io, st, carve);
    CHECK(laid.what == LaidOut::OK && !ws.io.overflowed && ws.io.cap >= ws.io.used);
    CHECK(now().syncs - t0.syncs == (ws.io.cap > cap_before ? 1u : 0u));  // synchronised exactly when the arena grew
    CHECK(ws.ensure_mailbox() == hipSuccess);
    CHECK(hipMemsetAsync(d_ctl, 0, 4 * CTL_WORDS, st) == hipSuccess);

    // ---- in
    const Counters t1 = now();
    bool staged_in = false;
    size_t n_in = 0;
    for (size_t k = 0; k < k_n; ++k) n_in += in[k] != nullptr;
    if (!dev) {
        uint8_t* const begin = k_n ? d_in[0] : in_end;
        if (k_n) in_end = d_in[k_n - 1] + c.arrays[k_n - 1].bytes;  // (the exact end of the last array, not of its padding)
        StagedInputs ins(ws, st, begin, in_end);
        for (size_t k = 0; k < k_n; ++k) ins.put(d_in[k], in[k], c.arrays[k].bytes);
        CHECK(ins.finish() == hipSuccess);
        staged_in = ins.staged;
        CHECK(staged_in == (!PHANT_ARENA_POISONS && (size_t)(in_end - ws.io.base) <= STAGE));
        CHECK(now().h2d - t1.h2d == (staged_in ? (in_end > begin ? 1u : 0u) : n_in));
        g_staged_in += staged_in;
    }
    const Counters t2 = now();
    CHECK(t2.d2h == t1.d2h && t2.d2d == t1.d2d && t2.syncs == t1.syncs);  // (the caller's own arrays: no synchronisation)

    // ---- the "kernel": exact bytes only, like the device's (a read of padding would be ASan's to report)
    size_t total = 0;
    for (size_t k = 0; k < k_n; ++k) {
        const uint8_t* src = dev ? in[k] : d_in[k];
        if (in[k]) std::memcpy(d_out[k], src, c.arrays[k].bytes);
        total += in[k] ? c.arrays[k].bytes : 0;
    }
    for (size_t i = 0; i < c.late_bytes; ++i) d_late[i] = pattern(99, i);
    d_ctl[1] = (uint32_t)total, d_ctl[2] = (uint32_t)c.late_bytes;

    // ---- out
    CallOutputs outs(ws, st, dev, d_ctl, d_ctl, MAILBOX_AT, CTL_WORDS);
    size_t n_out = 0;
    for (size_t k = 0; k < k_n; ++k) {
        outs.add(outb[k], d_out[k], in[k] ? c.arrays[k].bytes : 0);
        n_out += outb[k] && in[k];
    }
    const uint8_t* const span_end = outs.span_end;
    CHECK(outs.deliver() == hipSuccess);
    const bool staged_out = outs.staged;
    CHECK(staged_out == (!dev && !PHANT_ARENA_POISONS && (size_t)(span_end - ws.io.base) <= STAGE));
    g_staged_out += staged_out;
    const Counters t3 = now();
    CHECK(t3.h2d == t2.h2d && t3.memsets == t2.memsets && t3.syncs - t2.syncs == 1);
    CHECK(t3.d2d - t2.d2d == (dev ? n_out : 0u));
    CHECK(t3.d2h - t2.d2h == (dev ? 1u : staged_out ? 1u : n_out + 1u));
    CHECK(outs.ctl()[1] == (uint32_t)total && outs.ctl()[2] == (uint32_t)c.late_bytes);
    // the late output: its size from the control words just read
    const size_t late = outs.ctl()[2];
    outs.add(late_buf, d_late, late);
    CHECK(outs.deliver() == hipSuccess);
    const Counters t4 = now();
    const bool late_copied = late_buf && late;
    CHECK(t4.d2d - t3.d2d == (dev && late_copied ? 1u : 0u) && t4.d2h - t3.d2h == (!dev && late_copied ? 1u : 0u));
    CHECK(t4.syncs - t3.syncs == (!dev && late_copied ? 1u : 0u));
    CHECK(outs.ctl()[1] == (uint32_t)total);  // (still there)
    if (PHANT_ARENA_POISONS) CHECK(ws.stage == nullptr);

    // ---- every delivered byte, and nothing behind it
    for (size_t k = 0; k < k_n; ++k) {
        if (!outb[k]) continue;
        const size_t b = c.arrays[k].bytes;
        for (size_t i = 0; i < b; ++i) CHECK(outb[k][i] == (in[k] ? pattern(k, i) : 0xEE));
        for (size_t i = b; i < b + 16; ++i) CHECK(outb[k][i] == 0xEE);
    }
    if (late_buf) {
        for (size_t i = 0; i < late; ++i) CHECK(late_buf[i] == pattern(99, i));
        for (size_t i = late; i < late + 16; ++i) CHECK(late_buf[i] == 0xEE);
    }
    for (size_t k = 0; k < k_n; ++k) (void)hipFree(in[k]), (void)hipFree(outb[k]);
    (void)hipFree(late_buf);
}

int main() {
    Workspaces ws;
    hipStream_t st = nullptr;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    const std::vector<size_t> sizes = {1, 3, 255, 256, 257, 1000, 4096, 70001};
    for (Form form : {HOST, DEVICE})
        for (bool inputs_first : {false, true}) {
            // every array present; then a zero-byte, a NULL and an unwanted array at the first, a middle and the last position
            Call all;
            all.inputs_first = inputs_first;
            for (size_t b : sizes) all.arrays.push_back({b});
            all.late_bytes = 777;
            run(ws, st, form, all);
            for (size_t at : {(size_t)0, sizes.size() / 2, sizes.size() - 1}) {
                Call c = all;
                c.arrays[at].bytes = 0;
                run(ws, st, form, c);
                c = all;
                c.arrays[at].null_in = true;
                run(ws, st, form, c);
                c = all;
                c.arrays[at].wanted = false;
                run(ws, st, form, c);
            }
            // no output wanted at all: the control words alone come back; nothing late either
            Call none = all;
            for (Array& a : none.arrays) a.wanted = false;
            none.late_wanted = false;
            run(ws, st, form, none);
            none.late_bytes = 0;
            run(ws, st, form, none);
            Call empty;
            empty.inputs_first = inputs_first;
            run(ws, st, form, empty);
        }
    const int staged_before_edges = g_staged_in + g_staged_out;
    // a span that ends exactly at STAGE_BYTES, and one byte beyond: the outputs' (control words first: 256 bytes), then the inputs'
    const size_t cap_small = ws.io.cap;
    for (size_t extra : {(size_t)0, (size_t)1}) {
        Call out_edge;
        out_edge.arrays = {{1000}, {STAGE - 256 - 1024 + extra}};  // (ctl 256, the first array 1024 with its padding)
        out_edge.late_bytes = 5;
        const int before = g_staged_out;
        run(ws, st, HOST, out_edge);
        CHECK(g_staged_out - before == (!PHANT_ARENA_POISONS && !extra ? 1 : 0));
        Call in_edge;
        in_edge.inputs_first = true;
        in_edge.arrays = {{1000}, {STAGE - 1024 + extra}};
        const int before_in = g_staged_in;
        run(ws, st, HOST, in_edge);
        CHECK(g_staged_in - before_in == (!PHANT_ARENA_POISONS && !extra ? 1 : 0));
        run(ws, st, DEVICE, out_edge);
    }
    CHECK(ws.io.cap > cap_small);  // the arena grew between two calls ...
    Call small;
    small.arrays = {{5}, {0}, {600}};
    small.late_bytes = 1;
    run(ws, st, HOST, small);  // ... and a small call on the grown arena is staged again
    CHECK(PHANT_ARENA_POISONS ? staged_before_edges == 0 && ws.stage == nullptr : staged_before_edges > 40);
    ws.release();
    (void)hipStreamDestroy(st);
    std::printf("%d calls, %d staged in, %d staged out, poisons %d\n", g_cases, g_staged_in, g_staged_out, (int)PHANT_ARENA_POISONS);
    return 0;
}
