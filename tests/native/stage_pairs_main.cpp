// stage_pairs_main.cpp -- phant_amd/csrc/staging.h's stage_pairs alone, over the emulated runtime (tests/native/shim) and with no kernel
// at all, so at sizes the emulated hasher cannot afford: a forest's sorted pairs in host memory go in, and every staged byte and every
// rebased offset is read back from the "device" side.  tests/test_stage_pairs_native.py builds it twice: with AddressSanitizer the arena
// poisons the padding behind every sub-allocation, so nothing may be staged and no copy may touch padding (ASan stops the program if
// one does); without it the pinned stage is used wherever the inputs end within it.  In both builds the copies of every call are
// counted -- one when staged, one per non-empty array otherwise -- and so are the calls of operator new: the staged path makes none.
// Every invalid input is given alone and in pairs (which refusal comes first), and leaves nothing laid out or copied.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "../../phant_amd/csrc/staging.h"

using namespace phant;

static unsigned long long g_news = 0;
void* operator new(size_t n) {
    ++g_news;
    if (void* p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void* p) noexcept { std::free(p); }
void operator delete(void* p, size_t) noexcept { std::free(p); }

static int g_cases = 0, g_staged = 0;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s:%d: %s (case %d)\n", __FILE__, __LINE__, #cond, g_cases); \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

constexpr size_t STAGE = Workspaces::STAGE_BYTES;
static size_t R(size_t b) { return DevArena::round(b); }
static uint8_t pattern(size_t k, size_t i) { return (uint8_t)(i * 7 + k * 31 + (i >> 8) + 1); }

struct Shape {
    std::vector<uint32_t> key_len;
    std::vector<uint64_t> val_len;
    std::vector<uint32_t> seg;      // empty: seg_first is null (one trie)
    uint32_t key_base = 0;          // the caller's offset tables begin here, not at 0
    uint64_t val_base = 0;
    bool null_offsets = false;      // n == 0 and no offset tables at all
    size_t more_in = 0, more_out = 0;  // the caller's carve: an input array behind the five, an output behind that
    bool more_in_null = false;      // ... whose source the caller does not have
};

struct Counters {
    unsigned long long h2d, d2h, d2d, memsets, syncs;
};
static Counters now() { return {hipemu::M.h2d, hipemu::M.d2h, hipemu::M.d2d, hipemu::M.memsets, hipemu::M.stream_syncs}; }

// the caller's arrays of a shape, as a C caller would hold them
struct Caller {
    std::vector<uint8_t> keys, vals, more;
    std::vector<uint32_t> key_off;
    std::vector<uint64_t> val_off;
    HostPairs h;
    explicit Caller(const Shape& s) {
        const uint32_t n = (uint32_t)s.key_len.size();
        key_off.assign(1, s.key_base);
        val_off.assign(1, s.val_base);
        for (uint32_t i = 0; i < n; ++i) key_off.push_back(key_off.back() + s.key_len[i]), val_off.push_back(val_off.back() + s.val_len[i]);
        keys.resize(key_off.back());
        vals.resize(val_off.back());
        for (size_t i = 0; i < keys.size(); ++i) keys[i] = pattern(1, i);
        for (size_t i = 0; i < vals.size(); ++i) vals[i] = pattern(2, i);
        more.resize(s.more_in);
        for (size_t i = 0; i < more.size(); ++i) more[i] = pattern(3, i);
        h = HostPairs{keys.data(), s.null_offsets ? nullptr : key_off.data(), vals.data(), s.null_offsets ? nullptr : val_off.data(), n,
                      s.seg.empty() ? nullptr : s.seg.data(), s.seg.empty() ? 1u : (uint32_t)s.seg.size() - 1u};
    }
};

// one good call: -> whether it was staged
static bool run(Workspaces& ws, hipStream_t st, const Shape& s) {
    ++g_cases;
    const Caller c(s);
    const uint32_t n = c.h.n, n_tries = c.h.n_tries;
    const size_t kb = c.keys.size() - s.key_base, vb = c.vals.size() - s.val_base;
    // where the inputs end, by the layout's own rules
    const size_t five = R(kb + 16) + R(((size_t)n + 1) * 4) + R(vb + 16) + R(((size_t)n + 1) * 8) + ((size_t)n_tries + 1) * 4;
    const size_t in_end = s.more_in ? R(five) + s.more_in : five;
    const bool want_staged = !PHANT_ARENA_POISONS && in_end <= STAGE;
    uint8_t *d_more = nullptr, *d_out = nullptr;
    std::string err;
    const size_t cap_before = ws.io.cap;
    const Counters t0 = now();
    const unsigned long long news0 = g_news;
    const StagedPairs r = stage_pairs(ws, st, c.h, "test", err, [] { return PHANT_OK; }, [&](auto& io) -> const void* {
        if (s.more_in) d_more = io.template take<uint8_t>(s.more_in);
        if (s.more_out) d_out = io.template take<uint8_t>(s.more_out);
        return d_more ? d_more + s.more_in : nullptr;  // (the sizer hands out no addresses)
    }, [&](StagedInputs& ins) { ins.put(d_more, s.more_in_null ? nullptr : c.more.data(), s.more_in); });
    const unsigned long long news = g_news - news0;
    const Counters t1 = now();
    CHECK(r.rc == PHANT_OK && err.empty() && !ws.io.overflowed && ws.io.used <= ws.io.cap);
    CHECK(r.staged == want_staged);
    if (r.staged) CHECK(news == 0);  // (the offsets were rebased in place in the mirror)
    if (PHANT_ARENA_POISONS) CHECK(ws.stage == nullptr);
    const size_t arrays = (kb ? 1 : 0) + (vb ? 1 : 0) + 3 + (s.more_in && !s.more_in_null ? 1 : 0);
    CHECK(t1.h2d - t0.h2d == (r.staged ? 1u : arrays));
    CHECK(t1.d2h == t0.d2h && t1.d2d == t0.d2d && t1.memsets == t0.memsets);
    CHECK(t1.syncs - t0.syncs == (ws.io.cap > cap_before ? 1u : 0u));  // synchronised exactly when the arena grew
    // the device view, and every byte behind it
    const TriePairs& p = r.pairs;
    CHECK(p.n == n && p.n_tries == n_tries && p.key_bytes == kb && p.val_bytes == vb && p.roots == nullptr);
    CHECK(p.keys == ws.io.base && (size_t)(reinterpret_cast<const uint8_t*>(p.seg_first + n_tries + 1) - ws.io.base) == five);
    for (size_t i = 0; i < kb; ++i) CHECK(p.keys[i] == c.keys[s.key_base + i]);
    for (size_t i = 0; i < vb; ++i) CHECK(p.vals[i] == c.vals[s.val_base + i]);
    for (uint32_t i = 0; i <= n; ++i) CHECK(p.key_off[i] == c.key_off[i] - s.key_base && p.val_off[i] == c.val_off[i] - s.val_base);
    for (uint32_t t = 0; t <= n_tries; ++t) CHECK(p.seg_first[t] == (s.seg.empty() ? (t ? n : 0u) : s.seg[t]));
    if (s.more_in) CHECK((size_t)(d_more + s.more_in - ws.io.base) == in_end);
    for (size_t i = 0; i < s.more_in && !s.more_in_null; ++i) CHECK(d_more[i] == c.more[i]);
    if (s.more_out) CHECK(d_out >= ws.io.base + in_end && d_out + s.more_out <= ws.io.base + ws.io.used);
    g_staged += r.staged;
    return r.staged;
}

// one refused call: its code and text, and nothing laid out or copied
static void refuse(Workspaces& ws, hipStream_t st, const HostPairs& h, int32_t more_rc, int32_t want_rc, const char* want_text) {
    ++g_cases;
    const Counters t0 = now();
    const size_t used = ws.io.used, cap = ws.io.cap;
    std::string err;
    bool carved = false, put = false;
    const StagedPairs r = stage_pairs(ws, st, h, "test", err, [&] { return more_rc ? (err = "the caller's own refusal", more_rc) : PHANT_OK; },
                                      [&](auto&) -> const void* { return carved = true, nullptr; }, [&](StagedInputs&) { put = true; });
    const Counters t1 = now();
    CHECK(r.rc == want_rc && err == want_text && !r.staged && !carved && !put);
    CHECK(t1.h2d == t0.h2d && t1.d2h == t0.d2h && t1.d2d == t0.d2d && t1.memsets == t0.memsets && t1.syncs == t0.syncs);
    CHECK(ws.io.used == used && ws.io.cap == cap);
}

int main() {
    Workspaces ws;
    hipStream_t st = nullptr;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);

    // ---- small shapes: one trie without a segment table, several tries with empty ones at the first, a middle and the last position,
    // keys of 0 and 255 bytes, values of 0 bytes, offset tables that begin elsewhere, the caller's arrays behind the five
    Shape one;
    one.key_len = {32, 32, 1, 0, 255, 7};
    one.val_len = {5, 0, 300, 1, 70000, 33};
    for (int twice = 0; twice < 2; ++twice) CHECK(run(ws, st, one) == !PHANT_ARENA_POISONS);  // (the second call: an arena that fits)
    Shape forest = one;
    forest.seg = {0, 0, 2, 2, 2, 5, 6, 6};
    run(ws, st, forest);
    forest.key_base = 1000, forest.val_base = 3000000;
    run(ws, st, forest);
    one.key_base = 100000, one.val_base = 5000001;
    run(ws, st, one);
    for (bool null_src : {false, true}) {
        Shape more = forest;
        more.more_in = 777, more.more_out = 5000, more.more_in_null = null_src;
        run(ws, st, more);
        more.more_in = 0;
        run(ws, st, more);
    }
    Shape none;  // no pairs: offset tables of one entry, or none at all; one trie or several (all empty)
    run(ws, st, none);
    none.null_offsets = true;
    run(ws, st, none);
    none.seg = {0, 0, 0, 0};
    run(ws, st, none);
    none.more_in = 40, none.more_out = 8;
    CHECK(run(ws, st, none) == !PHANT_ARENA_POISONS);

    // ---- the stage's edge: 63 tries' segment table is one 256-byte line, so the inputs of one 32-byte key with a value of
    // STAGE - 1024 - 16 bytes end exactly at STAGE_BYTES; one more byte of the caller's behind them ends one byte beyond it
    const size_t cap_small = ws.io.cap;
    Shape edge;
    edge.key_len = {32};
    edge.val_len = {STAGE - 1024 - 16};
    edge.seg.assign(64, 1u);
    edge.seg[0] = 0;
    CHECK(run(ws, st, edge) == !PHANT_ARENA_POISONS);
    CHECK(ws.io.cap > cap_small);  // (the arena grew)
    edge.val_len = {STAGE - 1024 - 16 + 1};  // (the value's padding grows by a line)
    CHECK(!run(ws, st, edge));
    edge.val_len = {STAGE - 1280 - 16};
    edge.more_in = 1;  // ends at STAGE - 256 + 1: staged ...
    CHECK(run(ws, st, edge) == !PHANT_ARENA_POISONS);
    edge.val_len = {STAGE - 1024 - 16};  // ... and at STAGE + 1: not
    CHECK(!run(ws, st, edge));
    edge.more_in = 0, edge.more_out = 100000;  // outputs may lie beyond the stage: the inputs alone decide
    CHECK(run(ws, st, edge) == !PHANT_ARENA_POISONS);

    // ---- well beyond: nine values of 1 MiB, offsets that begin elsewhere, three tries
    Shape big;
    big.key_len.assign(9, 32);
    big.val_len.assign(9, 1u << 20);
    big.seg = {0, 3, 3, 9};
    big.key_base = 64, big.val_base = 4096;
    big.more_in = 100, big.more_out = 64;
    CHECK(!run(ws, st, big));
    CHECK(run(ws, st, one) == !PHANT_ARENA_POISONS);  // a small call on the grown arena is staged again

    // ---- refusals, alone and in pairs: the checks run in the order offsets (per pair: monotone, then the key's length), segment table
    // monotone, segment table's span, the caller's own
    {
        const uint8_t bytes[2048] = {};
        const uint32_t seg_ok[3] = {0, 1, 3}, seg_back[3] = {0, 2, 1}, seg_beyond[3] = {0, 4, 3}, seg_first[3] = {1, 1, 3}, seg_short[3] = {0, 1, 2}, seg_back_first[3] = {1, 0, 3};
        const uint32_t ko_ok[4] = {10, 20, 30, 40}, ko_back[4] = {10, 20, 15, 40}, ko_long[4] = {10, 266, 300, 310}, ko_long_then_back[4] = {10, 266, 300, 290};
        const uint64_t vo_ok[4] = {5, 5, 9, 100}, vo_back[4] = {5, 9, 8, 100}, vo_back_first[4] = {5, 4, 8, 100};
        auto pairs = [&](const uint32_t* ko, const uint64_t* vo, const uint32_t* seg) { return HostPairs{bytes, ko, bytes, vo, 3, seg, 2}; };
        const char *MONO = "offsets not monotone", *LONG = "key longer than 255 bytes", *SEG = "seg_first not monotone", *SPAN = "seg_first must span [0, n]";
        refuse(ws, st, pairs(ko_back, vo_ok, seg_ok), 0, PHANT_E_INVALID_ARG, MONO);
        refuse(ws, st, pairs(ko_ok, vo_back, seg_ok), 0, PHANT_E_INVALID_ARG, MONO);
        refuse(ws, st, pairs(ko_long, vo_ok, seg_ok), 0, PHANT_E_UNSUPPORTED, LONG);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_back), 0, PHANT_E_INVALID_ARG, SEG);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_beyond), 0, PHANT_E_INVALID_ARG, SEG);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_first), 0, PHANT_E_INVALID_ARG, SPAN);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_short), 0, PHANT_E_INVALID_ARG, SPAN);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_ok), PHANT_E_INVALID_ARG, PHANT_E_INVALID_ARG, "the caller's own refusal");
        HostPairs h1 = pairs(ko_ok, vo_ok, nullptr);  // a null segment table stands for one trie only
        h1.n_tries = 1;
        refuse(ws, st, h1, PHANT_E_UNSUPPORTED, PHANT_E_UNSUPPORTED, "the caller's own refusal");
        // in pairs
        refuse(ws, st, pairs(ko_long, vo_back_first, seg_ok), 0, PHANT_E_INVALID_ARG, MONO);       // the same pair: monotone first
        refuse(ws, st, pairs(ko_long_then_back, vo_ok, seg_ok), 0, PHANT_E_UNSUPPORTED, LONG);     // an earlier pair's length first
        refuse(ws, st, pairs(ko_long, vo_back, seg_ok), 0, PHANT_E_UNSUPPORTED, LONG);
        refuse(ws, st, pairs(ko_back, vo_ok, seg_back), 0, PHANT_E_INVALID_ARG, MONO);
        refuse(ws, st, pairs(ko_long, vo_ok, seg_first), 0, PHANT_E_UNSUPPORTED, LONG);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_back_first), 0, PHANT_E_INVALID_ARG, SEG);  // not monotone and not from 0
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_back), PHANT_E_UNSUPPORTED, PHANT_E_INVALID_ARG, SEG);
        refuse(ws, st, pairs(ko_ok, vo_ok, seg_short), PHANT_E_UNSUPPORTED, PHANT_E_INVALID_ARG, SPAN);
        refuse(ws, st, pairs(ko_back, vo_ok, seg_ok), PHANT_E_UNSUPPORTED, PHANT_E_INVALID_ARG, MONO);
    }
    CHECK(PHANT_ARENA_POISONS ? g_staged == 0 && ws.stage == nullptr : g_staged >= 15);
    ws.release();
    (void)hipStreamDestroy(st);
    std::printf("%d calls, %d staged, poisons %d\n", g_cases, g_staged, (int)PHANT_ARENA_POISONS);
    return 0;
}
