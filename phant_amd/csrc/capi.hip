// capi.hip -- the C-ABI of include/phant_gpu.h: context, device workspace,
// host-form (staging) and device-form (resident) entry points.
//
// No CPU fallback lives here: every entry point ends in a HIP kernel launch;
// without a gfx950 device phant_ctx_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "../../include/phant_gpu.h"
#include "../../include/phant_gpu_diag.h"
#include "arena.h"
#include "staging.h"
#include "launch.h"
#include "receipts.h"
#include "requests_check.h"
#include "filters_check.h"
#include "feehist_check.h"
#include "headers.h"
#include "transactions.h"
#include "settle.h"
#include "txstate.h"
#include "access_lists.h"
#include "trie_build.h"
#include "witness.h"
#include "host_rlp.h"

struct phant_witness {
    phant::Witness w;
};
struct phant_exec_witness {
    phant::ExecWitness w;
};

// The workspace of the node-set pipeline (mpt_verify_nodeset.hip): zeroed when it is allocated, never cleared afterwards -- every
// launch on it carries an epoch greater than all before it.
struct NodesetSpace {
    phant::DevArena dv;
    uint32_t cap_nodes = 0;  // what `dv` is laid out for (grow-only, a power of two: the layout never changes under a live claim word)
    uint32_t epoch = 0;
    bool dirty = true;  // to be zeroed before the next launch (fresh memory, a failed launch, the epoch about to wrap)
};

struct phant_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // grow-only device arenas for the host-form calls
    phant::Workspaces ws;
    phant::DevArena dv;  // workspace of the device-form verify pipeline
    NodesetSpace ns;     // ... of the node-set pipeline
    uint32_t ns_salt[2] = {0, 0};  // key of its record table's slot function
    phant::NodesetTune ns_tune;
    bool last_was_nodeset = false;  // which pipeline phant_verify_stats reports on
    uint32_t ns_last[3] = {0, 0, 0};  // what the last node-set launch on `ns` chose (NodesetTune::last; phant_nodeset_stats)
    phant::VerifyTune tune;
    int32_t dedup_levels = -1;  // trie levels deduplicated by the two-tier pipeline: < 0 = from the batch size, 0 = none
    // helper stream of the two-tier pipeline: its deep tier runs there, next to the shallow tier (created on first use)
    phant::FlatSide side{nullptr, nullptr, nullptr};
    // streaming slots (phant_mpt_verify_submit / phant_wait): own stream, staging and workspace each
    struct Slot {
        hipStream_t stream = nullptr;
        phant::DevArena io, dv;
        NodesetSpace ns;
        bool busy = false;
    } slots[PHANT_MAX_SLOTS];
    uint32_t last_shallow = 0;  // trie levels the last two-tier launch deduplicated (diagnostics)
    uint32_t last_form = 0;     // the shallow tier's form in the last launch (VerifyTune::last_form)
    hipEvent_t kev[phant::VERIFY_KERNEL_STAGES + 1] = {};  // diagnostics (PHANT_DIAG_VERIFY_SERIAL): events around the stages of a launch
    bool kev_valid = false;
    // stream-side timing of the last device-form call
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_pending = false;
    // phant_exec_witness_prestate: the codes are hashed on a helper stream of their own, next to the node-set kernels (created on
    // first use); code_form: PHANT_DIAG_CODE_HASH_FORM
    phant::FlatSide code_side{nullptr, nullptr, nullptr};
    uint32_t code_form = 0;
    bool post_raw_slot_keys = false;  // PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS
    uint64_t advance_estimate = 0;    // PHANT_DIAG_ADVANCE_ESTIMATE_BYTES (0: the call's own estimate)
    bool ranges_no_leaf_pass = false;     // PHANT_DIAG_RANGES_NO_LEAF_PASS
    int64_t ranges_items_per_range = -1;  // PHANT_DIAG_RANGES_ITEMS_PER_RANGE (-1: the call's own estimate)
    uint32_t logfilter_sets = 0;          // PHANT_DIAG_LOGFILTER_SETS
    int64_t feehist_block_max = 0;        // PHANT_DIAG_FEEHIST_BLOCK_MAX (0: PHANT_FEEHIST_BLOCK_MAX)
    uint32_t* secp_gtable = nullptr;  // phant_ecrecover_batch: 1 G .. 255 G, computed on the device by the first call that needs it
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            changed = hipSetDevice(dev) == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

int32_t fail(phant_ctx* c, int32_t code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        c->err = what;
        if (e != hipSuccess) {
            c->err += ": ";
            c->err += hipGetErrorString(e);
        }
    }
    return code;
}

#define HIP_TRY(c, call)                                               \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return fail((c), PHANT_E_DEVICE, #call, e_); \
    } while (0)

// Lay out a call's staging arrays in `io` (staging.h: phant::lay_out_arena; afterwards io.used is the counted total), a failure as this
// file reports one.
template <class Lay>
int32_t lay_out(phant_ctx* c, hipStream_t s, phant::DevArena& io, const Lay& lay) {
    const phant::LaidOut r = phant::lay_out_arena(io, s, lay);
    if (r.what == phant::LaidOut::SYNC_FAILED) return fail(c, PHANT_E_DEVICE, "hipStreamSynchronize(s)", r.e);
    if (r.what == phant::LaidOut::OOM) return fail(c, PHANT_E_OOM, "hipMalloc(workspace)", r.e);
    return r.what == phant::LaidOut::UNDERSIZED ? fail(c, PHANT_E_DEVICE, "staging arena undersized") : PHANT_OK;
}

struct TimedRegion {
    phant_ctx* c;  // null: not timed
    explicit TimedRegion(phant_ctx* ctx, bool timed = true) : c(timed && ctx->timing ? ctx : nullptr) {
        if (c) (void)hipEventRecord(c->ev0, c->stream);
    }
    ~TimedRegion() {
        if (c) {
            (void)hipEventRecord(c->ev1, c->stream);
            c->ev_pending = true;
        }
    }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

// The functions of include/phant_gpu.h are implemented in namespace phant_impl; the exported `extern "C"` symbols are generated
// wrappers (capi_guard_capi.inc, tools/gen_capi_guard.py) that call them inside a try block: host memory running out in a
// std::vector / std::string comes back as PHANT_E_OOM, nothing unwinds or aborts across the C boundary.
namespace phant_impl {
int32_t guard_failed(phant_ctx* c, int32_t code) noexcept {
    if (c) {
        try {
            c->err = code == PHANT_E_OOM ? "out of host memory" : "unexpected exception";
        } catch (...) {
        }
    }
    return code;
}
}  // namespace phant_impl

namespace phant_impl {

const char* phant_version(void) { return "phant_gpu 0.1 (gfx950)"; }

int32_t phant_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void phant_ctx_destroy(phant_ctx* c);
int32_t phant_ctx_create(const phant_opts* opts, phant_ctx** out) {
    if (!out) return PHANT_E_INVALID_ARG;
    *out = nullptr;
    int dev = 0;
    void* stream = nullptr;
    bool own = false;
    if (opts) {
        if (opts->struct_size < sizeof(phant_opts)) return PHANT_E_INVALID_ARG;
        dev = opts->device;
        stream = opts->stream;
        own = (opts->flags & PHANT_CTX_OWN_STREAM) != 0;
    }
    int32_t dedup_levels = -1;
    if (opts && (opts->flags & PHANT_CTX_DEDUP_LEVELS_MASK))
        dedup_levels = (int32_t)((opts->flags & PHANT_CTX_DEDUP_LEVELS_MASK) >> PHANT_CTX_DEDUP_LEVELS_SHIFT) - 1;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || dev < 0 || dev >= n) return PHANT_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return PHANT_E_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PHANT_E_NO_DEVICE;
    phant_ctx* c = new (std::nothrow) phant_ctx();
    if (!c) return PHANT_E_OOM;
    struct Holder {  // (destroyed on every way out but the last: also when something below runs out of host memory)
        phant_ctx* c;
        ~Holder() {
            if (c) phant_impl::phant_ctx_destroy(c);
        }
    } holder{c};
    c->device = dev;
    {
        std::random_device rd;
        c->ns_salt[0] = (uint32_t)rd();
        c->ns_salt[1] = (uint32_t)rd();
    }
    c->dedup_levels = dedup_levels;
    DeviceGuard g(dev);
    if (!own) {
        c->stream = (hipStream_t)stream;  // nullptr = the default stream
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            c->stream = nullptr;
            return PHANT_E_DEVICE;
        }
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) return PHANT_E_DEVICE;
    c->tune.last_shallow = &c->last_shallow;
    c->tune.last_form = &c->last_form;
    holder.c = nullptr;
    *out = c;
    return PHANT_OK;
}

void phant_ctx_destroy(phant_ctx* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->ws.release();
    c->dv.release();
    c->ns.dv.release();
    if (c->secp_gtable) (void)hipFree(c->secp_gtable);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->kev)
        if (e) (void)hipEventDestroy(e);
    for (auto& sl : c->slots) {
        if (sl.stream) {
            (void)hipStreamSynchronize(sl.stream);
            (void)hipStreamDestroy(sl.stream);
        }
        sl.io.release();
        sl.dv.release();
        sl.ns.dv.release();
    }
    if (c->side.stream) (void)hipStreamSynchronize(c->side.stream);
    if (c->side.stream2) (void)hipStreamSynchronize(c->side.stream2);
    if (c->side.fork) (void)hipEventDestroy(c->side.fork);
    if (c->side.join) (void)hipEventDestroy(c->side.join);
    if (c->side.join2) (void)hipEventDestroy(c->side.join2);
    if (c->code_side.stream) (void)hipStreamSynchronize(c->code_side.stream);
    if (c->code_side.fork) (void)hipEventDestroy(c->code_side.fork);
    if (c->code_side.join) (void)hipEventDestroy(c->code_side.join);
    if (c->code_side.stream) (void)hipStreamDestroy(c->code_side.stream);
    if (c->side.stream) (void)hipStreamDestroy(c->side.stream);
    if (c->side.stream2) (void)hipStreamDestroy(c->side.stream2);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* phant_last_error(const phant_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int32_t phant_set_stream(phant_ctx* c, void* stream) {
    if (!c) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->own_stream) {
        (void)hipStreamDestroy(c->stream);
        c->own_stream = false;
    }
    c->stream = (hipStream_t)stream;  // nullptr = the default stream
    return PHANT_OK;
}

int32_t phant_stream_sync(phant_ctx* c) {
    if (!c) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

int32_t phant_timing(phant_ctx* c, int32_t enable) {
    if (!c) return PHANT_E_INVALID_ARG;
    c->timing = enable != 0;
    c->ev_pending = false;
    return PHANT_OK;
}

int32_t phant_verify_stats(phant_ctx* c, uint32_t hashed[8]) {
    if (!c || !hashed) return PHANT_E_INVALID_ARG;
    for (int i = 0; i < 8; ++i) hashed[i] = 0;
    if (c->last_was_nodeset) {
        if (!c->ns.dv.base) return PHANT_OK;
        DeviceGuard g(c->device);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        uint32_t hdr[phant::VERIFY_HEADER_WORDS];
        HIP_TRY(c, hipMemcpy(hdr, c->ns.dv.base, sizeof(hdr), hipMemcpyDeviceToHost));
        phant::verify_nodeset_stats_from_header(hdr, c->ns.epoch, hashed, nullptr);
        return PHANT_OK;
    }
    if (!c->dv.base) return PHANT_OK;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->side.stream) HIP_TRY(c, hipStreamSynchronize(c->side.stream));
    // list counts and the deep tier's striped counters, in the header of the verify workspace (mpt_verify_v3.hip)
    uint32_t hdr[phant::VERIFY_HEADER_WORDS];
    HIP_TRY(c, hipMemcpy(hdr, c->dv.base, sizeof(hdr), hipMemcpyDeviceToHost));
    phant::verify_stats_from_header(hdr, hashed);
    return PHANT_OK;
}

int32_t phant_nodeset_stats(phant_ctx* c, uint32_t out[PHANT_NODESET_STATS]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    for (int i = 0; i < PHANT_NODESET_STATS; ++i) out[i] = 0;
    // (a workspace about to be zeroed -- fresh, or a launch on it failed -- holds no launch to describe)
    if (!c->ns.dv.base || c->ns.dirty || c->ns.epoch == 0u || c->ns_last[0] == 0u) return PHANT_OK;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t hdr[phant::VERIFY_HEADER_WORDS];
    HIP_TRY(c, hipMemcpy(hdr, c->ns.dv.base, sizeof(hdr), hipMemcpyDeviceToHost));
    uint32_t hashed[8], overflow = 0;
    phant::verify_nodeset_stats_from_header(hdr, c->ns.epoch, hashed, &overflow);
    phant::verify_nodeset_lists_from_header(hdr, c->ns.epoch, out + 1);
    out[0] = c->ns_last[0];
    out[10] = overflow;
    out[11] = c->ns_last[1];
    out[12] = c->ns_last[2];
    out[13] = c->ns.epoch;
    return PHANT_OK;
}

int32_t phant_verify_tier_stats(phant_ctx* c, uint32_t out[5]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!c->dv.base) return PHANT_OK;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->side.stream) HIP_TRY(c, hipStreamSynchronize(c->side.stream));
    uint32_t hdr[phant::VERIFY_HEADER_WORDS];
    HIP_TRY(c, hipMemcpy(hdr, c->dv.base, sizeof(hdr), hipMemcpyDeviceToHost));
    out[0] = c->last_shallow;
    phant::verify_tier_stats_from_header(hdr, out + 1);
    return PHANT_OK;
}

int32_t phant_verify_form(phant_ctx* c, uint32_t* form) {
    if (!c || !form) return PHANT_E_INVALID_ARG;
    *form = c->last_form;
    return PHANT_OK;
}

int32_t phant_verify_path_stats(phant_ctx* c, uint32_t out[2]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    out[0] = out[1] = 0;
    if (!c->dv.base) return PHANT_OK;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->side.stream) HIP_TRY(c, hipStreamSynchronize(c->side.stream));
    uint32_t hdr[phant::VERIFY_HEADER_WORDS];
    HIP_TRY(c, hipMemcpy(hdr, c->dv.base, sizeof(hdr), hipMemcpyDeviceToHost));
    phant::verify_paths_from_header(hdr, out);
    return PHANT_OK;
}

int32_t phant_trie_stats(phant_ctx* c, uint32_t out[PHANT_TRIE_STATS]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    const phant::TrieStats& s = c->ws.trie_stats;
    for (int i = 0; i < PHANT_TRIE_STATS; ++i) out[i] = 0;
    out[0] = s.pass;
    out[1] = s.ahead;
    out[2] = (uint32_t)s.deep_from;
    out[3] = s.bins;
    out[4] = s.max_bin;
    for (int k = 0; k < 5; ++k) out[5 + k] = s.by_class[k];
    out[11] = s.leaf_big;
    out[12] = s.n_rep;
    out[13] = s.n;
    out[14] = s.side_bins;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->ws.side) HIP_TRY(c, hipStreamSynchronize(c->ws.side));
    // the per-depth misfit counters, where the last general pass left them (an offset, not a pointer: whatever has happened to
    // the arena since, the copy stays inside it)
    constexpr size_t MISFIT_BYTES = 512 * sizeof(uint32_t);
    if (s.has_misfit && c->ws.t1.base && s.misfit_off + MISFIT_BYTES <= c->ws.t1.cap) {
        std::vector<uint32_t> mis(512);
        HIP_TRY(c, hipMemcpy(mis.data(), c->ws.t1.base + s.misfit_off, MISFIT_BYTES, hipMemcpyDeviceToHost));
        uint64_t tot = 0;
        for (const uint32_t m : mis) tot += m;
        out[10] = (uint32_t)std::min<uint64_t>(tot, 0xffffffffull);
    }
    if (s.has_cursor && c->ws.t1.base && s.cursor_off + sizeof(unsigned long long) <= c->ws.t1.cap) {
        unsigned long long used = 0;
        HIP_TRY(c, hipMemcpy(&used, c->ws.t1.base + s.cursor_off, sizeof used, hipMemcpyDeviceToHost));
        out[15] = (uint32_t)std::min<unsigned long long>(used, 0xffffffffull);
    }
    return PHANT_OK;
}

int32_t phant_verify_kernel_ms(phant_ctx* c, float ms[PHANT_VERIFY_KERNEL_STAGES]) {
    if (!c || !ms) return PHANT_E_INVALID_ARG;
    if (!c->tune.kernel_ev) return fail(c, PHANT_E_UNSUPPORTED, "verify_kernel_ms: the tiers are not serialised on this ctx (phant_diag_set: the verify-serial knob)");
    // (the events hold the LAST launch that recorded them: if the latest verify took the S = 0 form they are an earlier one's)
    if (!c->kev_valid) return fail(c, PHANT_E_INVALID_ARG, "verify_kernel_ms: the last verify launch on this ctx was not a two-tier one");
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    static_assert(PHANT_VERIFY_KERNEL_STAGES == phant::VERIFY_KERNEL_STAGES, "one stage list");
    for (int i = 0; i < PHANT_VERIFY_KERNEL_STAGES; ++i) {
        ms[i] = 0.f;
        if (hipEventElapsedTime(&ms[i], c->kev[i], c->kev[i + 1]) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, PHANT_E_INVALID_ARG, "verify_kernel_ms: no two-tier launch on this ctx yet");
        }
    }
    return PHANT_OK;
}

int32_t phant_last_kernel_ms(phant_ctx* c, float* ms) {
    if (!c || !ms) return PHANT_E_INVALID_ARG;
    if (!c->ev_pending) return fail(c, PHANT_E_INVALID_ARG, "no timed call pending");
    DeviceGuard g(c->device);
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return PHANT_OK;
}

int32_t phant_diag_set(phant_ctx* c, uint32_t knob, int64_t value) {
    if (!c) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    phant::TrieTune& t = c->ws.tune;
    switch (knob) {
        case PHANT_DIAG_VERIFY_SERIAL:
            if (value && !c->tune.kernel_ev) {  // events around every stage of a two-tier launch (phant_verify_kernel_ms)
                for (hipEvent_t& e : c->kev)
                    if (!e) HIP_TRY(c, hipEventCreate(&e));
                c->tune.kernel_ev = c->kev;
            }
            c->tune.serial = value != 0;
            c->kev_valid = false;
            return PHANT_OK;
        case PHANT_DIAG_VERIFY_HASH_LDS_KB:
            // (on top of the hash kernels' 8 KiB of static LDS, and the list kernel is launched with 8 KiB more: the sum must stay
            // within the 64 KiB a launch gets without opting in)
            c->tune.hash_lds = (uint32_t)(value < 0 ? 0 : value > 47 ? 47 : value) * 1024u;
            return PHANT_OK;
        case PHANT_DIAG_VERIFY_NO_COOP: c->tune.no_coop = value != 0; return PHANT_OK;
        case PHANT_DIAG_VERIFY_NO_WAVE: c->tune.no_wave = value != 0; return PHANT_OK;
        case PHANT_DIAG_VERIFY_COOP_MAX: c->tune.coop_max = (uint32_t)(value < 0 ? 0 : value > (1 << 20) ? (1 << 20) : value); return PHANT_OK;
        case PHANT_DIAG_STREAM_WGS: c->tune.diag_stream_wgs = (uint32_t)(value < 0 ? 0 : value > 65536 ? 65536 : value); return PHANT_OK;
        case PHANT_DIAG_STREAM_MB: c->tune.diag_stream_mb = (uint32_t)(value < 0 ? 0 : value > 65536 ? 65536 : value); return PHANT_OK;
        case PHANT_DIAG_TRIE_NO_SIDE: t.no_side = value != 0; return PHANT_OK;
        case PHANT_DIAG_TRIE_SIDE_MIN_KEYS: t.side_min_keys = value; return PHANT_OK;
        case PHANT_DIAG_TRIE_AHEAD_MAX_KEYS: t.ahead_max_keys = value; return PHANT_OK;
        case PHANT_DIAG_TRIE_SIDE_LDS: t.side_lds = value; return PHANT_OK;
        case PHANT_DIAG_TRIE_FALLBACK_GRID: t.fallback_grid = value; return PHANT_OK;
        case PHANT_DIAG_TRIE_SLOT_BLOCKS: t.slot_blocks = (int32_t)value; return PHANT_OK;
        case PHANT_DIAG_TRIE_NO_COOP: t.no_coop = value != 0; return PHANT_OK;
        case PHANT_DIAG_TRIE_COOP_MAX: t.coop_max = value; return PHANT_OK;
        case PHANT_DIAG_TRIE_NO_WAVE: t.no_wave = value != 0; return PHANT_OK;
        case PHANT_DIAG_TRIE_JOIN_IN_STREAM: t.join_in_stream = value != 0; return PHANT_OK;
        case PHANT_DIAG_SORT_NO_FALLBACK: t.sort_no_fallback = value != 0; return PHANT_OK;
        case PHANT_DIAG_SORT_PREFIX_BITS: t.sort_prefix_bits = value; return PHANT_OK;
        case PHANT_DIAG_SORT_REPAIR_BITS: t.sort_repair_bits = value; return PHANT_OK;
        case PHANT_DIAG_NODESET_WAVE_MAX: c->ns_tune.wave_max = (uint32_t)(value < 0 ? 0 : value > (1 << 20) ? (1 << 20) : value); return PHANT_OK;
        case PHANT_DIAG_TRIE_SMALL_MAX_KEYS: t.small_max_keys = value; return PHANT_OK;
        case PHANT_DIAG_CODE_HASH_FORM: c->code_form = value == 1 ? 1u : 0u; return PHANT_OK;
        case PHANT_DIAG_POSTSTATE_RAW_SLOT_KEYS: c->post_raw_slot_keys = value != 0; return PHANT_OK;
        case PHANT_DIAG_ADVANCE_ESTIMATE_BYTES: c->advance_estimate = value > 0 ? (uint64_t)value : 0u; return PHANT_OK;
        case PHANT_DIAG_VERIFY_LIST_WGS: c->tune.list_wgs_cap = (uint32_t)(value < 0 ? 0 : value > (1 << 20) ? (1 << 20) : value); return PHANT_OK;
        case PHANT_DIAG_RANGES_NO_LEAF_PASS: c->ranges_no_leaf_pass = value != 0; return PHANT_OK;
        case PHANT_DIAG_RANGES_ITEMS_PER_RANGE: c->ranges_items_per_range = value < 0 ? -1 : value > 1922 ? 1922 : value; return PHANT_OK;
        case PHANT_DIAG_LOGFILTER_SETS: c->logfilter_sets = value == 1 ? 1u : value == 2 ? 2u : 0u; return PHANT_OK;
        case PHANT_DIAG_FEEHIST_BLOCK_MAX: c->feehist_block_max = value; return PHANT_OK;
        default: return fail(c, PHANT_E_INVALID_ARG, "diag_set: no such knob");
    }
}

int32_t phant_nodeset_tune(phant_ctx* c, int32_t ladder, uint32_t order, uint32_t hash_lds_bytes, uint32_t resident_wgs) {
    if (!c || ladder < 0 || ladder > 2 || order > 1u || hash_lds_bytes > 56u * 1024u) return PHANT_E_INVALID_ARG;
    c->ns_tune.form = (uint32_t)ladder;
    c->ns_tune.order = order;
    c->ns_tune.hash_lds = hash_lds_bytes;
    c->ns_tune.resident_wgs = resident_wgs;
    return PHANT_OK;
}

int32_t phant_keccak_rate(phant_ctx* c, uint32_t waves_per_simd, uint32_t perms, double* perms_per_s) {
    if (!c || !perms_per_s || waves_per_simd == 0 || waves_per_simd > 8 || perms == 0) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    int cus = 0;
    HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const uint32_t blocks = (uint32_t)cus * waves_per_simd;  // a 256-lane workgroup = one wave on each of a CU's four SIMDs
    uint32_t* d_out = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) { d_out = io.template take<uint32_t>((size_t)blocks * 256); });
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(c, hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = phant::launch_keccak_rate(d_out, blocks, perms, c->stream);  // (warm-up: code in the instruction caches)
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    if (e == hipSuccess) e = phant::launch_keccak_rate(d_out, blocks, perms, c->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(c, PHANT_E_DEVICE, "keccak_rate", e);
    *perms_per_s = ms > 0.f ? (double)blocks * 256.0 * perms / (ms * 1e-3) : 0.0;
    return PHANT_OK;
}

/* ------------------------------------------------------------------ Keccak */

// the batch forms of both hash functions: message i = blob[off[i] .. off[i+1]), a launcher of keccak_batch.hip
using BatchLauncher = hipError_t (*)(const uint8_t*, const uint64_t*, uint32_t, uint8_t*, hipStream_t);

static int32_t hash_batch_dev(phant_ctx* c, const char* who, BatchLauncher launch, const uint8_t* d_blob, const uint64_t* d_off, uint32_t n, uint8_t* d_out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!d_off || !d_out || !aligned16(d_out)) return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + "_dev: null or unaligned pointer").c_str());
    DeviceGuard g(c->device);
    TimedRegion t(c);
    HIP_TRY(c, launch(d_blob, d_off, n, d_out, c->stream));
    return PHANT_OK;
}

int32_t phant_keccak256_batch_dev(phant_ctx* c, const uint8_t* d_blob, const uint64_t* d_off,
                                  uint32_t n, uint8_t* d_out) {
    return hash_batch_dev(c, "keccak256_batch", phant::launch_keccak256_var, d_blob, d_off, n, d_out);
}

int32_t phant_sha256_batch_dev(phant_ctx* c, const uint8_t* d_blob, const uint64_t* d_off, uint32_t n, uint8_t* d_out) {
    return hash_batch_dev(c, "sha256_batch", phant::launch_sha256_var, d_blob, d_off, n, d_out);
}

int32_t phant_keccak256_fixed_dev(phant_ctx* c, const uint8_t* d_blob, uint32_t msg_len,
                                  uint64_t stride, uint32_t n, uint8_t* d_out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!d_out || !aligned16(d_out) || (!d_blob && msg_len) || (stride < msg_len && n > 1))
        return fail(c, PHANT_E_INVALID_ARG, "keccak256_fixed_dev: bad argument");
    DeviceGuard g(c->device);
    TimedRegion t(c);
    HIP_TRY(c, phant::launch_keccak256_fixed(d_blob, msg_len, stride, n, d_out, c->stream));
    return PHANT_OK;
}

static int32_t hash_batch(phant_ctx* c, const char* who, BatchLauncher launch, const uint8_t* blob, const uint64_t* off, uint32_t n, uint8_t* out) {
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!off || !out) return bad("null pointer");
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return bad("offsets not monotone");
    const uint64_t lo = off[0], hi = off[n];
    const size_t blob_len = (size_t)(hi - lo);
    if (blob_len && !blob) return bad("null blob");
    DeviceGuard g(c->device);
    uint8_t *d_blob = nullptr, *d_out = nullptr;
    uint64_t* d_off = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_blob = io.template take<uint8_t>(blob_len + 16);
        d_off = io.template take<uint64_t>((size_t)n + 1);
        d_out = io.template take<uint8_t>((size_t)n * 32);
    });
    if (rc) return rc;
    std::vector<uint64_t> rel((size_t)n + 1);
    for (uint32_t i = 0; i <= n; ++i) rel[i] = off[i] - lo;
    if (blob_len) HIP_TRY(c, hipMemcpyAsync(d_blob, blob + lo, blob_len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch(d_blob, d_off, n, d_out, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

int32_t phant_keccak256_batch(phant_ctx* c, const uint8_t* blob, const uint64_t* off, uint32_t n,
                              uint8_t* out) {
    return hash_batch(c, "keccak256_batch", phant::launch_keccak256_var, blob, off, n, out);
}

int32_t phant_sha256_batch(phant_ctx* c, const uint8_t* blob, const uint64_t* off, uint32_t n, uint8_t* out) {
    return hash_batch(c, "sha256_batch", phant::launch_sha256_var, blob, off, n, out);
}

int32_t phant_keccak256(phant_ctx* c, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    const uint64_t off[2] = {0, len};
    return phant_impl::phant_keccak256_batch(c, data, off, 1, out);
}

int32_t phant_keccak256_with_prefix(phant_ctx* c, const uint8_t* prefix, uint64_t prefix_len,
                                    const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (!c) return PHANT_E_INVALID_ARG;
    if ((prefix_len && !prefix) || (len && !data)) return fail(c, PHANT_E_INVALID_ARG, "keccak256_with_prefix: null pointer");
    // hasher.zig:10-17 streams prefix then data through one sponge: same as
    // hashing the concatenation
    uint8_t* cat = (uint8_t*)std::malloc((size_t)(prefix_len + len) + 1);
    if (!cat) return fail(c, PHANT_E_OOM, "keccak256_with_prefix: host staging");
    if (prefix_len) std::memcpy(cat, prefix, (size_t)prefix_len);
    if (len) std::memcpy(cat + prefix_len, data, (size_t)len);
    const uint64_t off[2] = {0, prefix_len + len};
    const int32_t rc = phant_impl::phant_keccak256_batch(c, cat, off, 1, out);
    std::free(cat);
    return rc;
}

/* ------------------------------------------------- other bulk Keccak users */

int32_t phant_logs_bloom_dev(phant_ctx* c, const uint8_t* d_items, const uint64_t* d_item_off,
                             const uint32_t* d_item_receipt, uint32_t n_items, uint32_t n_receipts, uint8_t* d_blooms) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n_receipts == 0) return PHANT_OK;
    if (!d_blooms || ((uintptr_t)d_blooms & 3u) || (n_items && (!d_item_off || !d_item_receipt)))
        return fail(c, PHANT_E_INVALID_ARG, "logs_bloom_dev: null or unaligned pointer");
    DeviceGuard g(c->device);
    TimedRegion t(c);
    HIP_TRY(c, phant::launch_logs_bloom(d_items, d_item_off, d_item_receipt, n_items, n_receipts, d_blooms, c->stream));
    return PHANT_OK;
}

int32_t phant_logs_bloom(phant_ctx* c, const uint8_t* items, const uint64_t* item_off, const uint32_t* item_receipt,
                         uint32_t n_items, uint32_t n_receipts, uint8_t* blooms) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n_receipts == 0) return PHANT_OK;
    if (!blooms || (n_items && (!item_off || !item_receipt))) return fail(c, PHANT_E_INVALID_ARG, "logs_bloom: null pointer");
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_off[i + 1] < item_off[i]) return fail(c, PHANT_E_INVALID_ARG, "logs_bloom: offsets not monotone");
    const uint64_t lo = n_items ? item_off[0] : 0, hi = n_items ? item_off[n_items] : 0;
    const size_t blob_len = (size_t)(hi - lo);
    if (blob_len && !items) return fail(c, PHANT_E_INVALID_ARG, "logs_bloom: null items");
    DeviceGuard g(c->device);
    uint8_t *d_items = nullptr, *d_blooms = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t* d_rcpt = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_items = io.template take<uint8_t>(blob_len + 16);
        d_off = io.template take<uint64_t>((size_t)n_items + 1);
        d_rcpt = io.template take<uint32_t>((size_t)n_items + 1);
        d_blooms = io.template take<uint8_t>((size_t)n_receipts * 256);
    });
    if (rc) return rc;
    std::vector<uint64_t> rel((size_t)n_items + 1, 0);
    for (uint32_t i = 0; i <= n_items && n_items; ++i) rel[i] = item_off[i] - lo;
    if (blob_len) HIP_TRY(c, hipMemcpyAsync(d_items, items + lo, blob_len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (n_items) HIP_TRY(c, hipMemcpyAsync(d_rcpt, item_receipt, (size_t)n_items * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, phant::launch_logs_bloom(d_items, d_off, d_rcpt, n_items, n_receipts, d_blooms, c->stream));
    HIP_TRY(c, hipMemcpyAsync(blooms, d_blooms, (size_t)n_receipts * 256, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

int32_t phant_sender_addresses_dev(phant_ctx* c, const uint8_t* d_pubkeys, uint64_t stride, uint32_t n, uint8_t* d_out20) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!d_pubkeys || !d_out20 || ((uintptr_t)d_out20 & 3u) || stride < 64)
        return fail(c, PHANT_E_INVALID_ARG, "sender_addresses_dev: bad argument");
    DeviceGuard g(c->device);
    TimedRegion t(c);
    HIP_TRY(c, phant::launch_sender_addresses(d_pubkeys, stride, n, d_out20, c->stream));
    return PHANT_OK;
}

int32_t phant_sender_addresses(phant_ctx* c, const uint8_t* pubkeys, uint64_t stride, uint32_t n, uint8_t* out20) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!pubkeys || !out20 || stride < 64) return fail(c, PHANT_E_INVALID_ARG, "sender_addresses: bad argument");
    DeviceGuard g(c->device);
    uint8_t *d_pk = nullptr, *d_out = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_pk = io.template take<uint8_t>((size_t)n * 64 + 16);
        d_out = io.template take<uint8_t>((size_t)n * 20);
    });
    if (rc) return rc;
    if (stride == 64) {
        HIP_TRY(c, hipMemcpyAsync(d_pk, pubkeys, (size_t)n * 64, hipMemcpyHostToDevice, c->stream));
    } else {  // pack: only the 64 key bytes travel
        std::vector<uint8_t> packed((size_t)n * 64);
        for (uint32_t i = 0; i < n; ++i) std::memcpy(packed.data() + 64 * (size_t)i, pubkeys + stride * i, 64);
        HIP_TRY(c, hipMemcpyAsync(d_pk, packed.data(), packed.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // `packed` dies with this scope
    }
    HIP_TRY(c, phant::launch_sender_addresses(d_pk, 64, n, d_out, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out20, d_out, (size_t)n * 20, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

/* ------------------------------------------------- a block's receipts (receipts.hip.h) */

static int32_t block_receipts_impl(phant_ctx* c, const phant_receipts_in* in, phant_receipts_out* out, bool dev) {
    const char* const who = dev ? "block_receipts_dev" : "block_receipts";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_receipts_in) || out->struct_size != sizeof(phant_receipts_out)) return bad("wrong struct_size");
    out->encoded_len = 0;
    const uint32_t n = in->n_receipts, nl = in->n_logs;
    if (n && (!in->tx_type || !in->status || !in->cum_gas || !in->log_first)) return bad("null receipt array");
    if (nl && (!n || !in->address || !in->topic_first || !in->data_off)) return bad("null log array, or logs without receipts");
    if ((in->n_topics && (!nl || !in->topics)) || (in->data_bytes && (!nl || !in->data))) return bad("null topics / data, or topics / data without logs");
    if (in->receipts_at > in->n_lists) return bad("receipts_at > n_lists");
    if (in->n_lists && (!in->lists || !in->list_off || !in->list_n || (dev && !in->list_bytes))) return bad("null list table");
    for (uint32_t l = 0; l < in->n_lists; ++l)
        if (in->list_n[l] && (!in->list_off[l] || (!in->lists[l] && (!dev || in->list_bytes[l])))) return bad("null list");
    if (dev) {
        // (what a kernel reads or writes as words; roots, rows and the block's bloom arrive by device-to-device copies of bytes)
        bool mis = ((uintptr_t)in->cum_gas & 7u) || ((uintptr_t)in->data_off & 7u) || ((uintptr_t)out->encoded_off & 7u) || ((uintptr_t)in->log_first & 3u) ||
                   ((uintptr_t)in->topic_first & 3u);
        for (uint32_t l = 0; l < in->n_lists; ++l) mis = mis || ((uintptr_t)in->list_off[l] & 7u);
        if (mis) return bad("misaligned array");
    }
    phant::ReceiptsArgs a;
    a.tx_type = in->tx_type, a.status = in->status, a.cum_gas = in->cum_gas, a.log_first = in->log_first, a.address = in->address;
    a.topic_first = in->topic_first, a.data_off = in->data_off, a.topics = in->topics, a.data = in->data;
    a.n = n, a.n_logs = nl, a.n_topics = in->n_topics, a.data_bytes = in->data_bytes;
    a.lists = in->lists, a.list_off = in->list_off, a.list_n = in->list_n, a.list_bytes = in->list_bytes, a.n_lists = in->n_lists;
    a.receipts_at = in->receipts_at;
    a.receipts_root = out->receipts_root, a.logs_bloom = out->logs_bloom, a.blooms = out->blooms, a.encoded = out->encoded;
    a.encoded_off = out->encoded_off, a.roots_out = out->roots_out, a.encoded_cap = out->encoded_cap, a.encoded_off_cap = out->encoded_off_cap;
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    const int32_t rc = phant::block_receipts(c->ws, c->stream, a, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    out->encoded_len = a.encoded_len;
    return PHANT_OK;
}

int32_t phant_block_receipts(phant_ctx* c, const phant_receipts_in* in, phant_receipts_out* out) {
    return block_receipts_impl(c, in, out, false);
}

int32_t phant_block_receipts_dev(phant_ctx* c, const phant_receipts_in* in, phant_receipts_out* out) {
    return block_receipts_impl(c, in, out, true);
}


/* ------------------------------------------------- block headers (headers.hip.h) */

static int32_t header_chain_impl(phant_ctx* c, const phant_headers_in* in, phant_headers_out* out, bool dev) {
    const char* const who = dev ? "header_chain_dev" : "header_chain";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_headers_in) || out->struct_size != sizeof(phant_headers_out)) return bad("wrong struct_size");
    const uint32_t n = in->n;
    if (n == 0) {
        out->first_bad = 0, out->enc_len = 0;
        return PHANT_OK;
    }
    if (!in->parent_hash || !in->uncle_hash || !in->fee_recipient || !in->state_root || !in->transactions_root || !in->receipts_root ||
        !in->logs_bloom || !in->difficulty || !in->number || !in->gas_limit || !in->gas_used || !in->timestamp || !in->extra_off ||
        !in->prev_randao || !in->nonce || !in->n_fields)
        return bad("a NULL array that every header needs");
    if (in->seg_first && (in->n_segs == 0 || in->n_segs > n)) return bad("n_segs is 0 or beyond n");
    if (dev) {  // (what a kernel reads or writes as words; digests, flags and encodings arrive by device-to-device copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->difficulty | (uintptr_t)in->number | (uintptr_t)in->gas_limit | (uintptr_t)in->gas_used |
                             (uintptr_t)in->timestamp | (uintptr_t)in->blob_gas_used | (uintptr_t)in->excess_blob_gas | (uintptr_t)out->enc_off;
        const uintptr_t w4 = (uintptr_t)in->extra_off | (uintptr_t)in->seg_first | (uintptr_t)out->flags;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    phant_headers_out res = *out;
    const int32_t rc = phant::header_chain(c->ws, c->stream, *in, res, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    out->first_bad = res.first_bad, out->enc_len = res.enc_len;
    return PHANT_OK;
}

int32_t phant_header_chain(phant_ctx* c, const phant_headers_in* in, phant_headers_out* out) { return header_chain_impl(c, in, out, false); }

int32_t phant_header_chain_dev(phant_ctx* c, const phant_headers_in* in, phant_headers_out* out) { return header_chain_impl(c, in, out, true); }

int32_t phant_headers_decode_rlp(const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t flags, phant_headers_in* fields_out,
                                 uint8_t* status) {
    if (flags & ~PHANT_HEADERS_FROM_BLOCKS) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    const phant_headers_in* f = fields_out;
    if (!off || !f || !status || f->struct_size != sizeof(phant_headers_in)) return PHANT_E_INVALID_ARG;
    if (!f->parent_hash || !f->uncle_hash || !f->fee_recipient || !f->state_root || !f->transactions_root || !f->receipts_root || !f->logs_bloom ||
        !f->difficulty || !f->number || !f->gas_limit || !f->gas_used || !f->timestamp || !f->extra_data || !f->extra_off || !f->prev_randao ||
        !f->nonce || !f->base_fee || !f->withdrawals_root || !f->blob_gas_used || !f->excess_blob_gas || !f->parent_beacon_root ||
        !f->requests_hash || !f->n_fields)
        return PHANT_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return PHANT_E_INVALID_ARG;
    if (off[n] != off[0] && !blob) return PHANT_E_INVALID_ARG;
    auto w8 = [](const uint8_t* p) { return const_cast<uint8_t*>(p); };
    auto w64 = [](const uint64_t* p) { return const_cast<uint64_t*>(p); };
    const phant::HeaderArrays a{w8(f->parent_hash), w8(f->uncle_hash), w8(f->fee_recipient), w8(f->state_root), w8(f->transactions_root),
                                w8(f->receipts_root), w8(f->logs_bloom), w64(f->difficulty), w64(f->number), w64(f->gas_limit), w64(f->gas_used),
                                w64(f->timestamp), w8(f->extra_data), const_cast<uint32_t*>(f->extra_off), w8(f->prev_randao), w8(f->nonce),
                                w8(f->base_fee), w8(f->withdrawals_root), w64(f->blob_gas_used), w64(f->excess_blob_gas),
                                w8(f->parent_beacon_root), w8(f->requests_hash), w8(f->n_fields)};
    uint32_t extra_at = 0;
    a.extra_off[0] = 0;
    for (uint32_t i = 0; i < n; ++i)
        status[i] = phant::header_decode(blob ? blob + off[i] : nullptr, (size_t)(off[i + 1] - off[i]), (flags & PHANT_HEADERS_FROM_BLOCKS) != 0, a, i, &extra_at) ? 0 : 1;
    fields_out->n = n;
    return PHANT_OK;
}

/* --------------------------------------------------------- sender recovery */

// the context's table of multiples of G: allocated and computed (on the ctx stream, in front of the launch that reads it)
// by the first call that needs it
static int32_t ensure_gtable(phant_ctx* c) {
    if (c->secp_gtable) return PHANT_OK;
    uint32_t* t = nullptr;
    hipError_t e = hipMalloc((void**)&t, (size_t)phant::SECP_GTABLE_BYTES);
    if (e != hipSuccess) return fail(c, PHANT_E_OOM, "hipMalloc(secp256k1 table)", e);
    e = phant::launch_secp_gtable(t, c->stream);
    if (e != hipSuccess) {
        (void)hipFree(t);
        return fail(c, PHANT_E_DEVICE, "launch_secp_gtable", e);
    }
    c->secp_gtable = t;
    return PHANT_OK;
}

int32_t phant_ecrecover_batch_dev(phant_ctx* c, const uint8_t* d_hashes, const uint8_t* d_r, const uint8_t* d_s,
                                  const uint8_t* d_recid, uint32_t n, uint32_t flags, uint8_t* d_pubkeys64,
                                  uint8_t* d_addresses20, uint8_t* d_status) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (flags & ~PHANT_RECOVER_LOW_S) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch_dev: unknown flag");
    if (!d_pubkeys64 && !d_addresses20 && !d_status) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch_dev: no output");
    if (n == 0) return PHANT_OK;
    if (!d_hashes || !d_r || !d_s || !d_recid) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch_dev: null input");
    DeviceGuard g(c->device);
    if (const int32_t rc = ensure_gtable(c)) return rc;
    TimedRegion t(c);
    HIP_TRY(c, phant::launch_ecrecover(d_hashes, d_r, d_s, d_recid, nullptr, n, flags, c->secp_gtable, d_pubkeys64, d_addresses20,
                                       d_status, c->stream));
    return PHANT_OK;
}

int32_t phant_ecrecover_batch(phant_ctx* c, const uint8_t* hashes, const uint8_t* r, const uint8_t* s, const uint8_t* recid,
                              uint32_t n, uint32_t flags, uint8_t* pubkeys64, uint8_t* addresses20, uint8_t* status) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (flags & ~PHANT_RECOVER_LOW_S) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch: unknown flag");
    if (!pubkeys64 && !addresses20 && !status) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch: no output");
    if (n == 0) return PHANT_OK;
    if (!hashes || !r || !s || !recid) return fail(c, PHANT_E_INVALID_ARG, "ecrecover_batch: null input");
    DeviceGuard g(c->device);
    if (const int32_t rc = ensure_gtable(c)) return rc;
    uint8_t *d_h = nullptr, *d_r = nullptr, *d_s = nullptr, *d_id = nullptr, *d_pk = nullptr, *d_ad = nullptr, *d_st = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_h = io.template take<uint8_t>((size_t)n * 32);
        d_r = io.template take<uint8_t>((size_t)n * 32);
        d_s = io.template take<uint8_t>((size_t)n * 32);
        d_id = io.template take<uint8_t>(n);
        if (pubkeys64) d_pk = io.template take<uint8_t>((size_t)n * 64);
        if (addresses20) d_ad = io.template take<uint8_t>((size_t)n * 20);
        if (status) d_st = io.template take<uint8_t>(n);
    });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_h, hashes, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_r, r, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_s, s, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_id, recid, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, phant::launch_ecrecover(d_h, d_r, d_s, d_id, nullptr, n, flags, c->secp_gtable, d_pk, d_ad, d_st, c->stream));
    if (pubkeys64) HIP_TRY(c, hipMemcpyAsync(pubkeys64, d_pk, (size_t)n * 64, hipMemcpyDeviceToHost, c->stream));
    if (addresses20) HIP_TRY(c, hipMemcpyAsync(addresses20, d_ad, (size_t)n * 20, hipMemcpyDeviceToHost, c->stream));
    if (status) HIP_TRY(c, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

int32_t phant_tx_senders(phant_ctx* c, const uint8_t* txs, const uint64_t* tx_off, uint32_t n, uint64_t chain_id,
                         uint8_t* addresses20, uint8_t* status) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (!addresses20 && !status) return fail(c, PHANT_E_INVALID_ARG, "tx_senders: no output");
    if (n == 0) return PHANT_OK;
    if (!tx_off) return fail(c, PHANT_E_INVALID_ARG, "tx_senders: null offsets");
    for (uint32_t i = 0; i < n; ++i)
        if (tx_off[i + 1] < tx_off[i]) return fail(c, PHANT_E_INVALID_ARG, "tx_senders: offsets not monotone");
    if (tx_off[n] != tx_off[0] && !txs) return fail(c, PHANT_E_INVALID_ARG, "tx_senders: null transactions");
    // host: decode, split off the signature, splice the preimages (one blob, hashed by the variable-length Keccak launch)
    std::vector<uint8_t> pre, rs((size_t)n * 64), ids((size_t)n * 2);  // rs: all r, then all s; ids: all recid, then the host's verdicts
    std::vector<uint64_t> off((size_t)n + 1);
    uint8_t *r = rs.data(), *s = rs.data() + (size_t)n * 32, *recid = ids.data(), *pre_st = ids.data() + n;
    for (uint32_t i = 0; i < n; ++i) {
        off[i] = pre.size();
        recid[i] = 0;
        pre_st[i] = phant::tx_signing_parts(txs + tx_off[i], (size_t)(tx_off[i + 1] - tx_off[i]), chain_id, pre, r + 32 * (size_t)i,
                                            s + 32 * (size_t)i, recid + i);
    }
    off[n] = pre.size();
    DeviceGuard g(c->device);
    if (const int32_t rc = ensure_gtable(c)) return rc;
    uint8_t *d_pre = nullptr, *d_h = nullptr, *d_rs = nullptr, *d_ids = nullptr, *d_ad = nullptr, *d_st = nullptr;
    uint64_t* d_off = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_pre = io.template take<uint8_t>(pre.size() + 16);
        d_off = io.template take<uint64_t>((size_t)n + 1);
        d_h = io.template take<uint8_t>((size_t)n * 32);
        d_rs = io.template take<uint8_t>((size_t)n * 64);
        d_ids = io.template take<uint8_t>((size_t)n * 2);
        if (addresses20) d_ad = io.template take<uint8_t>((size_t)n * 20);
        if (status) d_st = io.template take<uint8_t>(n);
    });
    if (rc) return rc;
    if (!pre.empty()) HIP_TRY(c, hipMemcpyAsync(d_pre, pre.data(), pre.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_rs, rs.data(), rs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_ids, ids.data(), ids.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, phant::launch_keccak256_var(d_pre, d_off, n, d_h, c->stream));
    const uint32_t low_s = PHANT_RECOVER_LOW_S;  // validateSignatureFields
    HIP_TRY(c, phant::launch_ecrecover(d_h, d_rs, d_rs + (size_t)n * 32, d_ids, d_ids + n, n, low_s, c->secp_gtable,
                                       nullptr, d_ad, d_st, c->stream));
    if (addresses20) HIP_TRY(c, hipMemcpyAsync(addresses20, d_ad, (size_t)n * 20, hipMemcpyDeviceToHost, c->stream));
    if (status) HIP_TRY(c, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the host vectors above live until here)
    return PHANT_OK;
}

/* ------------------------------------------------- a block's transactions (transactions.hip.h) */

// xin / xout: the new structs of phant_block_transactions_ex; null for phant_block_transactions, which is the same path with
// PHANT_TXS_FORK_LONDON and none of the new outputs
static int32_t block_transactions_impl(phant_ctx* c, const phant_txs_in* in, phant_txs_out* out, const phant_txs_ex_in* xin, phant_txs_ex_out* xout,
                                       bool dev) {
    const char* const who = xin ? (dev ? "block_transactions_ex_dev" : "block_transactions_ex") : dev ? "block_transactions_dev" : "block_transactions";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (xin && (xin->struct_size != sizeof(phant_txs_ex_in) || xout->struct_size != sizeof(phant_txs_ex_out))) return bad("wrong struct_size");
    if (in->struct_size != sizeof(phant_txs_in) || out->struct_size != sizeof(phant_txs_out)) return bad("wrong struct_size");
    if (xin && xin->fork > PHANT_TXS_FORK_PRAGUE) return bad("unknown fork");
    if (xin && xin->reserved != 0u) return bad("reserved is not 0");
    if (xin && (in->flags & PHANT_TXS_NO_RECOVERY) && (xout->authority || xout->auth_status))
        return bad("authority / auth_status asked for together with the no-recovery flag");
    if (in->flags & ~(PHANT_TXS_HAVE_GAS_LIMIT | PHANT_TXS_NO_RECOVERY)) return bad("unknown flag");
    if ((in->flags & PHANT_TXS_NO_RECOVERY) && (out->sender || out->sig_status)) return bad("sender / sig_status asked for together with the no-recovery flag");
    const uint32_t n = in->n;
    if (dev) {  // (tx_off is read by kernels as words; the outputs arrive by device-to-device copies of bytes)
        uintptr_t w8 = (uintptr_t)in->tx_off | (uintptr_t)out->chain_id | (uintptr_t)out->nonce | (uintptr_t)out->gas_limit |
                       (uintptr_t)out->data_off | (uintptr_t)out->al_off | (uintptr_t)out->intrinsic_gas;
        uintptr_t w4 = (uintptr_t)out->data_len | (uintptr_t)out->al_len | (uintptr_t)out->al_addresses | (uintptr_t)out->al_keys |
                       (uintptr_t)out->flags;
        if (xout) {
            w8 |= (uintptr_t)xout->blob_off | (uintptr_t)xout->floor_gas | (uintptr_t)xout->auth_nonce;
            w4 |= (uintptr_t)xout->blobs | (uintptr_t)xout->auth_first;
        }
        if (n != 0 && ((w8 & 7u) || (w4 & 3u))) return bad("misaligned array");
    }
    if (n == 0) {
        out->first_bad = 0;
        if (xout) {
            xout->n_auth = 0, xout->blob_gas_used = 0;
            if (xout->auth_first) {  // its one entry
                const uint32_t zero = 0;
                if (dev) {
                    DeviceGuard g(c->device);
                    HIP_TRY(c, hipMemcpyAsync(xout->auth_first, &zero, 4, hipMemcpyHostToDevice, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                } else {
                    xout->auth_first[0] = zero;
                }
            }
        }
        return PHANT_OK;
    }
    if (!in->tx_off || !in->txs) return bad("null txs / tx_off");
    DeviceGuard g(c->device);
    if (!(in->flags & PHANT_TXS_NO_RECOVERY))
        if (const int32_t rc = ensure_gtable(c)) return rc;
    TimedRegion t(c, dev);
    std::string err;
    phant_txs_ex_in call;
    phant_txs_ex_out res;
    std::memset(&call, 0, sizeof call);
    std::memset(&res, 0, sizeof res);
    if (xin) call = *xin, res = *xout;
    else call.fork = PHANT_TXS_FORK_LONDON, call.base = *in, res.base = *out;
    const int32_t rc = phant::block_transactions(c->ws, c->stream, call, res, dev, c->secp_gtable, err);
    if (rc) return fail(c, rc, err.c_str());
    out->first_bad = res.base.first_bad;
    if (xout) xout->n_auth = res.n_auth, xout->blob_gas_used = res.blob_gas_used;
    return PHANT_OK;
}

int32_t phant_block_transactions(phant_ctx* c, const phant_txs_in* in, phant_txs_out* out) { return block_transactions_impl(c, in, out, nullptr, nullptr, false); }

int32_t phant_block_transactions_dev(phant_ctx* c, const phant_txs_in* in, phant_txs_out* out) { return block_transactions_impl(c, in, out, nullptr, nullptr, true); }

int32_t phant_block_transactions_ex(phant_ctx* c, const phant_txs_ex_in* in, phant_txs_ex_out* out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return fail(c, PHANT_E_INVALID_ARG, "block_transactions_ex: in / out is null");
    return block_transactions_impl(c, &in->base, &out->base, in, out, false);
}

int32_t phant_block_transactions_ex_dev(phant_ctx* c, const phant_txs_ex_in* in, phant_txs_ex_out* out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return fail(c, PHANT_E_INVALID_ARG, "block_transactions_ex_dev: in / out is null");
    return block_transactions_impl(c, &in->base, &out->base, in, out, true);
}

/* ------------------------------------------------- chain segments of block bodies (bodies.hip.h) */

int32_t phant_bodies_decode_rlp(const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t flags, phant_bodies_split* sp, uint8_t* status) {
    if (flags & ~PHANT_BODIES_NO_HEADER) return PHANT_E_INVALID_ARG;
    if (!sp || sp->struct_size != sizeof(phant_bodies_split) || sp->reserved != 0u) return PHANT_E_INVALID_ARG;
    if (n && (!off || !status)) return PHANT_E_INVALID_ARG;
    for (uint32_t b = 0; b < n; ++b)
        if (off[b + 1] < off[b]) return PHANT_E_INVALID_ARG;
    if (n && off[n] != off[0] && !blob) return PHANT_E_INVALID_ARG;
    const bool has_header = !(flags & PHANT_BODIES_NO_HEADER);
    auto block = [&](uint32_t b, phant::BodyTotals& t, const phant::BodySink* sink) {
        return phant::body_split(blob ? blob + off[b] : nullptr, (size_t)(off[b + 1] - off[b]), has_header, t, sink);
    };
    phant::BodyTotals t{0, 0, 0, 0};
    for (uint32_t b = 0; b < n; ++b) (void)block(b, t, nullptr);
    if (t.n > 0xffffffffull || t.n_wd > 0xffffffffull) return PHANT_E_UNSUPPORTED;
    sp->n = (uint32_t)t.n, sp->n_wd = (uint32_t)t.n_wd, sp->tx_bytes = t.tx_bytes, sp->wd_bytes = t.wd_bytes;
    const bool room = sp->tx_off && sp->block_first && sp->wd_off && sp->wd_first && t.n <= sp->tx_cap && t.n_wd <= sp->wd_cap &&
                      (sp->txs ? t.tx_bytes <= sp->tx_bytes_cap : t.tx_bytes == 0) && (sp->withdrawals ? t.wd_bytes <= sp->wd_bytes_cap : t.wd_bytes == 0);
    if (!room) return PHANT_OK;
    const phant::BodySink sink{sp->txs, sp->tx_off, sp->withdrawals, sp->wd_off};
    t = phant::BodyTotals{0, 0, 0, 0};
    sp->tx_off[0] = 0, sp->wd_off[0] = 0, sp->block_first[0] = 0, sp->wd_first[0] = 0;
    for (uint32_t b = 0; b < n; ++b) {
        status[b] = block(b, t, &sink);
        sp->block_first[b + 1] = (uint32_t)t.n, sp->wd_first[b + 1] = (uint32_t)t.n_wd;
    }
    return PHANT_OK;
}

static int32_t block_bodies_impl(phant_ctx* c, const phant_bodies_in* in, phant_bodies_out* out, bool dev) {
    const char* const who = dev ? "block_bodies_dev" : "block_bodies";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_bodies_in) || out->struct_size != sizeof(phant_bodies_out) || out->txs.struct_size != sizeof(phant_txs_ex_out) ||
        out->txs.base.struct_size != sizeof(phant_txs_out))
        return bad("wrong struct_size");
    if (in->fork > PHANT_TXS_FORK_PRAGUE) return bad("unknown fork");
    if (in->reserved != 0u) return bad("reserved is not 0");
    if (in->flags & ~(PHANT_TXS_HAVE_GAS_LIMIT | PHANT_TXS_NO_RECOVERY)) return bad("unknown flag");
    const phant_txs_ex_out& x = out->txs;
    const phant_txs_out& o = x.base;
    if ((in->flags & PHANT_TXS_NO_RECOVERY) && (o.sender || o.sig_status || x.authority || x.auth_status))
        return bad("sender / sig_status / authority / auth_status asked for together with the no-recovery flag");
    if (!in->wd_first && (in->n_wd || in->withdrawals || in->wd_off || in->withdrawals_root || out->withdrawals_root))
        return bad("withdrawals, their count, offsets or roots without wd_first");
    const uint32_t n = in->n, nb = in->n_blocks;
    if (nb == 0) {  // (no block: nothing to index, nothing to write but the scalars)
        if (n || in->n_wd) return bad("transactions or withdrawals without a block");
        out->first_bad_block = 0;
        out->txs.base.first_bad = 0, out->txs.n_auth = 0, out->txs.blob_gas_used = 0;
        return PHANT_OK;
    }
    if (!in->block_first) return bad("null block_first");
    if (n && (!in->txs || !in->tx_off)) return bad("null txs / tx_off");
    if (in->n_wd && (!in->withdrawals || !in->wd_off)) return bad("null withdrawals / wd_off");
    if ((in->flags & PHANT_TXS_HAVE_GAS_LIMIT) && !in->gas_limit) return bad("null gas_limit with the gas-limit flag");
    if (dev) {  // (the offsets and the 64- and 32-bit per-block arrays are read by kernels as words; the outputs arrive by copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->tx_off | (uintptr_t)in->wd_off | (uintptr_t)in->gas_limit | (uintptr_t)in->blob_gas_used | (uintptr_t)o.chain_id |
                             (uintptr_t)o.nonce | (uintptr_t)o.gas_limit | (uintptr_t)o.data_off | (uintptr_t)o.al_off | (uintptr_t)o.intrinsic_gas |
                             (uintptr_t)x.blob_off | (uintptr_t)x.floor_gas | (uintptr_t)x.auth_nonce | (uintptr_t)out->block_blob_gas_used;
        const uintptr_t w4 = (uintptr_t)in->block_first | (uintptr_t)in->wd_first | (uintptr_t)o.data_len | (uintptr_t)o.al_len | (uintptr_t)o.al_addresses |
                             (uintptr_t)o.al_keys | (uintptr_t)o.flags | (uintptr_t)x.blobs | (uintptr_t)x.auth_first | (uintptr_t)out->tx_block |
                             (uintptr_t)out->block_first_bad | (uintptr_t)out->block_flags;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    DeviceGuard g(c->device);
    if (n && !(in->flags & PHANT_TXS_NO_RECOVERY))
        if (const int32_t rc = ensure_gtable(c)) return rc;
    TimedRegion t(c, dev);
    std::string err;
    phant_bodies_out res = *out;
    const int32_t rc = phant::block_bodies(c->ws, c->stream, *in, res, dev, c->secp_gtable, err);
    if (rc) return fail(c, rc, err.c_str());
    out->first_bad_block = res.first_bad_block;
    out->txs.base.first_bad = res.txs.base.first_bad, out->txs.n_auth = res.txs.n_auth, out->txs.blob_gas_used = res.txs.blob_gas_used;
    return PHANT_OK;
}

int32_t phant_block_bodies(phant_ctx* c, const phant_bodies_in* in, phant_bodies_out* out) { return block_bodies_impl(c, in, out, false); }

int32_t phant_block_bodies_dev(phant_ctx* c, const phant_bodies_in* in, phant_bodies_out* out) { return block_bodies_impl(c, in, out, true); }

/* ------------------------------------------------- receipts of a chain segment from raw messages (receipt_segments.hip.h) */

int32_t phant_receipts_decode_rlp(const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t flags, phant_receipts_split* sp, uint8_t* status) {
    if (flags & ~PHANT_RCPTS_SPLIT_ETH69) return PHANT_E_INVALID_ARG;
    if (!sp || sp->struct_size != sizeof(phant_receipts_split) || sp->reserved != 0u) return PHANT_E_INVALID_ARG;
    if (n && (!off || !status)) return PHANT_E_INVALID_ARG;
    for (uint32_t b = 0; b < n; ++b)
        if (off[b + 1] < off[b]) return PHANT_E_INVALID_ARG;
    if (n && off[n] != off[0] && !blob) return PHANT_E_INVALID_ARG;
    const bool eth69 = (flags & PHANT_RCPTS_SPLIT_ETH69) != 0u;
    auto block = [&](uint32_t b, phant::ReceiptTotals& t, const phant::ReceiptSink* sink) {
        return phant::receipts_split(blob ? blob + off[b] : nullptr, (size_t)(off[b + 1] - off[b]), eth69, t, sink);
    };
    phant::ReceiptTotals t{0, 0};
    for (uint32_t b = 0; b < n; ++b) (void)block(b, t, nullptr);
    if (t.n > 0xffffffffull) return PHANT_E_UNSUPPORTED;
    sp->n = (uint32_t)t.n, sp->rc_bytes = t.bytes;
    const bool room = sp->rc_off && sp->block_first && t.n <= sp->rc_cap && (sp->receipts ? t.bytes <= sp->rc_bytes_cap : t.bytes == 0);
    if (!room) return PHANT_OK;
    const phant::ReceiptSink sink{sp->receipts, sp->rc_off};
    t = phant::ReceiptTotals{0, 0};
    sp->rc_off[0] = 0, sp->block_first[0] = 0;
    for (uint32_t b = 0; b < n; ++b) {
        status[b] = block(b, t, &sink);
        sp->block_first[b + 1] = (uint32_t)t.n;
    }
    return PHANT_OK;
}

static int32_t block_receipt_segments_impl(phant_ctx* c, const phant_rcpt_segs_in* in, phant_rcpt_segs_out* out, bool dev) {
    const char* const who = dev ? "block_receipt_segments_dev" : "block_receipt_segments";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_rcpt_segs_in) || out->struct_size != sizeof(phant_rcpt_segs_out)) return bad("wrong struct_size");
    if (in->form > PHANT_RCPTS_ETH69) return bad("unknown form");
    if (in->reserved[0] != 0u || in->reserved[1] != 0u) return bad("reserved is not 0");
    const uint32_t n = in->n, nb = in->n_blocks;
    if (nb == 0) {  // (no block: nothing to index, nothing to write but the scalars)
        if (n) return bad("receipts without a block");
        out->first_bad_block = 0, out->n_logs = 0, out->n_topics = 0, out->encoded_len = 0;
        return PHANT_OK;
    }
    if (!in->block_first) return bad("null block_first");
    if (n && (!in->receipts || !in->rc_off)) return bad("null receipts / rc_off");
    if (dev) {  // (kernels read the offsets and the per-block integers as words; the outputs arrive by copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->rc_off | (uintptr_t)in->gas_used | (uintptr_t)out->cum_gas | (uintptr_t)out->gas_used | (uintptr_t)out->data_at |
                             (uintptr_t)out->encoded_off | (uintptr_t)out->block_gas_used;
        const uintptr_t w4 = (uintptr_t)in->block_first | (uintptr_t)in->tx_count | (uintptr_t)out->log_first | (uintptr_t)out->flags | (uintptr_t)out->log_receipt |
                             (uintptr_t)out->topic_first | (uintptr_t)out->data_len | (uintptr_t)out->block_first_bad | (uintptr_t)out->block_flags;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    phant_rcpt_segs_out res = *out;
    const int32_t rc = phant::block_receipt_segments(c->ws, c->stream, *in, res, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    out->first_bad_block = res.first_bad_block, out->n_logs = res.n_logs, out->n_topics = res.n_topics, out->encoded_len = res.encoded_len;
    return PHANT_OK;
}

int32_t phant_block_receipt_segments(phant_ctx* c, const phant_rcpt_segs_in* in, phant_rcpt_segs_out* out) {
    return block_receipt_segments_impl(c, in, out, false);
}

int32_t phant_block_receipt_segments_dev(phant_ctx* c, const phant_rcpt_segs_in* in, phant_rcpt_segs_out* out) {
    return block_receipt_segments_impl(c, in, out, true);
}

/* ------------------------------------------------- execution requests of a chain segment (requests.hip.h) */

static int32_t block_requests_impl(phant_ctx* c, const phant_requests_in* in, phant_requests_out* out, bool dev) {
    const char* const who = dev ? "block_requests_dev" : "block_requests";
    if (!c) return PHANT_E_INVALID_ARG;
    if (const char* const what = phant::qreq::check_args(in, out, dev); *what) return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str());
    if (in->n_blocks == 0) {  // (no block: nothing to index, nothing to write but the scalars)
        out->n_deposits = 0, out->first_bad_block = 0;
        return PHANT_OK;
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    phant_requests_out res = *out;
    const int32_t rc = phant::block_requests(c->ws, c->stream, *in, res, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    out->n_deposits = res.n_deposits, out->first_bad_block = res.first_bad_block;
    return PHANT_OK;
}

int32_t phant_block_requests(phant_ctx* c, const phant_requests_in* in, phant_requests_out* out) { return block_requests_impl(c, in, out, false); }

int32_t phant_block_requests_dev(phant_ctx* c, const phant_requests_in* in, phant_requests_out* out) { return block_requests_impl(c, in, out, true); }

/* ------------------------------------------------- log filters over a chain segment (filters.hip.h) */

static int32_t block_log_filters_impl(phant_ctx* c, const phant_logmatch_in* in, const phant_log_filters* filters, phant_logmatch_out* out, bool dev) {
    const char* const who = dev ? "block_log_filters_dev" : "block_log_filters";
    if (!c) return PHANT_E_INVALID_ARG;
    if (const char* const what = phant::lf::check_match_args(in, filters, out, dev); *what) return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str());
    if (filters->n_filters == 0) {  // (no filter: nothing to index, nothing to write but the scalar)
        out->n_matches = 0;
        return PHANT_OK;
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    phant_logmatch_out res = *out;
    // every non-empty set through the table: none is small; every set entry by entry: none is large
    const uint32_t linear_max = c->logfilter_sets == 1u ? 0u : c->logfilter_sets == 2u ? 0xffffffffu : PHANT_LOGFILTER_LINEAR_MAX;
    const int32_t rc = phant::block_log_filters(c->ws, c->stream, *in, *filters, res, dev, c->ns_salt, linear_max, err);
    if (rc) return fail(c, rc, err.c_str());
    out->n_matches = res.n_matches;
    return PHANT_OK;
}

int32_t phant_block_log_filters(phant_ctx* c, const phant_logmatch_in* in, const phant_log_filters* filters, phant_logmatch_out* out) {
    return block_log_filters_impl(c, in, filters, out, false);
}

int32_t phant_block_log_filters_dev(phant_ctx* c, const phant_logmatch_in* in, const phant_log_filters* filters, phant_logmatch_out* out) {
    return block_log_filters_impl(c, in, filters, out, true);
}

static int32_t log_filters_bloom_impl(phant_ctx* c, const uint8_t* blooms, uint32_t n_blooms, const phant_log_filters* filters, uint64_t* may, uint32_t* may_count, bool dev) {
    const char* const who = dev ? "log_filters_bloom_dev" : "log_filters_bloom";
    if (!c) return PHANT_E_INVALID_ARG;
    if (const char* const what = phant::lf::check_bloom_args(blooms, n_blooms, filters, may, may_count, dev); *what)
        return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str());
    if (filters->n_filters == 0) return PHANT_OK;  // (no filter: no word, no count)
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    const int32_t rc = phant::log_filters_bloom(c->ws, c->stream, blooms, n_blooms, *filters, may, may_count, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_log_filters_bloom(phant_ctx* c, const uint8_t* blooms, uint32_t n_blooms, const phant_log_filters* filters, uint64_t* may, uint32_t* may_count) {
    return log_filters_bloom_impl(c, blooms, n_blooms, filters, may, may_count, false);
}

int32_t phant_log_filters_bloom_dev(phant_ctx* c, const uint8_t* d_blooms, uint32_t n_blooms, const phant_log_filters* filters, uint64_t* d_may, uint32_t* d_may_count) {
    return log_filters_bloom_impl(c, d_blooms, n_blooms, filters, d_may, d_may_count, true);
}

/* ------------------------------------------------- fee history over a chain segment (fee_history.hip.h) */

static int32_t block_fee_history_impl(phant_ctx* c, const phant_fee_history_in* in, phant_fee_history_out* out, bool dev) {
    const char* const who = dev ? "block_fee_history_dev" : "block_fee_history";
    if (!c) return PHANT_E_INVALID_ARG;
    if (const char* const what = phant::fh::check_args(in, out, dev); *what) return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str());
    if (const char* const what = phant::fh::check_percentiles(*in); *what) return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str());
    if (in->n_blocks == 0) {  // (no block: nothing to index, nothing to write but the scalar)
        out->first_bad_block = 0;
        return PHANT_OK;
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    phant_fee_history_out res = *out;
    const int32_t rc = phant::block_fee_history(c->ws, c->stream, *in, res, dev, phant::fh::block_max_of(c->feehist_block_max), err);
    if (rc) return fail(c, rc, err.c_str());
    out->first_bad_block = res.first_bad_block;
    return PHANT_OK;
}

int32_t phant_block_fee_history(phant_ctx* c, const phant_fee_history_in* in, phant_fee_history_out* out) { return block_fee_history_impl(c, in, out, false); }

int32_t phant_block_fee_history_dev(phant_ctx* c, const phant_fee_history_in* in, phant_fee_history_out* out) { return block_fee_history_impl(c, in, out, true); }

/* ------------------------------------------------- a block's transactions against the pre-state (txstate.hip.h) */

static int32_t block_txs_prestate_impl(phant_ctx* c, const phant_txstate_in* in, phant_txstate_out* out, bool dev) {
    const char* const who = dev ? "block_txs_prestate_dev" : "block_txs_prestate";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_txstate_in) || out->struct_size != sizeof(phant_txstate_out)) return bad("wrong struct_size");
    if (in->fork > PHANT_TXS_FORK_PRAGUE) return bad("unknown fork");
    if (in->reserved != 0u) return bad("reserved is not 0");
    if (in->n && (!in->sender || !in->sig_status || !in->tx_flags || !in->nonce || !in->upfront_cost || !in->to)) return bad("null transaction array");
    if (in->n_auth && (!in->authority || !in->auth_status)) return bad("null authority / auth_status");
    if (in->n_accounts && (!in->addresses || !in->account_status || !in->nonces || !in->balances || !in->code_hashes || !in->code_index))
        return bad("null pre-state array");
    if (in->n_codes && !in->code_off) return bad("null code_off");
    if (in->code_bytes && !in->codes) return bad("null codes");
    if (in->n_probe && !in->probe) return bad("null probe");
    if (in->n_accounts > 0x7fffffffu) return fail(c, PHANT_E_UNSUPPORTED, (std::string(who) + ": 2^31 pre-state rows or more").c_str());
    if (dev) {  // (kernels read these as words; the outputs arrive by device-to-device copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->nonce | (uintptr_t)in->nonces | (uintptr_t)in->code_off | (uintptr_t)out->expected_nonce;
        const uintptr_t w4 = (uintptr_t)in->tx_flags | (uintptr_t)in->auth_first | (uintptr_t)in->code_index | (uintptr_t)out->sender_row |
                             (uintptr_t)out->to_row | (uintptr_t)out->state_flags | (uintptr_t)out->sends | (uintptr_t)out->probe_row;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    const int32_t rc = phant::block_txs_prestate(c->ws, c->stream, *in, *out, dev, c->ns_salt, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_block_txs_prestate(phant_ctx* c, const phant_txstate_in* in, phant_txstate_out* out) { return block_txs_prestate_impl(c, in, out, false); }

int32_t phant_block_txs_prestate_dev(phant_ctx* c, const phant_txstate_in* in, phant_txstate_out* out) { return block_txs_prestate_impl(c, in, out, true); }

/* ------------------------------------------------- a block of plain transfers settled (settle.hip.h) */

static int32_t block_settle_impl(phant_ctx* c, const phant_settle_in* in, phant_settle_out* out, bool dev) {
    const char* const who = dev ? "block_settle_dev" : "block_settle";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_settle_in) || out->struct_size != sizeof(phant_settle_out)) return bad("wrong struct_size");
    if (in->fork > PHANT_TXS_FORK_PRAGUE) return bad("unknown fork");
    if (in->reserved[0] != 0u || in->reserved[1] != 0u) return bad("reserved is not 0");
    if (!in->base_fee) return bad("null base_fee");
    if (in->n && (!in->type || !in->tx_flags || !in->gas_limit || !in->intrinsic_gas || !in->value || !in->effective_gas_price || !in->upfront_cost ||
                  !in->to || !in->sender_row || !in->to_row || !in->state_flags))
        return bad("null transaction array");
    if (in->n_accounts && (!in->account_status || !in->nonces || !in->balances || !in->code_hashes)) return bad("null pre-state array");
    if (in->n_wd && (!in->wd_row || !in->wd_amount_gwei)) return bad("null wd_row / wd_amount_gwei");
    if (in->coinbase_row != PHANT_ROW_NONE && in->coinbase_row >= in->n_accounts) return bad("coinbase_row is neither a pre-state row nor the NONE value");
    if (in->n_accounts > 0x7fffffffu || 3ull * in->n + in->n_wd > 0x7fffffffull)
        return fail(c, PHANT_E_UNSUPPORTED, (std::string(who) + ": 2^31 pre-state rows or balance events or more").c_str());
    if (dev) {  // (kernels read these as words; the outputs arrive by device-to-device copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->gas_limit | (uintptr_t)in->intrinsic_gas | (uintptr_t)in->floor_gas | (uintptr_t)in->nonces |
                             (uintptr_t)in->wd_amount_gwei | (uintptr_t)out->cumulative_gas_used | (uintptr_t)out->nonces_after;
        const uintptr_t w4 = (uintptr_t)in->tx_flags | (uintptr_t)in->sender_row | (uintptr_t)in->to_row | (uintptr_t)in->state_flags |
                             (uintptr_t)in->wd_row | (uintptr_t)out->settle_flags;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    const int32_t rc = phant::block_settle(c->ws, c->stream, *in, *out, dev, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_block_settle(phant_ctx* c, const phant_settle_in* in, phant_settle_out* out) { return block_settle_impl(c, in, out, false); }

int32_t phant_block_settle_dev(phant_ctx* c, const phant_settle_in* in, phant_settle_out* out) { return block_settle_impl(c, in, out, true); }

/* ------------------------------------------------- a block's access lists against the pre-state tables (access_lists.hip.h) */

static int32_t block_access_lists_impl(phant_ctx* c, const phant_access_in* in, phant_access_out* out, bool dev) {
    const char* const who = dev ? "block_access_lists_dev" : "block_access_lists";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_access_in) || out->struct_size != sizeof(phant_access_out)) return bad("wrong struct_size");
    if (in->reserved[0] != 0u || in->reserved[1] != 0u) return bad("reserved is not 0");
    if (in->n && (!in->al_off || !in->al_len)) return bad("null al_off / al_len");
    if (in->n && in->tx_bytes && !in->txs) return bad("null txs");
    if (in->n_accounts && (!in->addresses || !in->slot_first)) return bad("null addresses / slot_first");
    if (in->n_accounts && in->n_slots && !in->slots) return bad("null slots");
    if (in->n_accounts > (1u << 30) || (in->n_accounts && in->n_slots > (1u << 30)))
        return fail(c, PHANT_E_UNSUPPORTED, (std::string(who) + ": more than 2^30 pre-state rows or slots").c_str());
    if (dev) {  // (kernels read these as words; the outputs arrive by device-to-device copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->al_off;
        const uintptr_t w4 = (uintptr_t)in->al_len | (uintptr_t)in->slot_first | (uintptr_t)out->tuple_first | (uintptr_t)out->al_flags |
                             (uintptr_t)out->warm_addresses | (uintptr_t)out->warm_keys | (uintptr_t)out->key_first | (uintptr_t)out->account_row |
                             (uintptr_t)out->tuple_same | (uintptr_t)out->slot_row | (uintptr_t)out->key_same;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    }
    if (in->n == 0) {  // no totals, and the one entry of tuple_first and of key_first
        out->n_tuples = out->n_keys = out->n_missing_accounts = out->n_missing_slots = out->first_malformed = 0;
        const uint32_t zero = 0;
        if (dev && (out->tuple_first || out->key_first)) {
            DeviceGuard g(c->device);
            if (out->tuple_first) HIP_TRY(c, hipMemcpyAsync(out->tuple_first, &zero, 4, hipMemcpyHostToDevice, c->stream));
            if (out->key_first) HIP_TRY(c, hipMemcpyAsync(out->key_first, &zero, 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        } else if (!dev) {
            if (out->tuple_first) out->tuple_first[0] = zero;
            if (out->key_first) out->key_first[0] = zero;
        }
        return PHANT_OK;
    }
    DeviceGuard g(c->device);
    TimedRegion t(c, dev);
    std::string err;
    const int32_t rc = phant::block_access_lists(c->ws, c->stream, *in, *out, dev, c->ns_salt, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_block_access_lists(phant_ctx* c, const phant_access_in* in, phant_access_out* out) { return block_access_lists_impl(c, in, out, false); }

int32_t phant_block_access_lists_dev(phant_ctx* c, const phant_access_in* in, phant_access_out* out) { return block_access_lists_impl(c, in, out, true); }

int32_t phant_diag_secp_op(phant_ctx* c, uint32_t op, const uint8_t* a, const uint8_t* b, uint32_t n, uint8_t* out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (op >= PHANT_DIAG_SECP_OPS) return fail(c, PHANT_E_INVALID_ARG, "diag_secp_op: unknown op");
    if (n == 0) return PHANT_OK;
    const bool two = op == 0 || op == 4 || op == 7 || op == 8;
    if (!a || !out || (two && !b)) return fail(c, PHANT_E_INVALID_ARG, "diag_secp_op: null pointer");
    const size_t in_row = op >= 6 ? 65 : 32, out_row = op >= 6 ? 65 : op == 3 ? 33 : 32;
    DeviceGuard g(c->device);
    uint8_t *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        d_a = io.template take<uint8_t>(n * in_row);
        d_b = io.template take<uint8_t>(n * in_row);
        d_out = io.template take<uint8_t>(n * out_row);
    });
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_a, a, n * in_row, hipMemcpyHostToDevice, c->stream));
    if (two) HIP_TRY(c, hipMemcpyAsync(d_b, b, n * in_row, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, phant::launch_secp_op(op, d_a, d_b, n, d_out, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, d_out, n * out_row, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PHANT_OK;
}

// phant_diag_scan_u32 / _sort_pairs / _order_digests: a device buffer of exactly `bytes` bytes (a multiple of 4: what launch.h's size
// functions give) with GUARD_BYTES of 0xEE directly behind it, so that a kernel that writes past what its launcher asked for is caught.
namespace {
constexpr size_t GUARD_BYTES = 256;
struct Guarded {
    const char* name;
    size_t bytes;
    uint8_t* p = nullptr;
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};
template <size_t N>
int32_t carve_guarded(phant_ctx* c, Guarded (&b)[N]) {
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) {
        for (Guarded& g : b) g.p = io.template take<uint8_t>(g.bytes + GUARD_BYTES);
    });
    if (rc) return rc;
    for (const Guarded& g : b) HIP_TRY(c, hipMemsetAsync(g.p + g.bytes, 0xEE, GUARD_BYTES, c->stream));
    return PHANT_OK;
}
// (synchronises the ctx stream: the call's results are in host memory behind it, too)
template <size_t N>
int32_t check_guards(phant_ctx* c, const char* who, const Guarded (&b)[N]) {
    std::vector<uint8_t> seen(N * GUARD_BYTES);
    for (size_t i = 0; i < N; ++i)
        HIP_TRY(c, hipMemcpyAsync(seen.data() + i * GUARD_BYTES, b[i].p + b[i].bytes, GUARD_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < N; ++i)
        for (size_t k = 0; k < GUARD_BYTES; ++k)
            if (seen[i * GUARD_BYTES + k] != 0xEE)
                return fail(c, PHANT_E_DEVICE, (std::string(who) + ": the guard behind " + b[i].name + " (" + std::to_string(b[i].bytes) +
                                                " bytes) was written at byte " + std::to_string(k)).c_str());
    return PHANT_OK;
}
}  // namespace

int32_t phant_diag_scan_u32(phant_ctx* c, uint32_t* counters, uint32_t n) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n == 0) return PHANT_OK;
    if (!counters) return fail(c, PHANT_E_INVALID_ARG, "diag_scan_u32: null pointer");
    DeviceGuard g(c->device);
    Guarded b[2] = {{"counters", 4 * (size_t)n}, {"scan scratch", 4 * phant::scan_scratch_entries(n)}};
    const int32_t rc = carve_guarded(c, b);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(b[0].p, counters, b[0].bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, phant::launch_exclusive_scan_u32(b[0].as<uint32_t>(), n, b[1].as<uint32_t>(), c->stream));
    HIP_TRY(c, hipMemcpyAsync(counters, b[0].p, b[0].bytes, hipMemcpyDeviceToHost, c->stream));
    return check_guards(c, "diag_scan_u32", b);
}

int32_t phant_diag_sort_pairs(phant_ctx* c, const uint64_t* keys, const uint32_t* vals, uint32_t n, uint32_t bits, uint64_t* keys_out,
                              uint32_t* vals_out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (bits > 64u) return fail(c, PHANT_E_INVALID_ARG, "diag_sort_pairs: more than 64 key bits");
    if (n == 0) return PHANT_OK;
    if (!keys || !vals || !keys_out || !vals_out) return fail(c, PHANT_E_INVALID_ARG, "diag_sort_pairs: null pointer");
    DeviceGuard g(c->device);
    const size_t kb = 8 * (size_t)n, vb = 4 * (size_t)n;
    Guarded b[6] = {{"keys", kb},       {"alternate keys", kb}, {"values", vb}, {"alternate values", vb}, {"digit table", 4 * phant::sort_hist_entries(n)},
                    {"digit totals", 512 * 4}};
    const int32_t rc = carve_guarded(c, b);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(b[0].p, keys, kb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b[2].p, vals, vb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(b[5].p, 0, b[5].bytes, c->stream));
    uint64_t* d_keys = nullptr;
    uint32_t* d_vals = nullptr;
    HIP_TRY(c, phant::launch_sort_pairs(b[0].as<uint64_t>(), b[2].as<uint32_t>(), b[1].as<uint64_t>(), b[3].as<uint32_t>(), n, bits, b[4].as<uint32_t>(),
                                        b[5].as<uint32_t>(), &d_keys, &d_vals, c->stream));
    HIP_TRY(c, hipMemcpyAsync(keys_out, d_keys, kb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(vals_out, d_vals, vb, hipMemcpyDeviceToHost, c->stream));
    return check_guards(c, "diag_sort_pairs", b);
}

int32_t phant_diag_order_digests(phant_ctx* c, const uint8_t* digests, const uint32_t* seg_of, uint32_t n, uint32_t n_seg, uint32_t prefix_bits,
                                 uint32_t* order_out, uint32_t* flag_out) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (!flag_out || (n && (!digests || !order_out))) return fail(c, PHANT_E_INVALID_ARG, "diag_order_digests: null pointer");
    if (seg_of)
        for (uint32_t i = 0; i < n; ++i)
            if (seg_of[i] >= n_seg) return fail(c, PHANT_E_INVALID_ARG, "diag_order_digests: a segment index beyond n_seg");
    DeviceGuard g(c->device);
    Guarded b[3] = {{"digests", 32 * (size_t)n}, {"segments", seg_of ? 4 * (size_t)n : 0}, {"order workspace", phant::order_workspace_bytes(n)}};
    const int32_t rc = carve_guarded(c, b);
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(b[0].p, digests, b[0].bytes, hipMemcpyHostToDevice, c->stream));
    if (n && seg_of) HIP_TRY(c, hipMemcpyAsync(b[1].p, seg_of, b[1].bytes, hipMemcpyHostToDevice, c->stream));
    uint32_t *d_order = nullptr, *d_flag = nullptr;
    HIP_TRY(c, phant::launch_order_digests(b[0].p, seg_of ? b[1].as<uint32_t>() : nullptr, n, n_seg, b[2].p, &d_order, &d_flag, prefix_bits, c->stream));
    if (n) HIP_TRY(c, hipMemcpyAsync(order_out, d_order, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(flag_out, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    return check_guards(c, "diag_order_digests", b);
}

/* ------------------------------------------------------- proof verification */

// helper stream + events of the two-tier pipeline (created on first use)
static int32_t ensure_side(phant_ctx* c) {
    const bool need = c->dedup_levels != 0;
    if (!need || c->side.stream) return PHANT_OK;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->side.stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side.fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side.join, hipEventDisableTiming));
    // (diagnostics, phant_verify_bound_experiment: the clean read stream runs on a helper stream of its own)
    HIP_TRY(c, hipStreamCreateWithFlags(&c->side.stream2, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side.join2, hipEventDisableTiming));
    return PHANT_OK;
}

// The workspace `sp` sized for total_nodes and the epoch of the next launch on it (stream `st`).
static int32_t nodeset_prepare(phant_ctx* c, uint32_t total_nodes, hipStream_t st, NodesetSpace& sp) {
    if (total_nodes > sp.cap_nodes || !sp.dv.base) {
        const uint32_t cap = phant::verify_nodeset_capacity(total_nodes);
        HIP_TRY(c, hipStreamSynchronize(st));
        sp.cap_nodes = 0;
        hipError_t e = sp.dv.reset(phant::verify_nodeset_workspace_bytes(cap));
        if (e != hipSuccess) return fail(c, PHANT_E_OOM, "hipMalloc(node-set workspace)", e);
        sp.cap_nodes = cap;
        sp.dirty = true;
    }
    if (sp.dirty || sp.epoch >= 0xfffffff0u) {
        HIP_TRY(c, hipMemsetAsync(sp.dv.base, 0, sp.dv.cap, st));
        sp.epoch = 0;
        sp.dirty = false;
    }
    ++sp.epoch;
    if (&sp == &c->ns) c->last_was_nodeset = true;
    return PHANT_OK;
}

// The ctx's tune for a launch on `sp`; on the ctx's own workspace the launcher notes what it chose (phant_nodeset_stats).
static phant::NodesetTune nodeset_tune_on(phant_ctx* c, const NodesetSpace& sp) {
    phant::NodesetTune t = c->ns_tune;
    t.last = &sp == &c->ns ? c->ns_last : nullptr;
    return t;
}

namespace {

// A copy in of an array that may be empty, and a copy back that the caller may not want (a NULL destination): neither is a copy.
hipError_t up(void* dst, const void* src, size_t bytes, hipStream_t s) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}
hipError_t back(void* dst, const void* src, size_t bytes, hipStream_t s) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
}

// The pre-state stage of the execution-witness calls, once for phant_exec_witness_prestate and poststate_run:
//   copies -> trie keys -> node-set hash -> account walk -> account decode -> slot walk -> slot decode
// The set is hashed ONCE; the accounts walk from the trusted root, the slots from the storage roots the account leaves prove.  A
// caller carves inside its own lay_out, calls nodeset_prepare(c->ns) before it queues anything, and may put work of its own between
// the two launch steps.  `p`'s code side (nc, code_index, codes .. salt1) is the pre-state call's own.
struct PrestateStage {
    uint32_t na = 0, ns = 0, total_nodes = 0, n_counters = 0;
    size_t nk = 0, pre_len = 0, nodes_len = 0;
    uint8_t *pre = nullptr, *keys = nullptr, *root = nullptr, *nodes = nullptr;
    uint64_t *poff = nullptr, *noff = nullptr, *avoff = nullptr, *svoff = nullptr;
    uint32_t *sacc = nullptr, *avlen = nullptr, *svlen = nullptr;
    phant::PrestateArgs p{};

    // the stage's part of the call's layout; counters: the words behind p.counters (PRE_CNT_*, then the caller's own)
    template <class Arena>
    void carve(Arena& a, const phant::ExecWitness& w, uint32_t counters) {
        p.na = na = w.n_accounts;
        p.ns = ns = w.n_slots;
        total_nodes = (uint32_t)(w.node_off.size() - 1);
        n_counters = counters;
        nk = (size_t)na + ns;
        pre_len = w.preimages.size();
        nodes_len = w.nodes.size();
        pre = a.template take<uint8_t>(pre_len + 16);
        poff = a.template take<uint64_t>(nk + 1);
        keys = a.template take<uint8_t>(nk * 32);
        root = a.template take<uint8_t>(32);
        p.storage_roots = a.template take<uint8_t>((size_t)na * 32);
        p.slot_account = sacc = a.template take<uint32_t>(ns);
        p.nodes = nodes = a.template take<uint8_t>(nodes_len + 16);
        noff = a.template take<uint64_t>((size_t)total_nodes + 1);
        p.acc_status = a.template take<uint8_t>(na);
        p.acc_voff = avoff = a.template take<uint64_t>(na);
        p.acc_vlen = avlen = a.template take<uint32_t>(na);
        p.slot_status = a.template take<uint8_t>(ns);
        p.slot_voff = svoff = a.template take<uint64_t>(ns);
        p.slot_vlen = svlen = a.template take<uint32_t>(ns);
        p.nonces = a.template take<uint64_t>(na);
        p.balances = a.template take<uint8_t>((size_t)na * 32);
        p.code_hashes = a.template take<uint8_t>((size_t)na * 32);
        p.slot_vals = a.template take<uint8_t>((size_t)ns * 32);
        p.counters = a.template take<uint32_t>(counters);
    }
    // the witness and the root the caller trusts on their way in (an empty array is no copy), the counters zeroed
    hipError_t upload(const phant::ExecWitness& w, const uint8_t* trusted_root, hipStream_t s) const {
        hipError_t e = up(pre, w.preimages.data(), pre_len, s);
        if (e == hipSuccess) e = up(poff, w.preimage_off.data(), (nk + 1) * 8, s);
        if (e == hipSuccess) e = up(root, trusted_root, 32, s);
        if (e == hipSuccess) e = up(sacc, w.slot_account.data(), (size_t)ns * 4, s);
        if (e == hipSuccess) e = up(nodes, w.nodes.data(), nodes_len, s);
        if (e == hipSuccess) e = up(noff, w.node_off.data(), ((size_t)total_nodes + 1) * 8, s);
        return e == hipSuccess ? hipMemsetAsync(p.counters, 0, (size_t)n_counters * 4, s) : e;
    }
    // secure-trie keys: keccak256(address) / keccak256(slot), one batched launch
    hipError_t hash_keys(hipStream_t s) const { return phant::launch_keccak256_var(pre, poff, (uint32_t)nk, keys, s); }
    // ... and everything behind them, on c->ns at the epoch nodeset_prepare took.  A failure (the first one is returned) leaves the
    // workspace dirty, whatever part of the launch ran: the next one starts from zeroed memory.
    hipError_t resolve(phant_ctx* c, hipStream_t s) const {
        NodesetSpace& sp = c->ns;
        const phant::VerifyArgs acc{root, 1, nullptr, keys, 32, nodes, nodes_len, noff, nullptr, na, p.acc_status, avoff, avlen};
        const phant::VerifyArgs sto{p.storage_roots, na, sacc, keys + 32ull * na, 32, nodes, nodes_len, noff, nullptr, ns,
                                    p.slot_status, svoff, svlen};
        hipError_t e = phant::launch_nodeset_hash(acc, total_nodes, sp.cap_nodes, sp.dv.base, sp.epoch, c->ns_salt, s, nodeset_tune_on(c, sp));
        if (e == hipSuccess) e = phant::launch_nodeset_walk(acc, sp.cap_nodes, sp.dv.base, sp.epoch, c->ns_salt, s);
        if (e == hipSuccess) e = phant::launch_prestate_accounts(p, s);
        if (e == hipSuccess) e = phant::launch_nodeset_walk(sto, sp.cap_nodes, sp.dv.base, sp.epoch, c->ns_salt, s);
        if (e == hipSuccess) e = phant::launch_prestate_slots(p, s);
        if (e != hipSuccess) sp.dirty = true;
        return e;
    }
    // the pre-state fields of the post-state build's arguments
    void fill(phant::PoststateArgs& q) const {
        q.nodes = nodes;
        q.nodes_len = nodes_len;
        q.na = na;
        q.ns = ns;
        q.keys = keys;
        q.parent_root = root;
        q.acc_status = p.acc_status;
        q.slot_status = p.slot_status;
        q.acc_voff = avoff;
        q.acc_vlen = avlen;
        q.slot_voff = svoff;
        q.slot_vlen = svlen;
        q.pre_nonces = p.nonces;
        q.pre_balances = p.balances;
        q.pre_sroots = p.storage_roots;
        q.pre_code_hashes = p.code_hashes;
        q.slot_account = sacc;
        q.counters = p.counters;
    }
};

}  // namespace

// Where a verify call runs: a stream and the workspaces that go with it, the ctx's own or a streaming slot's.
struct Lane {
    hipStream_t stream;
    phant::DevArena& io;          // staging of the host forms
    phant::DevArena& dv;          // workspace of the per-proof pipeline
    NodesetSpace& ns;             // ... of the node-set pipeline
    const phant::FlatSide* side;  // per-proof form: the ctx's helper stream (null: the two tiers one after the other)
    bool timed;                   // inside phant_timing's events
};
static Lane ctx_lane(phant_ctx* c, bool timed) { return {c->stream, c->ws.io, c->dv, c->ns, &c->side, timed}; }
static Lane slot_lane(phant_ctx::Slot& sl) { return {sl.stream, sl.io, sl.dv, sl.ns, nullptr, false}; }

// Runs the pipeline of a's form (a.proof_first_node == nullptr: the node-set one) on device-resident arguments, on w's stream
// with w's workspaces.  What phant_verify_stats and phant_verify_kernel_ms report follows the ctx's own workspaces only.
static int32_t run_verify(phant_ctx* c, const Lane& w, phant::VerifyArgs a, uint32_t total_nodes) {
    if (!a.proof_first_node) {
        const int32_t rc = nodeset_prepare(c, total_nodes, w.stream, w.ns);
        if (rc) return rc;
        hipError_t e;
        {
            TimedRegion t(c, w.timed);
            e = phant::launch_mpt_verify_nodeset(a, total_nodes, w.ns.cap_nodes, w.ns.dv.base, w.ns.epoch, c->ns_salt, w.stream,
                                                 nodeset_tune_on(c, w.ns));
        }
        if (e != hipSuccess) {
            w.ns.dirty = true;  // (whatever part of the launch ran: the next one starts from zeroed memory)
            return fail(c, PHANT_E_DEVICE, "launch_mpt_verify_nodeset", e);
        }
        return PHANT_OK;
    }
    if (w.side) {
        const int32_t rc = ensure_side(c);
        if (rc) return rc;
    }
    a.total_nodes = total_nodes;
    const size_t need = phant::verify_workspace_bytes(total_nodes);
    if (need > w.dv.cap) {
        HIP_TRY(c, hipStreamSynchronize(w.stream));
        hipError_t e = w.dv.reset(need);
        if (e != hipSuccess) return fail(c, PHANT_E_OOM, "hipMalloc(verify workspace)", e);
        // (the pipeline validates whatever its group table holds -- it never clears it --, so this is not needed for
        // correctness; it keeps the first launch on fresh memory deterministic)
        HIP_TRY(c, hipMemsetAsync(w.dv.base, 0, w.dv.cap, w.stream));
    }
    const bool own = &w.dv == &c->dv;
    if (own) c->last_was_nodeset = false;
    {
        TimedRegion t(c, w.timed);
        HIP_TRY(c, phant::launch_mpt_verify(a, total_nodes, w.dv.base, c->dedup_levels, w.stream, w.side, c->tune));
    }
    // phant_verify_kernel_ms reads the per-kernel events of THIS launch or nothing: a launch that took the S = 0 form (or ran
    // the tiers next to each other) recorded none
    if (own) c->kev_valid = c->tune.serial && c->tune.kernel_ev && c->last_shallow != 0u;
    return PHANT_OK;
}

// Results of a call that went through the pinned staging buffer: where they wait for the stream to finish
struct StagedResults {
    const uint8_t *status = nullptr, *value_off = nullptr, *value_len = nullptr;  // inside c->ws.stage (null: not staged)
};
static void deliver_staged(const StagedResults& r, uint32_t n, uint8_t* status, uint64_t* value_off, uint32_t* value_len) {
    if (!r.status) return;
    std::memcpy(status, r.status, n);
    if (value_off) std::memcpy(value_off, r.value_off, (size_t)n * 8);
    if (value_len) std::memcpy(value_len, r.value_len, (size_t)n * 4);
}

// Stage a host witness `h` (arrays in host memory; h.proof_first_node == nullptr: a node set of h.total_nodes nodes) into w.io,
// run the pipeline there and queue the copies of the results back into the caller's buffers.  Does NOT wait; after a failure
// nothing of the call stays in flight.  d_fail_out != null: the per-root verdict, left on the device.  staged_out != null:
// small batches on the ctx's own arena may go through c->ws.stage; the caller then synchronises the stream and calls
// deliver_staged().
static int32_t stage_and_verify(phant_ctx* c, const Lane& w, const phant::VerifyArgs& h, uint32_t** d_fail_out = nullptr,
                                 StagedResults* staged_out = nullptr) {
    const bool nodeset = !h.proof_first_node;
    const uint32_t n = h.n, n_roots = h.n_roots;
    // The number of node offsets the caller provided is what the LAST entry of proof_first_node says
    // (include/phant_gpu.h): node_off has proof_first_node[n] + 1 entries.  An earlier entry that points
    // beyond it makes its proofs BAD_INPUT on the device; it never widens what is read from the caller.
    const uint32_t total_nodes = nodeset ? h.total_nodes : h.proof_first_node[n];
    uint8_t *d_roots = nullptr, *d_keys = nullptr, *d_nodes = nullptr, *d_status = nullptr;
    uint32_t *d_ridx = nullptr, *d_pfn = nullptr, *d_vlen = nullptr, *d_fail = nullptr;
    uint64_t *d_noff = nullptr, *d_voff = nullptr;
    const auto lay = [&](auto& io) {
        d_roots = io.template take<uint8_t>((size_t)n_roots * 32);
        d_ridx = io.template take<uint32_t>(n);
        d_keys = io.template take<uint8_t>((size_t)n * h.key_len + 4);
        d_nodes = io.template take<uint8_t>((size_t)h.nodes_len + 16);
        d_noff = io.template take<uint64_t>((size_t)total_nodes + 1);
        if (!nodeset) d_pfn = io.template take<uint32_t>((size_t)n + 1);
        d_status = io.template take<uint8_t>(n);
        d_voff = io.template take<uint64_t>(n);
        d_vlen = io.template take<uint32_t>(n);
        d_fail = io.template take<uint32_t>(n_roots);
    };
    const int32_t rc = [&]() -> int32_t {
        {
            const int32_t lrc = lay_out(c, w.stream, w.io, lay);
            if (lrc) return lrc;
        }
        // Small batches (the witness of an ordinary block): the arena's layout mirrored in pinned memory, one copy in, one out
        const bool staged = staged_out != nullptr && &w.io == &c->ws.io && w.io.used <= phant::Workspaces::STAGE_BYTES;
        if (staged) {
            hipError_t e = c->ws.ensure_stage();
            if (e != hipSuccess) return fail(c, PHANT_E_OOM, "hipHostMalloc(staging)", e);
        }
        auto put = [&](void* d_dst, const void* src, size_t bytes) -> hipError_t {
            if (!bytes) return hipSuccess;
            if (!staged) return hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, w.stream);
            uint8_t* const hp = c->ws.staged(static_cast<uint8_t*>(d_dst));
            std::memcpy(hp, src, bytes);
            // (sanitizer test builds poison the arena's padding: array by array there)
            return PHANT_ARENA_POISONS ? hipMemcpyAsync(d_dst, hp, bytes, hipMemcpyHostToDevice, w.stream) : hipSuccess;
        };
        HIP_TRY(c, put(d_roots, h.roots, (size_t)n_roots * 32));
        if (h.root_idx) HIP_TRY(c, put(d_ridx, h.root_idx, (size_t)n * 4));
        if (h.key_len) HIP_TRY(c, put(d_keys, h.keys, (size_t)n * h.key_len));
        if (h.nodes_len) HIP_TRY(c, put(d_nodes, h.nodes, (size_t)h.nodes_len));
        HIP_TRY(c, put(d_noff, h.node_off, ((size_t)total_nodes + 1) * 8));
        if (!nodeset) HIP_TRY(c, put(d_pfn, h.proof_first_node, ((size_t)n + 1) * 4));
        if (staged && !PHANT_ARENA_POISONS)  // [roots .. proof_first_node]: consecutive allocations of the arena
            HIP_TRY(c, hipMemcpyAsync(w.io.base, c->ws.stage, (size_t)(reinterpret_cast<uint8_t*>(d_pfn + n + 1) - w.io.base),
                                      hipMemcpyHostToDevice, w.stream));
        phant::VerifyArgs a{d_roots, n_roots, h.root_idx ? d_ridx : nullptr, d_keys, h.key_len, d_nodes, h.nodes_len,
                            d_noff, d_pfn, n, d_status, d_voff, d_vlen};
        if (staged) {
            // the results are written straight into the pinned buffer (hipHostMalloc memory is mapped into the device's address
            // space and coherent): no copy back, the caller's stream synchronisation makes them visible
            a.status = c->ws.staged(d_status);
            a.value_off = c->ws.staged(d_voff);
            a.value_len = c->ws.staged(d_vlen);
        }
        if (d_fail_out) {
            *d_fail_out = d_fail;
            a.fail_count = d_fail;
        }
        {
            const int32_t vrc = run_verify(c, w, a, total_nodes);
            if (vrc) return vrc;
        }
        if (staged) {  // [status .. value_len]: consecutive as well
            staged_out->status = a.status;
            staged_out->value_off = reinterpret_cast<const uint8_t*>(a.value_off);
            staged_out->value_len = reinterpret_cast<const uint8_t*>(a.value_len);
            return PHANT_OK;
        }
        HIP_TRY(c, hipMemcpyAsync(h.status, d_status, n, hipMemcpyDeviceToHost, w.stream));
        if (h.value_off) HIP_TRY(c, hipMemcpyAsync(h.value_off, d_voff, (size_t)n * 8, hipMemcpyDeviceToHost, w.stream));
        if (h.value_len) HIP_TRY(c, hipMemcpyAsync(h.value_len, d_vlen, (size_t)n * 4, hipMemcpyDeviceToHost, w.stream));
        return PHANT_OK;
    }();
    if (rc) (void)hipStreamSynchronize(w.stream);  // nothing of a failed call stays in flight
    return rc;
}

// The argument contract of the verify entry points, both forms (nodeset: no proof_first_node).  host: the arrays are the
// caller's, so the node blob must be there whenever nodes_len says so.  verdict: a _verdict_dev call, which owes its counts
// even for n == 0 -- the per-proof form insists on them, the node-set form zeroes them when it has them.
// -> PHANT_OK (run it), NOTHING_TO_DO (n == 0) or the error.
constexpr int32_t NOTHING_TO_DO = 1;
static int32_t check_verify_args(phant_ctx* c, const phant::VerifyArgs& a, bool nodeset, bool host, bool verdict, const char* what) {
    auto refuse = [&]() { return fail(c, PHANT_E_INVALID_ARG, (std::string(what) + ": bad argument").c_str()); };
    if (verdict && !nodeset && (!a.fail_count || a.n_roots == 0)) return refuse();
    if (a.n == 0) {
        if (verdict && a.fail_count && a.n_roots)
            HIP_TRY(c, hipMemsetAsync(a.fail_count, 0, sizeof(uint32_t) * (size_t)a.n_roots, c->stream));
        return NOTHING_TO_DO;
    }
    if (!a.roots || a.n_roots == 0 || !a.node_off || !a.status || (a.key_len && !a.keys) || a.key_len > 0x3fffffffu ||
        (!nodeset && !a.proof_first_node) || (host && a.nodes_len && !a.nodes))
        return refuse();
    return PHANT_OK;
}

// The device forms: on the ctx's own stream, arrays already on the device.
static int32_t verify_dev(phant_ctx* c, const phant::VerifyArgs& a, uint32_t total_nodes, bool nodeset, bool verdict,
                          const char* what) {
    if (!c) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    const int32_t rc = check_verify_args(c, a, nodeset, false, verdict, what);
    if (rc != PHANT_OK) return rc == NOTHING_TO_DO ? PHANT_OK : rc;
    return run_verify(c, ctx_lane(c, true), a, total_nodes);
}

// The host forms: staged through the ctx's own arena, waited for.
static int32_t verify_host(phant_ctx* c, const phant::VerifyArgs& h, bool nodeset, const char* what) {
    if (!c) return PHANT_E_INVALID_ARG;
    DeviceGuard g(c->device);
    int32_t rc = check_verify_args(c, h, nodeset, true, false, what);
    if (rc != PHANT_OK) return rc == NOTHING_TO_DO ? PHANT_OK : rc;
    StagedResults staged;  // (the per-proof form only: pinned staging for node sets is not measured)
    rc = stage_and_verify(c, ctx_lane(c, true), h, nullptr, nodeset ? nullptr : &staged);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    deliver_staged(staged, h.n, h.status, h.value_off, h.value_len);
    return PHANT_OK;
}

// The streaming forms: staged and queued on the slot's own stream; phant_wait collects them.
static int32_t verify_submit(phant_ctx* c, uint32_t slot, const phant::VerifyArgs& h, bool nodeset, const char* what) {
    if (!c || slot >= PHANT_MAX_SLOTS) return PHANT_E_INVALID_ARG;
    phant_ctx::Slot& sl = c->slots[slot];
    if (sl.busy) return fail(c, PHANT_E_INVALID_ARG, (std::string(what) + ": slot still in flight (phant_wait it first)").c_str());
    DeviceGuard g(c->device);
    int32_t rc = check_verify_args(c, h, nodeset, true, false, what);
    if (rc != PHANT_OK) return rc == NOTHING_TO_DO ? PHANT_OK : rc;
    if (!sl.stream) HIP_TRY(c, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    rc = stage_and_verify(c, slot_lane(sl), h);
    if (rc) return rc;
    sl.busy = true;
    return PHANT_OK;
}

constexpr bool PROOFS = false, NODESET = true;

int32_t phant_mpt_verify_batch_dev(phant_ctx* c, const uint8_t* d_roots, uint32_t n_roots,
                                   const uint32_t* d_root_idx, const uint8_t* d_keys,
                                   uint32_t key_len, const uint8_t* d_nodes, uint64_t nodes_len,
                                   const uint64_t* d_node_off, uint32_t total_nodes,
                                   const uint32_t* d_proof_first_node, uint32_t n, uint8_t* d_status,
                                   uint64_t* d_value_off, uint32_t* d_value_len) {
    const phant::VerifyArgs a{d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len,
                              d_node_off, d_proof_first_node, n, d_status, d_value_off, d_value_len};
    return verify_dev(c, a, total_nodes, PROOFS, false, "mpt_verify_batch_dev");
}

int32_t phant_verify_bound_experiment(phant_ctx* c, const uint8_t* d_roots, uint32_t n_roots, const uint32_t* d_root_idx,
                                      const uint8_t* d_keys, uint32_t key_len, const uint8_t* d_nodes, uint64_t nodes_len,
                                      const uint64_t* d_node_off, uint32_t total_nodes, const uint32_t* d_proof_first_node,
                                      uint32_t n, uint8_t* d_status, uint32_t reps, float out_ms[3]) {
    if (!c || !out_ms || reps == 0) return PHANT_E_INVALID_ARG;
    out_ms[0] = out_ms[1] = out_ms[2] = 0.f;
    if (c->tune.serial) return fail(c, PHANT_E_UNSUPPORTED, "bound_experiment: needs the two tiers next to each other");
    if (((uintptr_t)d_nodes & 15u) != 0) return fail(c, PHANT_E_INVALID_ARG, "bound_experiment: the node blob must be 16-byte aligned");
    // one complete launch: its lists and counts are what the hashing-only launches below work from
    int32_t rc = phant_impl::phant_mpt_verify_batch_dev(c, d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len, d_node_off,
                                            total_nodes, d_proof_first_node, n, d_status, nullptr, nullptr);
    if (rc) return rc;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->last_form == 0u) return fail(c, PHANT_E_INVALID_ARG, "bound_experiment: the batch is hashed whole (no shallow tier)");
    phant::VerifyArgs a{d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len,
                        d_node_off, d_proof_first_node, n, d_status, nullptr, nullptr};
    a.total_nodes = total_nodes;
    phant::VerifyTune tune = c->tune;
    tune.last_shallow = nullptr;
    tune.last_form = nullptr;
    tune.diag_sink = reinterpret_cast<uint32_t*>(c->dv.base + 4096);  // (header words nothing of these launches reads)
    for (uint32_t what = 1; what <= 3u; ++what) {
        tune.diag = what;
        // (a warm-up, then `reps` back-to-back, events around them on the ctx stream)
        HIP_TRY(c, phant::launch_mpt_verify(a, total_nodes, c->dv.base, c->dedup_levels, c->stream, &c->side, tune));
        HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
        for (uint32_t k = 0; k < reps; ++k)
            HIP_TRY(c, phant::launch_mpt_verify(a, total_nodes, c->dv.base, c->dedup_levels, c->stream, &c->side, tune));
        HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        out_ms[what - 1u] = ms / (float)reps;
    }
    return PHANT_OK;
}

int32_t phant_mpt_verify_verdict_dev(phant_ctx* c, const uint8_t* d_roots, uint32_t n_roots,
                                     const uint32_t* d_root_idx, const uint8_t* d_keys,
                                     uint32_t key_len, const uint8_t* d_nodes, uint64_t nodes_len,
                                     const uint64_t* d_node_off, uint32_t total_nodes,
                                     const uint32_t* d_proof_first_node, uint32_t n, uint8_t* d_status,
                                     uint64_t* d_value_off, uint32_t* d_value_len, uint32_t* d_fail_count) {
    const phant::VerifyArgs a{d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len,
                              d_node_off, d_proof_first_node, n, d_status, d_value_off, d_value_len, d_fail_count};
    return verify_dev(c, a, total_nodes, PROOFS, true, "mpt_verify_verdict_dev");
}

int32_t phant_mpt_verdict_dev(phant_ctx* c, const uint8_t* d_status, const uint32_t* d_root_idx,
                              uint32_t n, uint32_t n_roots, uint32_t* d_fail_count) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n_roots == 0 || !d_fail_count || (n && !d_status))
        return fail(c, PHANT_E_INVALID_ARG, "mpt_verdict_dev: bad argument");
    DeviceGuard g(c->device);
    HIP_TRY(c, phant::launch_mpt_verdict(d_status, d_root_idx, n, n_roots, d_fail_count, c->stream));
    return PHANT_OK;
}

int32_t phant_mpt_verify_batch(phant_ctx* c, const uint8_t* roots, uint32_t n_roots,
                               const uint32_t* root_idx, const uint8_t* keys, uint32_t key_len,
                               const uint8_t* nodes, uint64_t nodes_len, const uint64_t* node_off,
                               const uint32_t* proof_first_node, uint32_t n, uint8_t* status,
                               uint64_t* value_off, uint32_t* value_len) {
    const phant::VerifyArgs h{roots, n_roots, root_idx, keys, key_len, nodes, nodes_len,
                              node_off, proof_first_node, n, status, value_off, value_len};
    return verify_host(c, h, PROOFS, "mpt_verify_batch");
}

/* -------------------------------------------------------------- node-set witnesses */

int32_t phant_mpt_verify_nodeset_verdict_dev(phant_ctx* c, const uint8_t* d_roots, uint32_t n_roots, const uint32_t* d_root_idx,
                                             const uint8_t* d_keys, uint32_t key_len, const uint8_t* d_nodes, uint64_t nodes_len,
                                             const uint64_t* d_node_off, uint32_t total_nodes, uint32_t n, uint8_t* d_status,
                                             uint64_t* d_value_off, uint32_t* d_value_len, uint32_t* d_fail_count) {
    const phant::VerifyArgs a{d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len, d_node_off, nullptr, n,
                              d_status, d_value_off, d_value_len, d_fail_count};
    return verify_dev(c, a, total_nodes, NODESET, true, "mpt_verify_nodeset_verdict_dev");
}

int32_t phant_mpt_verify_nodeset_dev(phant_ctx* c, const uint8_t* d_roots, uint32_t n_roots, const uint32_t* d_root_idx,
                                     const uint8_t* d_keys, uint32_t key_len, const uint8_t* d_nodes, uint64_t nodes_len,
                                     const uint64_t* d_node_off, uint32_t total_nodes, uint32_t n, uint8_t* d_status,
                                     uint64_t* d_value_off, uint32_t* d_value_len) {
    const phant::VerifyArgs a{d_roots, n_roots, d_root_idx, d_keys, key_len, d_nodes, nodes_len, d_node_off, nullptr, n,
                              d_status, d_value_off, d_value_len};
    return verify_dev(c, a, total_nodes, NODESET, false, "mpt_verify_nodeset_dev");
}

int32_t phant_mpt_verify_nodeset(phant_ctx* c, const uint8_t* roots, uint32_t n_roots, const uint32_t* root_idx,
                                 const uint8_t* keys, uint32_t key_len, const uint8_t* nodes, uint64_t nodes_len,
                                 const uint64_t* node_off, uint32_t total_nodes, uint32_t n, uint8_t* status,
                                 uint64_t* value_off, uint32_t* value_len) {
    phant::VerifyArgs h{roots, n_roots, root_idx, keys, key_len, nodes, nodes_len, node_off, nullptr, n, status, value_off, value_len};
    h.total_nodes = total_nodes;
    return verify_host(c, h, NODESET, "mpt_verify_nodeset");
}

/* ------------------------------------------------------------------ range proofs (range_verify.hip.h) */

// One run with room for cap_items items: carve -> (host form) one staged upload / (device form) the offsets' check -> node-set hash ->
// the range kernels -> one copy back.  *need_items: the list's length (beyond cap_items nothing was built).
static int32_t verify_ranges_run(phant_ctx* c, const phant_ranges_in& in, phant_ranges_out& out, bool dev, uint32_t cap_items, uint32_t* need_items) {
    const char* const who = dev ? "mpt_verify_ranges_dev" : "mpt_verify_ranges";
    const uint32_t R = in.n_ranges, L = in.n_leaves, N = in.n_nodes, lanes = L + 2u * R;
    hipStream_t s = c->stream;
    phant::Workspaces& ws = c->ws;
    HIP_TRY(c, ws.ensure_mailbox());
    phant::RangeArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_ranges = R, a.n_leaves = L, a.n_nodes = N, a.vals_len = in.vals_len, a.nodes_len = in.nodes_len;
    a.roots = in.roots, a.origins = in.origins, a.leaf_first = in.leaf_first, a.has_proof = in.has_proof, a.keys = in.keys, a.vals = in.vals,
    a.val_off = in.val_off, a.nodes = in.nodes, a.node_off = in.node_off;
    a.cap_items = cap_items;
    a.leaf_pass = c->ranges_no_leaf_pass ? 0u : 1u;
    // the arena: the zeroed words and the outputs in front (one span goes back), (host form) the inputs, then the workspace
    const size_t zero_words = (size_t)phant::RANGE_CTL_WORDS + 8 + 4 * (size_t)R;  // ctl, counters, walk_err x 2, more, trie_bad
    uint32_t* zero = nullptr;
    uint8_t *in_begin = nullptr, *in_end = nullptr;
    uint8_t *d_roots = nullptr, *d_origins = nullptr, *d_hp = nullptr, *d_keys = nullptr, *d_vals = nullptr, *d_nodes = nullptr;
    uint32_t* d_lf = nullptr;
    uint64_t *d_voff = nullptr, *d_noff = nullptr;
    const auto carve = [&](auto& io) {
        zero = io.template take<uint32_t>(zero_words);
        a.status = io.template take<uint8_t>(R);
        a.has_more = io.template take<uint8_t>(R);
        a.computed_root = io.template take<uint8_t>((size_t)R * 32);
        a.out_bad_leaf = io.template take<uint32_t>(R);
        if (!dev) {
            in_begin = d_roots = io.template take<uint8_t>((size_t)R * 32);
            d_origins = io.template take<uint8_t>((size_t)R * 32);
            d_lf = io.template take<uint32_t>((size_t)R + 1);
            d_hp = io.template take<uint8_t>(R);
            d_keys = io.template take<uint8_t>((size_t)L * 32 + 4);
            d_vals = io.template take<uint8_t>((size_t)in.vals_len + 16);
            d_voff = io.template take<uint64_t>((size_t)L + 1);
            d_nodes = io.template take<uint8_t>((size_t)in.nodes_len + 16);
            d_noff = io.template take<uint64_t>((size_t)N + 1);
            in_end = io.template take<uint8_t>(0);
        }
        a.bad_leaf = io.template take<uint32_t>(R);
        a.built_root = io.template take<uint8_t>((size_t)R * 32);
        a.cnt = io.template take<uint32_t>((size_t)lanes + 4);
        a.scan_scratch = io.template take<uint32_t>(phant::scan_scratch_entries(lanes + 1u) + 4);
        a.items_raw = io.template take<uint8_t>((size_t)cap_items * phant::POSTSTATE_ITEM_BYTES);
    };
    if (const int32_t rc = lay_out(c, s, ws.io, carve)) return rc;
    a.ctl = zero, a.counters = zero + phant::RANGE_CTL_WORDS, a.walk_err = a.counters + 8, a.more = a.walk_err + 2 * (size_t)R, a.trie_bad = a.more + R;
    if (const int32_t rc = nodeset_prepare(c, N, s, c->ns)) return rc;
    HIP_TRY(c, hipMemsetAsync(zero, 0, 4 * zero_words, s));
    HIP_TRY(c, hipMemsetAsync(a.bad_leaf, 0xff, 4 * (size_t)R, s));
    if (!dev) {
        phant::StagedInputs ins(ws, s, in_begin, in_end);
        ins.put(d_roots, in.roots, (size_t)R * 32);
        ins.put(d_origins, in.origins, (size_t)R * 32);
        ins.put(d_lf, in.leaf_first, ((size_t)R + 1) * 4);
        ins.put(d_hp, in.has_proof, R);
        ins.put(d_keys, in.keys, (size_t)L * 32);
        ins.put(d_vals, in.vals, (size_t)in.vals_len);
        if (L) ins.put(d_voff, in.val_off, ((size_t)L + 1) * 8);
        ins.put(d_nodes, in.nodes, (size_t)in.nodes_len);
        if (N) ins.put(d_noff, in.node_off, ((size_t)N + 1) * 8);
        HIP_TRY(c, ins.finish());
        a.roots = d_roots, a.origins = d_origins, a.leaf_first = d_lf, a.has_proof = d_hp, a.keys = d_keys, a.vals = d_vals,
        a.val_off = L ? d_voff : nullptr, a.nodes = d_nodes, a.node_off = N ? d_noff : nullptr;
    } else {
        HIP_TRY(c, phant::launch_range_check(a, s));
        HIP_TRY(c, ws.read_words(phant::Workspaces::MAILBOX_RANGES, a.ctl, phant::RANGE_CTL_WORDS, s));
        if (ws.mailbox[phant::Workspaces::MAILBOX_RANGES + phant::RANGE_CTL_CHECK])
            return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": leaf_first / val_off / node_off do not run from 0 to their totals without going backwards").c_str());
    }
    {
        TimedRegion t(c);
        phant::VerifyArgs v{};
        v.nodes = a.nodes, v.nodes_len = a.nodes_len, v.node_off = a.node_off, v.n = R, v.total_nodes = N;
        hipError_t e = phant::launch_nodeset_hash(v, N, c->ns.cap_nodes, c->ns.dv.base, c->ns.epoch, c->ns_salt, s, nodeset_tune_on(c, c->ns));
        if (e == hipSuccess) e = phant::launch_range_verify(a, c->ns.cap_nodes, c->ns.dv.base, c->ns.epoch, c->ns_salt, s);
        if (e != hipSuccess) {
            c->ns.dirty = true;
            (void)hipStreamSynchronize(s);
            return fail(c, PHANT_E_DEVICE, (std::string(who) + ": launch").c_str(), e);
        }
    }
    // out: the control words and everything up to the last wanted output (a run whose list outgrew its room has built nothing and
    // left the outputs alone: what goes back then is overwritten by the run with the counted room)
    phant::CallOutputs outs(ws, s, dev, a.ctl, a.ctl, phant::Workspaces::MAILBOX_RANGES, phant::RANGE_CTL_WORDS);
    outs.add(out.status, a.status, R);
    outs.add(out.has_more, a.has_more, R);
    outs.add(out.computed_root, a.computed_root, (size_t)R * 32);
    outs.add(out.bad_leaf, a.out_bad_leaf, (size_t)R * 4);
    HIP_TRY(c, outs.deliver());
    const volatile uint32_t* const w = outs.ctl();
    *need_items = w[phant::RANGE_CTL_ITEMS];
    out.n_failed = w[phant::RANGE_CTL_FAILED], out.first_failed = R - w[phant::RANGE_CTL_FIRST];
    return PHANT_OK;
}

static int32_t verify_ranges_impl(phant_ctx* c, const phant_ranges_in* in, phant_ranges_out* out, bool dev) {
    const char* const who = dev ? "mpt_verify_ranges_dev" : "mpt_verify_ranges";
    auto bad = [&](const char* what) { return fail(c, PHANT_E_INVALID_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!c) return PHANT_E_INVALID_ARG;
    if (!in || !out) return bad("in / out is null");
    if (in->struct_size != sizeof(phant_ranges_in) || out->struct_size != sizeof(phant_ranges_out)) return bad("wrong struct_size");
    if (in->reserved[0] != 0u || in->reserved[1] != 0u || out->reserved[0] != 0u || out->reserved[1] != 0u) return bad("reserved is not 0");
    const uint32_t R = in->n_ranges, L = in->n_leaves, N = in->n_nodes;
    if (R && (!in->roots || !in->leaf_first || !in->has_proof)) return bad("null roots / leaf_first / has_proof");
    if (L && (!in->keys || !in->val_off)) return bad("null keys / val_off");
    if (in->vals_len && !in->vals) return bad("null vals");
    if (N && !in->node_off) return bad("null node_off");
    if (in->nodes_len && !in->nodes) return bad("null nodes");
    if (R == 0 && (L || N)) return bad("leaves or nodes without a range");
    if (dev && R && !in->origins) return bad("null origins");
    if ((uint64_t)L + 2ull * R >= 0x7fffffffull) return fail(c, PHANT_E_UNSUPPORTED, (std::string(who) + ": 2^31 leaves + ranges or more").c_str());
    if (dev) {  // (kernels read these as words; the outputs arrive by device-to-device copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->val_off | (uintptr_t)in->node_off;
        const uintptr_t w4 = (uintptr_t)in->leaf_first | (uintptr_t)out->bad_leaf;
        if ((w8 & 7u) || (w4 & 3u)) return bad("misaligned array");
    } else if (R) {
        const char* const offsets = "leaf_first / val_off / node_off do not run from 0 to their totals without going backwards";
        if (in->leaf_first[0] != 0u || in->leaf_first[R] != L) return bad(offsets);
        for (uint32_t r = 0; r < R; ++r)
            if (in->leaf_first[r + 1] < in->leaf_first[r]) return bad(offsets);
        if (L && (in->val_off[0] != 0u || in->val_off[L] != in->vals_len)) return bad(offsets);
        if (!L && in->vals_len) return bad(offsets);
        for (uint32_t j = 0; j < L; ++j)
            if (in->val_off[j + 1] < in->val_off[j]) return bad(offsets);
        if (N && (in->node_off[0] != 0u || in->node_off[N] != in->nodes_len)) return bad(offsets);
        if (!N && in->nodes_len) return bad(offsets);
        for (uint32_t i = 0; i < N; ++i)
            if (in->node_off[i + 1] < in->node_off[i]) return bad(offsets);
        bool any_proof = false;
        for (uint32_t r = 0; r < R; ++r) any_proof = any_proof || in->has_proof[r] != 0u;
        if (any_proof && !in->origins) return bad("null origins");
    }
    if (R == 0) {
        out->n_failed = 0, out->first_failed = 0;
        return PHANT_OK;
    }
    if (dev && ((!L && in->vals_len) || (!N && in->nodes_len))) return bad("bytes without leaves / nodes");
    DeviceGuard g(c->device);
    // The item list: the leaves and what the two walks of a range leave beside their paths -- at most 2 x (64 x 15 + 1) = 1 922 per
    // range, and in a trie of 16^k keys about 15 k.  Room for sixteen full levels a walk (2 x 241 a range: a balanced trie of 2^64 keys)
    // is what an ordinary call gets; a list that outgrows it is counted exactly and the call's kernels run once more with that room.
    const uint64_t per_range = c->ranges_items_per_range >= 0 ? (uint64_t)c->ranges_items_per_range : 482u;
    uint64_t cap = (uint64_t)L + per_range * R + 64u;
    for (int attempt = 0;; ++attempt) {
        if (cap >= 0x40000000ull) return fail(c, PHANT_E_OOM, (std::string(who) + ": item list too long").c_str());
        uint32_t need = 0;
        const int32_t rc = verify_ranges_run(c, *in, *out, dev, (uint32_t)cap, &need);
        if (rc) return rc;
        if (need <= cap) return PHANT_OK;
        if (attempt == 1) return fail(c, PHANT_E_DEVICE, (std::string(who) + ": the item list did not settle").c_str());
        cap = need;
    }
}

int32_t phant_mpt_verify_ranges(phant_ctx* c, const phant_ranges_in* in, phant_ranges_out* out) { return verify_ranges_impl(c, in, out, false); }

int32_t phant_mpt_verify_ranges_dev(phant_ctx* c, const phant_ranges_in* in, phant_ranges_out* out) { return verify_ranges_impl(c, in, out, true); }

/* ------------------------------------------------------------------ streaming */

int32_t phant_host_alloc(phant_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    *out = nullptr;
    DeviceGuard g(c->device);
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, PHANT_E_OOM, "hipHostMalloc", e);
    return PHANT_OK;
}

int32_t phant_host_free(phant_ctx* c, void* p) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (!p) return PHANT_OK;
    DeviceGuard g(c->device);
    HIP_TRY(c, hipHostFree(p));
    return PHANT_OK;
}

int32_t phant_mpt_verify_submit(phant_ctx* c, uint32_t slot, const uint8_t* roots, uint32_t n_roots,
                                const uint32_t* root_idx, const uint8_t* keys, uint32_t key_len,
                                const uint8_t* nodes, uint64_t nodes_len, const uint64_t* node_off,
                                const uint32_t* proof_first_node, uint32_t n, uint8_t* status,
                                uint64_t* value_off, uint32_t* value_len) {
    const phant::VerifyArgs h{roots, n_roots, root_idx, keys, key_len, nodes, nodes_len,
                              node_off, proof_first_node, n, status, value_off, value_len};
    return verify_submit(c, slot, h, PROOFS, "mpt_verify_submit");
}

int32_t phant_mpt_verify_nodeset_submit(phant_ctx* c, uint32_t slot, const uint8_t* roots, uint32_t n_roots, const uint32_t* root_idx,
                                        const uint8_t* keys, uint32_t key_len, const uint8_t* nodes, uint64_t nodes_len,
                                        const uint64_t* node_off, uint32_t total_nodes, uint32_t n, uint8_t* status,
                                        uint64_t* value_off, uint32_t* value_len) {
    phant::VerifyArgs h{roots, n_roots, root_idx, keys, key_len, nodes, nodes_len, node_off, nullptr, n, status, value_off, value_len};
    h.total_nodes = total_nodes;
    return verify_submit(c, slot, h, NODESET, "mpt_verify_nodeset_submit");
}

int32_t phant_wait(phant_ctx* c, uint32_t slot) {
    if (!c || slot >= PHANT_MAX_SLOTS) return PHANT_E_INVALID_ARG;
    phant_ctx::Slot& sl = c->slots[slot];
    if (!sl.busy) return PHANT_OK;
    DeviceGuard g(c->device);
    sl.busy = false;
    HIP_TRY(c, hipStreamSynchronize(sl.stream));
    return PHANT_OK;
}

}  // namespace phant_impl

/* ------------------------------------------------- internal: what comm.hip (several devices in one process) builds on */
namespace phant {

// Stage a host witness of either form (stage_and_verify) on the ctx's own stream, verify it there with the per-root verdict
// left in a device array of the ctx, queue the copies of statuses / values back to the caller's buffers.  Does NOT wait.
int32_t ctx_stage_and_verify(phant_ctx* c, const VerifyArgs& h, uint32_t** d_fail) {
    DeviceGuard g(c->device);
    return phant_impl::stage_and_verify(c, phant_impl::ctx_lane(c, false), h, d_fail);
}
// a device array of n_roots zeroed counters owned by the ctx (a rank without proofs still takes part in the reduction)
int32_t ctx_zero_verdict(phant_ctx* c, uint32_t n_roots, uint32_t** d_fail) {
    DeviceGuard g(c->device);
    const int32_t rc = lay_out(c, c->stream, c->ws.io, [&](auto& io) { *d_fail = io.template take<uint32_t>(n_roots); });
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(*d_fail, 0, (size_t)n_roots * 4, c->stream));
    return PHANT_OK;
}
hipStream_t ctx_stream(phant_ctx* c) { return c->stream; }
int ctx_device(const phant_ctx* c) { return c->device; }

}  // namespace phant

namespace phant_impl {

/* ------------------------------------------------------------------ block witness */

using phant::account_absent_consistent;
using phant::account_consistent;
using phant::be_equals_padded;
using phant::host_rlp_item;

int32_t phant_witness_parse_json(const char* json, uint64_t len, phant_witness** out, char* err, uint32_t err_cap) {
    return phant_witness_parse_json_mt(json, len, 1, out, err, err_cap);
}

int32_t phant_witness_parse_json_mt(const char* json, uint64_t len, uint32_t threads, phant_witness** out, char* err,
                                    uint32_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out || (!json && len)) return PHANT_E_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<phant_witness> w(new (std::nothrow) phant_witness());  // (owned here until handed out: a parse that runs out of
    if (!w) return PHANT_E_OOM;                                            //  memory half way unwinds through this function)
    std::string msg;
    const bool parsed = threads == 1 ? phant::witness_parse_json(json, (size_t)len, w->w, msg)
                                     : phant::witness_parse_json_mt(json, (size_t)len, threads, w->w, msg);
    if (!parsed) {
        if (err && err_cap) {
            std::strncpy(err, msg.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return PHANT_E_INVALID_ARG;
    }
    *out = w.release();
    return PHANT_OK;
}

int32_t phant_witness_index_json(const char* json, uint64_t len, uint32_t threads, phant_witness** out, char* err,
                                 uint32_t err_cap) {
    if (!out || (!json && len)) return PHANT_E_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<phant_witness> w(new (std::nothrow) phant_witness());
    if (!w) return PHANT_E_OOM;
    std::string msg;
    if (!phant::witness_index_json(json, (size_t)len, threads, w->w, msg)) {
        if (err && err_cap) {
            std::strncpy(err, msg.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return PHANT_E_INVALID_ARG;
    }
    *out = w.release();
    return PHANT_OK;
}

void phant_witness_free(phant_witness* w) { delete w; }

int32_t phant_witness_get(const phant_witness* pw, phant_witness_info* info) {
    // (node_set is the struct's last member, added in round 6: a caller compiled against the shorter struct gets the rest)
    if (!pw || !info || info->struct_size < offsetof(phant_witness_info, node_set)) return PHANT_E_INVALID_ARG;
    if (info->struct_size >= sizeof(phant_witness_info)) info->node_set = pw->w.node_set ? 1u : 0u;
    const phant::Witness& w = pw->w;
    info->n_proofs = (uint32_t)w.root_idx.size();
    info->n_roots = (uint32_t)(w.roots.size() / 32);
    info->n_accounts = (uint32_t)w.accounts.size();
    info->n_slots = (uint32_t)w.slots.size();
    info->total_nodes = (uint32_t)(w.node_off.size() - 1);
    info->nodes_len = w.deferred ? w.nodes_bytes : (uint64_t)w.nodes.size();
    info->roots = w.roots.data();
    info->root_idx = w.root_idx.data();
    info->account_of = w.account_of.data();
    info->preimages = w.preimages.data();
    info->preimage_off = w.preimage_off.data();
    info->nodes = w.deferred ? nullptr : w.nodes.data();  // index form: the nodes are decoded on the device only
    info->node_off = w.node_off.data();
    info->proof_first_node = w.proof_first_node.data();
    return PHANT_OK;
}

int32_t phant_witness_to_json(const phant_witness* pw, char* buf, uint64_t cap, uint64_t* len_out) {
    if (!pw || !len_out || (!buf && cap)) return PHANT_E_INVALID_ARG;
    return phant::witness_to_json(pw->w, buf, cap, *len_out) ? PHANT_OK : PHANT_E_UNSUPPORTED;  // (the index form: its nodes were never decoded)
}

int32_t phant_witness_verify(phant_ctx* c, const phant_witness* pw, const uint8_t* expected_state_root, uint8_t* status,
                             uint32_t* n_failed) {
    if (!c || !pw) return PHANT_E_INVALID_ARG;
    const phant::Witness& w = pw->w;
    const uint32_t n = (uint32_t)w.root_idx.size();
    if (n_failed) *n_failed = 0;
    if (n == 0) return PHANT_OK;
    if (!status) return fail(c, PHANT_E_INVALID_ARG, "witness_verify: null status");
    const uint32_t n_roots = (uint32_t)(w.roots.size() / 32);
    const uint32_t total_nodes = (uint32_t)(w.node_off.size() - 1);
    // index form (phant_witness_index_json): the nodes' hex is still in the JSON text -- ship the text, decode on
    // the device, fetch only the proven values back for the consistency check
    const bool deferred = w.deferred;
    constexpr uint32_t VAL_CAP = 128;  // an account body is <= 110 bytes, a slot value <= 33
    const size_t nodes_len = deferred ? (size_t)w.nodes_bytes : w.nodes.size(), pre_len = w.preimages.size();
    if (deferred && total_nodes && !w.json) return fail(c, PHANT_E_INVALID_ARG, "witness_verify: index-form witness without its JSON text");
    DeviceGuard g(c->device);
    hipStream_t s = c->stream;
    uint8_t *d_pre, *d_keys, *d_roots, *d_nodes, *d_status, *d_json = nullptr, *d_vals = nullptr;
    uint64_t *d_poff, *d_noff, *d_voff, *d_src = nullptr;
    uint32_t *d_ridx, *d_pfn, *d_vlen, *d_err = nullptr;
    int32_t rc = lay_out(c, s, c->ws.io, [&](auto& io) {
        d_pre = io.template take<uint8_t>(pre_len + 16);
        d_poff = io.template take<uint64_t>((size_t)n + 1);
        d_keys = io.template take<uint8_t>((size_t)n * 32);
        d_roots = io.template take<uint8_t>((size_t)n_roots * 32);
        d_ridx = io.template take<uint32_t>(n);
        d_nodes = io.template take<uint8_t>(nodes_len + 16);
        d_noff = io.template take<uint64_t>((size_t)total_nodes + 1);
        d_pfn = io.template take<uint32_t>((size_t)n + 1);
        d_status = io.template take<uint8_t>(n);
        d_voff = io.template take<uint64_t>(n);
        d_vlen = io.template take<uint32_t>(n);
        if (deferred) {
            d_json = io.template take<uint8_t>(w.json_len + 16);
            d_src = io.template take<uint64_t>((size_t)total_nodes + 1);
            d_err = io.template take<uint32_t>(4);
            d_vals = io.template take<uint8_t>((size_t)n * VAL_CAP);
        }
    });
    if (rc) return rc;
    std::vector<uint64_t> poff64(w.preimage_off.begin(), w.preimage_off.end());
    HIP_TRY(c, hipMemcpyAsync(d_pre, w.preimages.data(), pre_len, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_poff, poff64.data(), poff64.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_roots, w.roots.data(), w.roots.size(), hipMemcpyHostToDevice, s));
    // root 0 = the state root: the one the caller trusts, not the one the document claims
    if (expected_state_root && n_roots) HIP_TRY(c, hipMemcpyAsync(d_roots, expected_state_root, 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_ridx, w.root_idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_noff, w.node_off.data(), ((size_t)total_nodes + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_pfn, w.proof_first_node.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    if (!deferred) {
        if (nodes_len) HIP_TRY(c, hipMemcpyAsync(d_nodes, w.nodes.data(), nodes_len, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(c, hipMemcpyAsync(d_json, w.json, w.json_len, hipMemcpyHostToDevice, s));
        if (total_nodes) HIP_TRY(c, hipMemcpyAsync(d_src, w.node_src.data(), (size_t)total_nodes * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, phant::launch_hex_decode(d_json, d_src, d_noff, total_nodes, d_nodes, d_err, s));
    }
    // secure-trie keys: keccak256(address) / keccak256(slot), one batched launch
    HIP_TRY(c, phant::launch_keccak256_var(d_pre, d_poff, n, d_keys, s));
    // the document's "state" array (w.node_set): every node once, references resolved by hash
    phant::VerifyArgs a{d_roots, n_roots, d_ridx, d_keys, 32, d_nodes, nodes_len, d_noff, w.node_set ? nullptr : d_pfn, n,
                        d_status, d_voff, d_vlen};
    rc = run_verify(c, ctx_lane(c, true), a, total_nodes);
    if (rc) return rc;
    std::vector<uint64_t> voff(n);
    std::vector<uint32_t> vlen(n);
    std::vector<uint8_t> vals;
    uint32_t herr[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(voff.data(), d_voff, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(vlen.data(), d_vlen, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (deferred) {
        vals.resize((size_t)n * VAL_CAP);
        HIP_TRY(c, phant::launch_gather_values(d_nodes, d_voff, d_vlen, n, VAL_CAP, d_vals, s));
        HIP_TRY(c, hipMemcpyAsync(vals.data(), d_vals, vals.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(herr, d_err, 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (deferred && herr[0]) {  // what the host parser says for the same document (witness_json.cpp)
        char msg[96];
        std::snprintf(msg, sizeof(msg), "witness_verify: proof node %u is not hex data", herr[1]);
        return fail(c, PHANT_E_INVALID_ARG, msg);
    }
    // where proof p's proven value can be read on the host (index form: the compacted copy, cut at VAL_CAP -- a
    // longer value is no account body / slot value and fails the checks below on its length)
    auto value_of = [&](uint32_t p) -> const uint8_t* {
        return deferred ? vals.data() + (size_t)p * VAL_CAP : w.nodes.data() + voff[p];
    };
    if (deferred)
        for (uint32_t p = 0; p < n; ++p)
            if (vlen[p] > VAL_CAP && status[p] == PHANT_PROOF_PRESENT) status[p] = PHANT_PROOF_MISMATCH;

    // ---- host: does what was proven agree with what the witness declares? ----
    std::vector<uint8_t> anchored(w.accounts.size(), 0);
    for (size_t ai = 0; ai < w.accounts.size(); ++ai) {
        const phant::WitnessAccount& acc = w.accounts[ai];
        uint8_t& st = status[acc.proof];
        if (st == PHANT_PROOF_PRESENT) {
            if (account_consistent(acc, value_of(acc.proof), vlen[acc.proof])) anchored[ai] = 1;
            else st = PHANT_PROOF_MISMATCH;
        } else if (st == PHANT_PROOF_ABSENT) {
            if (account_absent_consistent(acc)) anchored[ai] = 1;
            else st = PHANT_PROOF_MISMATCH;
        }
    }
    for (const phant::WitnessSlot& sl : w.slots) {
        uint8_t& st = status[sl.proof];
        if (st != PHANT_PROOF_PRESENT && st != PHANT_PROOF_ABSENT) continue;
        if (!anchored[sl.account]) {
            st = PHANT_PROOF_MISMATCH;  // verified against a storage root nothing commits to
            continue;
        }
        if (!sl.has_value) continue;
        static const uint8_t zero[32] = {0};
        if (st == PHANT_PROOF_ABSENT) {
            if (std::memcmp(sl.value, zero, 32) != 0) st = PHANT_PROOF_MISMATCH;
        } else {
            // slot value = rlp(minimal big-endian integer)
            size_t pay, len, total;
            bool is_list;
            const uint8_t* v = value_of(sl.proof);
            if (!host_rlp_item(v, vlen[sl.proof], pay, len, total, is_list) || is_list || total != vlen[sl.proof] ||
                !be_equals_padded(v + pay, len, sl.value))
                st = PHANT_PROOF_MISMATCH;
        }
    }
    if (n_failed) {
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n; ++i) bad += !(status[i] == PHANT_PROOF_PRESENT || status[i] == PHANT_PROOF_ABSENT);
        *n_failed = bad;
    }
    return PHANT_OK;
}

/* ------------------------------------------------------- execution witness -> pre-state */

int32_t phant_exec_witness_parse_json(const char* json, uint64_t len, phant_exec_witness** out, char* err, uint32_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out || (!json && len)) return PHANT_E_INVALID_ARG;
    *out = nullptr;
    std::unique_ptr<phant_exec_witness> w(new (std::nothrow) phant_exec_witness());
    if (!w) return PHANT_E_OOM;
    std::string msg;
    if (!phant::exec_witness_parse_json(json, (size_t)len, w->w, msg)) {
        if (err && err_cap) {
            std::strncpy(err, msg.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return PHANT_E_INVALID_ARG;
    }
    *out = w.release();
    return PHANT_OK;
}

void phant_exec_witness_free(phant_exec_witness* w) { delete w; }

int32_t phant_exec_witness_get(const phant_exec_witness* pw, phant_exec_witness_info* info) {
    if (!pw || !info || info->struct_size < sizeof(phant_exec_witness_info)) return PHANT_E_INVALID_ARG;
    const phant::ExecWitness& w = pw->w;
    info->n_accounts = w.n_accounts;
    info->n_slots = w.n_slots;
    info->n_codes = (uint32_t)(w.code_off.size() - 1);
    info->total_nodes = (uint32_t)(w.node_off.size() - 1);
    info->nodes_len = (uint64_t)w.nodes.size();
    info->code_bytes = (uint64_t)w.codes.size();
    info->addresses = w.preimages.data();
    info->slot_first = w.slot_first.data();
    info->slots = w.preimages.data() + 20 * (size_t)w.n_accounts;
    info->codes = w.codes.data();
    info->code_off = w.code_off.data();
    info->nodes = w.nodes.data();
    info->node_off = w.node_off.data();
    return PHANT_OK;
}

// helper stream + events of the code hashing (created on first use)
static int32_t ensure_code_side(phant_ctx* c) {
    if (c->code_side.stream) return PHANT_OK;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->code_side.stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->code_side.fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->code_side.join, hipEventDisableTiming));
    return PHANT_OK;
}

// Everything on the device, one synchronisation at the end:
//   ctx stream   copies -> fork --------------------------------------------------------------------------- join -> code_match -> copies
//                              \-> trie keys -> node-set hash -> account walk -> account decode -> slot walk -> slot decode /
//   helper stream               `-> table clear -> code hash ------------------------------------------------------------'
int32_t phant_exec_witness_prestate(phant_ctx* c, const phant_exec_witness* pw, const uint8_t* state_root, phant_prestate* out) {
    if (!c || !pw || !out) return PHANT_E_INVALID_ARG;
    if (out->struct_size < sizeof(phant_prestate)) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_prestate: struct_size too small");
    if (!state_root) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_prestate: the trusted state root is required");
    const phant::ExecWitness& w = pw->w;
    const uint32_t na = w.n_accounts, ns = w.n_slots, nc = (uint32_t)(w.code_off.size() - 1);
    const size_t code_bytes = w.codes.size();
    const uint32_t slots_t = phant::code_table_slots(nc);
    out->n_failed = out->n_missing_code = out->n_unused_codes = 0;
    DeviceGuard g(c->device);
    hipStream_t s = c->stream;
    uint8_t* d_codes;
    uint64_t* d_coff;
    PrestateStage st;
    phant::PrestateArgs& p = st.p;
    int32_t rc = lay_out(c, s, c->ws.io, [&](auto& io) {
        st.carve(io, w, 4);
        d_codes = io.template take<uint8_t>(code_bytes + 16);
        d_coff = io.template take<uint64_t>((size_t)nc + 1);
        p.code_index = io.template take<uint32_t>(na);
        p.code_dig = io.template take<uint32_t>((size_t)nc * 8);
        p.code_slot = io.template take<uint32_t>(nc);
        p.table = io.template take<uint32_t>(slots_t);
        p.table_used = io.template take<uint32_t>(slots_t);
    });
    if (rc) return rc;
    p.nc = nc;
    p.codes = d_codes;
    p.code_off = d_coff;
    p.mask = slots_t - 1u;
    p.salt0 = c->ns_salt[0];
    p.salt1 = c->ns_salt[1];
    rc = ensure_code_side(c);
    if (rc) return rc;
    if (na) {  // (the node-set workspace sized and its epoch taken before anything is queued: sizing it may wait for the stream)
        rc = nodeset_prepare(c, st.total_nodes, s, c->ns);
        if (rc) return rc;
    }
    if (code_bytes) HIP_TRY(c, hipMemcpyAsync(d_codes, w.codes.data(), code_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_coff, w.code_off.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, st.upload(w, state_root, s));
    {
        TimedRegion t(c);  // (phant_timing: the kernels of both streams, the copies in and out left out)
        HIP_TRY(c, hipEventRecord(c->code_side.fork, s));
        hipStream_t h = c->code_side.stream;
        HIP_TRY(c, hipStreamWaitEvent(h, c->code_side.fork, 0));
        HIP_TRY(c, hipMemsetAsync(p.table, 0, (size_t)slots_t * 4, h));
        HIP_TRY(c, hipMemsetAsync(p.table_used, 0, (size_t)slots_t * 4, h));
        HIP_TRY(c, phant::launch_code_hash(p, c->code_form, h));
        HIP_TRY(c, hipEventRecord(c->code_side.join, h));
        if (na) {
            HIP_TRY(c, st.hash_keys(s));
            const hipError_t e = st.resolve(c, s);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(h);
                return fail(c, PHANT_E_DEVICE, "exec_witness_prestate: node-set launch", e);
            }
        }
        HIP_TRY(c, hipStreamWaitEvent(s, c->code_side.join, 0));
        HIP_TRY(c, phant::launch_code_match(p, s));
    }
    uint32_t cnt[4] = {0, 0, 0, 0};
    HIP_TRY(c, back(out->account_status, p.acc_status, na, s));
    HIP_TRY(c, back(out->nonces, p.nonces, (size_t)na * 8, s));
    HIP_TRY(c, back(out->balances, p.balances, (size_t)na * 32, s));
    HIP_TRY(c, back(out->storage_roots, p.storage_roots, (size_t)na * 32, s));
    HIP_TRY(c, back(out->code_hashes, p.code_hashes, (size_t)na * 32, s));
    HIP_TRY(c, back(out->code_index, p.code_index, (size_t)na * 4, s));
    HIP_TRY(c, back(out->slot_status, p.slot_status, ns, s));
    HIP_TRY(c, back(out->slot_vals, p.slot_vals, (size_t)ns * 32, s));
    HIP_TRY(c, back(cnt, p.counters, 12, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    out->n_failed = cnt[phant::PRE_CNT_FAILED];
    out->n_missing_code = cnt[phant::PRE_CNT_MISSING_CODE];
    out->n_unused_codes = cnt[phant::PRE_CNT_UNUSED_CODES];
    return PHANT_OK;
}

/* ------------------------------------------------------- execution witness + writes -> post-state root */

// One run of the whole pipeline on the ctx stream, one synchronisation at its end:
//   copies -> trie keys -> node-set hash -> account walk -> account decode -> slot walk -> slot decode      (the pre-state's kernels)
//          -> actions -> key order -> count / scan / emit -> link -> storage tries, level by level -> state trie -> finish -> copies
// host_order (may be null): the keys' order when the device sort left it undecided.  *need_items: the length of the item list;
// *undecided: the device sort's flag; keys_back: the hashed keys.
// sink (null: phant_exec_witness_poststate, which allocates and copies nothing of it): phant_exec_witness_advance's room for the nodes
// the build hashes.  The whole room comes back with the other copies, in front of the one synchronisation; need_* say what the
// run would have filled.
struct AdvanceSink {
    uint64_t cap_bytes = 0;
    uint32_t cap_desc = 0;
    std::vector<uint8_t> blob;
    std::vector<phant::PoststateNodeDesc> desc;
    uint64_t need_bytes = 0;
    uint32_t need_desc = 0, overflow = 0;
};
static int32_t poststate_run(phant_ctx* c, const phant::ExecWitness& w, const uint8_t* parent_root, phant_poststate* io,
                             const uint32_t* host_order, uint32_t cap_items, uint32_t* need_items, uint32_t* undecided,
                             std::vector<uint8_t>& keys_back, uint32_t cnt[8], AdvanceSink* sink) {
    const uint32_t na = w.n_accounts, ns = w.n_slots;
    const size_t nk = (size_t)na + ns;
    hipStream_t s = c->stream;
    uint8_t *d_sort, *d_op, *d_pbal, *d_pch, *d_swr, *d_sval;
    uint64_t* d_pnonce;
    uint32_t *d_sfirst, *d_order_host;
    PrestateStage st;
    phant::PoststateArgs q{};
    const size_t sort_ws = phant::order_workspace_bytes((uint32_t)nk);
    int32_t rc = lay_out(c, s, c->ws.io, [&](auto& a) {
        st.carve(a, w, 8);
        d_sfirst = a.template take<uint32_t>((size_t)na + 1);
        d_op = a.template take<uint8_t>(na);
        d_pnonce = a.template take<uint64_t>(na);
        d_pbal = a.template take<uint8_t>((size_t)na * 32);
        d_pch = a.template take<uint8_t>((size_t)na * 32);
        d_swr = a.template take<uint8_t>(ns);
        d_sval = a.template take<uint8_t>((size_t)ns * 32);
        q.post_sroots = a.template take<uint8_t>((size_t)na * 32);
        q.state_root = a.template take<uint8_t>(32);
        q.acc_flag = a.template take<uint32_t>(na);
        q.act = a.template take<uint8_t>(nk);
        q.seg_of = a.template take<uint32_t>(nk);
        d_order_host = a.template take<uint32_t>(nk);
        q.key_bad = a.template take<uint8_t>(nk);
        q.cnt = a.template take<uint32_t>(nk + 4);
        q.scan_scratch = a.template take<uint32_t>(phant::scan_scratch_entries((uint32_t)nk + 1) + 4);
        q.items_raw = a.template take<uint8_t>((size_t)cap_items * phant::POSTSTATE_ITEM_BYTES);
        d_sort = a.template take<uint8_t>(sort_ws + 256);
        if (sink) {
            q.sink_blob = a.template take<uint8_t>(sink->cap_bytes + 16);
            q.sink_desc = a.template take<phant::PoststateNodeDesc>(sink->cap_desc);
            q.sink_bytes = a.template take<unsigned long long>(1);
            q.sink_cnt = a.template take<uint32_t>(2);
        }
    });
    if (rc) return rc;
    if (sink) {
        q.sink_cap_bytes = sink->cap_bytes;
        q.sink_cap_desc = sink->cap_desc;
    }
    st.fill(q);
    q.slot_first = d_sfirst;
    q.op = d_op;
    q.post_nonces = d_pnonce;
    q.post_balances = d_pbal;
    q.post_code_hashes = d_pch;
    q.slot_write = io->slot_write ? d_swr : nullptr;
    q.post_slot_vals = d_sval;
    q.cap_items = cap_items;
    rc = nodeset_prepare(c, st.total_nodes, s, c->ns);
    if (rc) return rc;
    HIP_TRY(c, st.upload(w, parent_root, s));
    HIP_TRY(c, up(d_sfirst, w.slot_first.data(), ((size_t)na + 1) * 4, s));
    HIP_TRY(c, up(d_op, io->account_op, na, s));
    // (the post arrays are only read where op == SET; an all-KEEP / DELETE call may leave them out)
    if (io->nonces) HIP_TRY(c, up(d_pnonce, io->nonces, (size_t)na * 8, s));
    if (io->balances) HIP_TRY(c, up(d_pbal, io->balances, (size_t)na * 32, s));
    if (io->code_hashes) HIP_TRY(c, up(d_pch, io->code_hashes, (size_t)na * 32, s));
    if (io->slot_write) {
        HIP_TRY(c, up(d_swr, io->slot_write, ns, s));
        HIP_TRY(c, up(d_sval, io->slot_vals, (size_t)ns * 32, s));
    }
    if (host_order) HIP_TRY(c, up(d_order_host, host_order, nk * 4, s));
    HIP_TRY(c, hipMemsetAsync(q.acc_flag, 0, (size_t)na * 4, s));
    HIP_TRY(c, hipMemsetAsync(q.key_bad, 0, nk, s));
    if (sink) {
        HIP_TRY(c, hipMemsetAsync(q.sink_bytes, 0, 8, s));
        HIP_TRY(c, hipMemsetAsync(q.sink_cnt, 0, 8, s));
    }
    uint32_t* d_flag = nullptr;
    {
        TimedRegion t(c);
        HIP_TRY(c, st.hash_keys(s));
        if (c->post_raw_slot_keys && ns)  // (tests: the slots' 32 bytes verbatim as their trie keys)
            HIP_TRY(c, hipMemcpyAsync(st.keys + 32ull * na, st.pre + 20ull * na, (size_t)ns * 32, hipMemcpyDeviceToDevice, s));
        hipError_t e = st.resolve(c, s);
        if (e == hipSuccess) e = phant::launch_poststate_actions(q, s);
        if (e == hipSuccess) {
            if (host_order) {
                q.order = d_order_host;
            } else {
                uint32_t* d_order = nullptr;
                e = phant::launch_order_digests(st.keys, q.seg_of, (uint32_t)nk, na + 1u, d_sort, &d_order, &d_flag, 0, s);
                q.order = d_order;
                if (sink) q.sink_undecided = d_flag;
            }
        }
        if (e == hipSuccess) e = phant::launch_poststate_build(q, c->ns.cap_nodes, c->ns.dv.base, c->ns.epoch, c->ns_salt, s);
        if (e != hipSuccess) {
            c->ns.dirty = true;  // (the build's launches write the same workspace)
            return fail(c, PHANT_E_DEVICE, "exec_witness_poststate: launch", e);
        }
    }
    keys_back.resize(nk * 32);
    *undecided = 0;
    HIP_TRY(c, back(io->account_status, q.acc_status, na, s));
    HIP_TRY(c, back(io->slot_status, q.slot_status, ns, s));
    HIP_TRY(c, back(io->storage_roots, q.post_sroots, (size_t)na * 32, s));
    HIP_TRY(c, back(io->state_root, q.state_root, 32, s));
    HIP_TRY(c, back(keys_back.data(), st.keys, nk * 32, s));
    HIP_TRY(c, back(cnt, q.counters, 32, s));
    if (d_flag) HIP_TRY(c, back(undecided, d_flag, 4, s));
    uint32_t sink_cnt[2] = {0, 0};
    unsigned long long sink_bytes = 0;
    if (sink) {
        sink->blob.resize(sink->cap_bytes);
        sink->desc.resize(sink->cap_desc);
        HIP_TRY(c, back(sink->blob.data(), q.sink_blob, sink->cap_bytes, s));
        HIP_TRY(c, back(sink->desc.data(), q.sink_desc, (size_t)sink->cap_desc * sizeof(phant::PoststateNodeDesc), s));
        HIP_TRY(c, back(&sink_bytes, q.sink_bytes, 8, s));
        HIP_TRY(c, back(sink_cnt, q.sink_cnt, 8, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    *need_items = cnt[phant::POST_CNT_ITEMS];
    if (sink) {
        sink->need_bytes = sink_bytes;
        sink->need_desc = sink_cnt[phant::POST_SINK_NODES];
        sink->overflow = sink_cnt[phant::POST_SINK_OVERFLOW];
    }
    return PHANT_OK;
}

// The call behind both entry points.  sink null: phant_exec_witness_poststate.  Otherwise the nodes of the last run are left in it
// (sink->need_desc of them) unless the call failed or reports no root.
static int32_t poststate_call(phant_ctx* c, const phant_exec_witness* pw, const uint8_t* parent_state_root, phant_poststate* io,
                              AdvanceSink* sink) {
    if (!c || !pw || !io) return PHANT_E_INVALID_ARG;
    if (io->struct_size != sizeof(phant_poststate)) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: wrong struct_size");
    if (!parent_state_root) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: the trusted parent state root is required");
    const phant::ExecWitness& w = pw->w;
    const uint32_t na = w.n_accounts, ns = w.n_slots;
    io->n_failed = 0;
    if (na && !io->account_op) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: account_op is null");
    bool any_set = false;
    for (uint32_t i = 0; i < na; ++i) {
        if (io->account_op[i] > PHANT_POST_DELETE) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: an account op outside 0..2");
        any_set = any_set || io->account_op[i] == PHANT_POST_SET;
    }
    if (any_set && (!io->nonces || !io->balances || !io->code_hashes))
        return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: an account is SET but nonces / balances / code_hashes is null");
    if (ns && io->slot_write && !io->slot_vals) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_poststate: slot_write without slot_vals");
    if (na == 0) {  // nothing is touched: the root stays
        if (io->state_root) std::memcpy(io->state_root, parent_state_root, 32);
        return PHANT_OK;
    }
    DeviceGuard g(c->device);
    const size_t nk = (size_t)na + ns;
    // the item list: a leaf per key and the other children of the branches on their paths -- at most one per reference the set's
    // bytes can hold in the usual case; a list that outgrows this is counted exactly and the call's kernels run again
    uint64_t cap = nk + w.nodes.size() / 16u + 1024u;
    std::vector<uint32_t> order;
    std::vector<uint8_t> keys;
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int attempt = 0;; ++attempt) {
        if (cap >= 0x40000000ull) return fail(c, PHANT_E_OOM, "exec_witness_poststate: item list too long");
        uint32_t need = 0, undecided = 0;
        const int32_t rc = poststate_run(c, w, parent_state_root, io, order.empty() ? nullptr : order.data(), (uint32_t)cap, &need,
                                         &undecided, keys, cnt, sink);
        if (rc) return rc;
        const bool again_order = undecided != 0 && order.empty(), again_cap = need > cap && cnt[phant::PRE_CNT_FAILED] + cnt[phant::POST_CNT_EMIT_FAILED] == 0;
        // (the nodes outgrew their estimate: only a run that would otherwise have been the last is worth repeating for them)
        const bool again_sink = sink && sink->overflow != 0 && !again_order && !again_cap &&
                                cnt[phant::PRE_CNT_FAILED] + cnt[phant::POST_CNT_INTERNAL] + cnt[phant::POST_CNT_EMIT_FAILED] == 0;
        if ((!again_order && !again_cap && !again_sink) || attempt == (sink ? 3 : 2)) {
            if (again_order || again_cap || again_sink) return fail(c, PHANT_E_DEVICE, "exec_witness_poststate: the item list did not settle");
            break;
        }
        if (again_sink) {
            sink->cap_bytes = sink->need_bytes;
            sink->cap_desc = sink->need_desc;
        }
        if (again_order) {  // (duplicate keys or a long run of equal prefixes: ordered here, as the state root does)
            order.resize(nk);
            for (uint32_t k = 0; k < nk; ++k) order[k] = k;
            auto seg = [&](uint32_t k) { return k < na ? na : w.slot_account[k - na]; };
            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                if (seg(x) != seg(y)) return seg(x) < seg(y);
                const int m = std::memcmp(keys.data() + 32ull * x, keys.data() + 32ull * y, 32);
                return m != 0 ? m < 0 : x < y;
            });
        }
        if (need > cap) cap = need;
    }
    io->n_failed = cnt[phant::PRE_CNT_FAILED] + cnt[phant::POST_CNT_INTERNAL] + cnt[phant::POST_CNT_EMIT_FAILED];
    if (io->n_failed != 0) {
        if (io->state_root) std::memset(io->state_root, 0, 32);
        if (io->storage_roots) std::memset(io->storage_roots, 0, (size_t)na * 32);
    }
    return PHANT_OK;
}

int32_t phant_exec_witness_poststate(phant_ctx* c, const phant_exec_witness* pw, const uint8_t* parent_state_root, phant_poststate* io) {
    return poststate_call(c, pw, parent_state_root, io, nullptr);
}

/* ------------------------------------------------------- execution witness + writes -> the next block's witness */

// The post-state call with a sink behind node_ref (poststate.hip.h): the nodes come back in the order the lanes reserved their room,
// which no two runs share, so they are ordered here by what they ARE -- trie (the storage tries by account, then the state trie),
// the item that carries them in the call's sorted list (path order), deepest first, a child before the branch over it.
int32_t phant_exec_witness_advance(phant_ctx* c, const phant_exec_witness* pw, const uint8_t* parent_state_root, phant_poststate* io,
                                   uint32_t flags, phant_exec_witness** next) {
    if (!c || !pw || !io) return PHANT_E_INVALID_ARG;
    if (!next) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_advance: next is null");
    *next = nullptr;
    if (flags & ~PHANT_ADVANCE_KEEP_OLD) return fail(c, PHANT_E_INVALID_ARG, "exec_witness_advance: unknown flag");
    const phant::ExecWitness& w = pw->w;
    const uint64_t nk = (uint64_t)w.n_accounts + w.n_slots, total_nodes = w.node_off.size() - 1;
    AdvanceSink sink;
    // the nodes on the touched paths are about the ones the witness came with, plus a leaf per key and what the writes reshape
    sink.cap_bytes = c->advance_estimate ? c->advance_estimate : (uint64_t)w.nodes.size() + 256u * nk + 4096u;
    const uint64_t cap_desc = c->advance_estimate ? c->advance_estimate / 64u + 1u : total_nodes + 3u * nk + 64u;
    if (cap_desc >= 0x40000000ull) return fail(c, PHANT_E_OOM, "exec_witness_advance: too many nodes");
    sink.cap_desc = (uint32_t)cap_desc;
    const int32_t rc = poststate_call(c, pw, parent_state_root, io, &sink);
    if (rc) return rc;
    if (io->n_failed != 0) return PHANT_OK;
    std::unique_ptr<phant_exec_witness> out(new (std::nothrow) phant_exec_witness());
    if (!out) return fail(c, PHANT_E_OOM, "exec_witness_advance: out of host memory");
    phant::ExecWitness& x = out->w;
    x.codes = w.codes;
    x.code_off = w.code_off;
    x.preimages = w.preimages;
    x.preimage_off = w.preimage_off;
    x.slot_first = w.slot_first;
    x.slot_account = w.slot_account;
    x.n_accounts = w.n_accounts;
    x.n_slots = w.n_slots;
    x.node_off.push_back(0);
    if (w.n_accounts != 0) {  // (without accounts nothing ran)
        if (sink.overflow || sink.need_desc > sink.desc.size()) return fail(c, PHANT_E_DEVICE, "exec_witness_advance: the node list did not settle");
        std::vector<uint32_t> by(sink.need_desc);
        for (uint32_t i = 0; i < sink.need_desc; ++i) by[i] = i;
        const phant::PoststateNodeDesc* d = sink.desc.data();
        std::sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
            if (d[a].trie != d[b].trie) return d[a].trie < d[b].trie;
            if (d[a].item != d[b].item) return d[a].item < d[b].item;
            return d[a].where > d[b].where;
        });
        x.nodes.resize(sink.need_bytes);
        uint64_t at = 0;
        for (uint32_t i : by) {
            if (d[i].off + d[i].len > sink.blob.size() || at + d[i].len > sink.need_bytes)
                return fail(c, PHANT_E_DEVICE, "exec_witness_advance: a node descriptor out of range");
            std::memcpy(x.nodes.data() + at, sink.blob.data() + d[i].off, d[i].len);
            at += d[i].len;
            x.node_off.push_back(at);
        }
        x.nodes.resize(at);
    }
    if (flags & PHANT_ADVANCE_KEEP_OLD) {
        const uint64_t b0 = x.nodes.size();
        x.nodes.resize(b0 + w.nodes.size());
        if (!w.nodes.empty()) std::memcpy(x.nodes.data() + b0, w.nodes.data(), w.nodes.size());
        for (size_t i = 1; i < w.node_off.size(); ++i) x.node_off.push_back(b0 + w.node_off[i]);
    }
    *next = out.release();
    return PHANT_OK;
}

/* ------------------------------------------------- sharded trie roots (multi-GPU mptize) */

int32_t phant_mpt_root_nodes(phant_ctx* c, const uint8_t* keys, const uint32_t* key_off, const uint8_t* vals,
                             const uint64_t* val_off, uint32_t n, const uint32_t* seg_first, uint32_t n_tries,
                             uint8_t* roots, uint8_t* node_rlp, uint32_t node_cap, uint32_t* node_len) {
    if (!c || !roots || !seg_first || n_tries == 0 || !node_rlp || !node_len || node_cap == 0)
        return c ? fail(c, PHANT_E_INVALID_ARG, "mpt_root_nodes: bad argument") : PHANT_E_INVALID_ARG;
    if (n && (!key_off || !val_off)) return fail(c, PHANT_E_INVALID_ARG, "mpt_root_nodes: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    int32_t rc = phant::trie_forest_host(c->ws, c->stream, phant::HostPairs{keys, key_off, vals, val_off, n, seg_first, n_tries}, roots, err,
                                         phant::RootNodes{node_rlp, node_len, node_cap});
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_mpt_strip_first_nibble(const uint8_t* node, uint32_t len, uint8_t* out, uint32_t cap, uint32_t* out_len,
                                     uint32_t* is_ref) {
    return phant::strip_first_nibble(node, len, out, cap, out_len, is_ref);  // host-only (host_rlp.cpp)
}

/* ---------------------------------------------------------------- trie root */

int32_t phant_mpt_root(phant_ctx* c, const uint8_t* keys, const uint32_t* key_off,
                       const uint8_t* vals, const uint64_t* val_off, uint32_t n, uint8_t out[32]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    if (n && (!key_off || !val_off)) return fail(c, PHANT_E_INVALID_ARG, "mpt_root: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    int32_t rc = phant::trie_forest_host(c->ws, c->stream, phant::HostPairs{keys, key_off, vals, val_off, n}, out, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_mpt_root_dev(phant_ctx* c, const uint8_t* d_keys, const uint32_t* d_key_off, uint64_t key_bytes,
                           const uint8_t* d_vals, const uint64_t* d_val_off, uint64_t val_bytes, uint32_t n, uint8_t* d_root) {
    if (!c || !d_root || ((uintptr_t)d_root & 3u)) return PHANT_E_INVALID_ARG;
    if (n && (!d_key_off || !d_val_off || (key_bytes && !d_keys) || (val_bytes && !d_vals)))
        return fail(c, PHANT_E_INVALID_ARG, "mpt_root_dev: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    TimedRegion t(c);
    const int32_t rc = phant::trie_root_dev(c->ws, c->stream, phant::TriePairs{d_keys, d_key_off, key_bytes, d_vals, d_val_off, val_bytes, n, nullptr, 1, d_root}, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

/* ---------------------------------------------------------------- witness generation */

// The four entry points of the prover: two forms (the node set, a list per query), each over host and over device arrays.  Their out
// structs differ in the name of the first-node table alone (Out: either; first_node: that table), their refusals in the entry
// point's `name`.
static int32_t prove_refuse(phant_ctx* c, const char* name, const std::string& what) {
    return fail(c, PHANT_E_INVALID_ARG, (std::string(name) + ": " + what).c_str());
}

template <class Out>
static int32_t prove_check_host(phant_ctx* c, const char* name, const Out* out, const phant::HostPairs& h, const phant::ProveQueries& q) {
    if (!c || !out) return c ? prove_refuse(c, name, "out is null") : PHANT_E_INVALID_ARG;
    if (out->struct_size != sizeof(Out)) return prove_refuse(c, name, "wrong struct_size");
    if (h.n_tries == 0 || (!h.seg_first && h.n_tries != 1)) return prove_refuse(c, name, "seg_first is null, or no trie");
    if (h.n && (!h.key_off || !h.val_off)) return prove_refuse(c, name, "null pointer");
    if (q.n_queries && !q.qkey_off) return prove_refuse(c, name, "qkey_off is null");
    if (q.n_queries && !q.q_trie && h.n_tries != 1) return prove_refuse(c, name, "q_trie is null with several tries");
    return PHANT_OK;
}

template <class Out>
static int32_t prove_check_dev(phant_ctx* c, const char* name, const Out* out, uint32_t* Out::*first_node, const char* first_name,
                               const phant::TriePairs& p, const phant::ProveQueries& q, uint64_t qkey_bytes) {
    if (!c || !out) return c ? prove_refuse(c, name, "out is null") : PHANT_E_INVALID_ARG;
    if (out->struct_size != sizeof(Out)) return prove_refuse(c, name, "wrong struct_size");
    if (p.n_tries == 0 || (!p.seg_first && p.n_tries != 1)) return prove_refuse(c, name, "d_seg_first is null, or no trie");
    if (p.n && (!p.key_off || !p.val_off || (p.key_bytes && !p.keys) || (p.val_bytes && !p.vals))) return prove_refuse(c, name, "null pointer");
    if (q.n_queries && (!q.qkey_off || (qkey_bytes && !q.qkeys))) return prove_refuse(c, name, "null query pointer");
    if (q.n_queries && !q.q_trie && p.n_tries != 1) return prove_refuse(c, name, "d_q_trie is null with several tries");
    if (((uintptr_t)out->roots & 3u) || ((uintptr_t)out->node_off & 7u) || ((uintptr_t)(out->*first_node) & 3u))
        return prove_refuse(c, name, std::string("roots / ") + first_name + " 4-byte, node_off 8-byte aligned");
    return PHANT_OK;
}

// The call behind the checks: the out struct's buffers and capacities as the driver's arguments, `run(args, err)`, the totals back.
template <class Out, class Run>
static int32_t prove_run(phant_ctx* c, Out* out, uint32_t* Out::*first_node, bool per_proof, const phant::ProveQueries& q, Run&& run) {
    out->total_nodes = 0;
    out->nodes_len = 0;
    DeviceGuard g(c->device);
    std::string err;
    phant::ProveArgs a;
    a.q = q;
    a.per_proof = per_proof;
    a.nodes = out->nodes;
    a.node_off = out->node_off;
    a.first_node = out->*first_node;
    a.roots = out->roots;
    a.q_status = out->q_status;
    // (a buffer nobody wants has no capacity to exceed: the other one is then written under its own bound alone)
    a.nodes_cap = out->nodes ? out->nodes_cap : ~0ull;
    a.max_nodes = out->node_off ? out->max_nodes : 0xffffffffu;
    const int32_t rc = run(a, err);
    if (rc) return fail(c, rc, err.c_str());
    out->total_nodes = a.total_nodes;
    out->nodes_len = a.nodes_len;
    return PHANT_OK;
}

int32_t phant_mpt_prove_nodeset(phant_ctx* c, const uint8_t* keys, const uint32_t* key_off, const uint8_t* vals,
                                const uint64_t* val_off, uint32_t n, const uint32_t* seg_first, uint32_t n_tries,
                                const uint8_t* qkeys, const uint32_t* qkey_off, const uint32_t* q_trie, const uint8_t* q_flags,
                                uint32_t n_queries, phant_prove_out* out) {
    const phant::HostPairs h{keys, key_off, vals, val_off, n, seg_first, n_tries};
    const phant::ProveQueries q{qkeys, qkey_off, q_trie, q_flags, n_queries};
    if (const int32_t bad = prove_check_host(c, "mpt_prove_nodeset", out, h, q)) return bad;
    return prove_run(c, out, &phant_prove_out::trie_first_node, false, q,
                     [&](phant::ProveArgs& a, std::string& err) { return phant::prove_host(c->ws, c->stream, h, a, err); });
}

int32_t phant_mpt_prove_nodeset_dev(phant_ctx* c, const uint8_t* d_keys, const uint32_t* d_key_off, uint64_t key_bytes,
                                    const uint8_t* d_vals, const uint64_t* d_val_off, uint64_t val_bytes, uint32_t n,
                                    const uint32_t* d_seg_first, uint32_t n_tries, const uint8_t* d_qkeys, const uint32_t* d_qkey_off,
                                    uint64_t qkey_bytes, const uint32_t* d_q_trie, const uint8_t* d_q_flags, uint32_t n_queries,
                                    phant_prove_out* out) {
    const phant::TriePairs p{d_keys, d_key_off, key_bytes, d_vals, d_val_off, val_bytes, n, d_seg_first, n_tries};
    const phant::ProveQueries q{d_qkeys, d_qkey_off, d_q_trie, d_q_flags, n_queries};
    if (const int32_t bad = prove_check_dev(c, "mpt_prove_nodeset_dev", out, &phant_prove_out::trie_first_node, "trie_first_node", p, q, qkey_bytes))
        return bad;
    return prove_run(c, out, &phant_prove_out::trie_first_node, false, q, [&](phant::ProveArgs& a, std::string& err) {
        TimedRegion t(c);
        return phant::prove_dev(c->ws, c->stream, p, a, err);
    });
}

int32_t phant_mpt_prove_batch(phant_ctx* c, const uint8_t* keys, const uint32_t* key_off, const uint8_t* vals, const uint64_t* val_off,
                              uint32_t n, const uint32_t* seg_first, uint32_t n_tries, const uint8_t* qkeys, const uint32_t* qkey_off,
                              const uint32_t* q_trie, uint32_t n_queries, phant_prove_batch_out* out) {
    const phant::HostPairs h{keys, key_off, vals, val_off, n, seg_first, n_tries};
    const phant::ProveQueries q{qkeys, qkey_off, q_trie, nullptr, n_queries};
    if (const int32_t bad = prove_check_host(c, "mpt_prove_batch", out, h, q)) return bad;
    return prove_run(c, out, &phant_prove_batch_out::proof_first_node, true, q,
                     [&](phant::ProveArgs& a, std::string& err) { return phant::prove_host(c->ws, c->stream, h, a, err); });
}

int32_t phant_mpt_prove_batch_dev(phant_ctx* c, const uint8_t* d_keys, const uint32_t* d_key_off, uint64_t key_bytes, const uint8_t* d_vals,
                                  const uint64_t* d_val_off, uint64_t val_bytes, uint32_t n, const uint32_t* d_seg_first, uint32_t n_tries,
                                  const uint8_t* d_qkeys, const uint32_t* d_qkey_off, uint64_t qkey_bytes, const uint32_t* d_q_trie,
                                  uint32_t n_queries, phant_prove_batch_out* out) {
    const phant::TriePairs p{d_keys, d_key_off, key_bytes, d_vals, d_val_off, val_bytes, n, d_seg_first, n_tries};
    const phant::ProveQueries q{d_qkeys, d_qkey_off, d_q_trie, nullptr, n_queries};
    if (const int32_t bad = prove_check_dev(c, "mpt_prove_batch_dev", out, &phant_prove_batch_out::proof_first_node, "proof_first_node", p, q, qkey_bytes))
        return bad;
    return prove_run(c, out, &phant_prove_batch_out::proof_first_node, true, q, [&](phant::ProveArgs& a, std::string& err) {
        TimedRegion t(c);
        return phant::prove_dev(c->ws, c->stream, p, a, err);
    });
}

int32_t phant_index_root_rlp(phant_ctx* c, const uint8_t* items, const uint64_t* item_off,
                             uint32_t n, uint8_t out[32]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    if (n && (!items || !item_off)) return fail(c, PHANT_E_INVALID_ARG, "index_root_rlp: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    int32_t rc = phant::index_root_host(c->ws, c->stream, items, item_off, n, /*be32=*/false, out, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_block_roots(phant_ctx* c, const uint8_t* const* items, const uint64_t* const* item_off, const uint32_t* n,
                          uint32_t n_lists, uint8_t* roots_out, const uint8_t* bloom_items, const uint64_t* bloom_item_off,
                          const uint32_t* bloom_item_receipt, uint32_t n_bloom_items, uint32_t n_receipts, uint8_t* blooms) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (n_lists && (!items || !item_off || !n || !roots_out)) return fail(c, PHANT_E_INVALID_ARG, "block_roots: null pointer");
    for (uint32_t l = 0; l < n_lists; ++l)
        if (n[l] && (!items[l] || !item_off[l])) return fail(c, PHANT_E_INVALID_ARG, "block_roots: null list");
    DeviceGuard g(c->device);
    if (n_lists) {
        std::string err;
        const int32_t rc = phant::index_roots_host(c->ws, c->stream, items, item_off, n, n_lists, roots_out, err);
        if (rc) return fail(c, rc, err.c_str());
    }
    if (bloom_items || n_bloom_items) {
        if (!blooms) return fail(c, PHANT_E_INVALID_ARG, "block_roots: blooms is null");
        return phant_impl::phant_logs_bloom(c, bloom_items, bloom_item_off, bloom_item_receipt, n_bloom_items, n_receipts, blooms);
    }
    return PHANT_OK;
}

int32_t phant_index_root_be32(phant_ctx* c, const uint8_t* items, const uint64_t* item_off,
                              uint32_t n, uint8_t out[32]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    if (n && (!items || !item_off)) return fail(c, PHANT_E_INVALID_ARG, "index_root_be32: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    int32_t rc = phant::index_root_host(c->ws, c->stream, items, item_off, n, /*be32=*/true, out, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_state_root(phant_ctx* c, const uint8_t* addrs, const uint64_t* nonces,
                         const uint8_t* balances, const uint8_t* code, const uint64_t* code_off,
                         const uint8_t* slot_keys, const uint8_t* slot_vals,
                         const uint32_t* slot_first, uint32_t n, uint8_t out[32]) {
    if (!c || !out) return PHANT_E_INVALID_ARG;
    if (n && (!addrs || !nonces || !balances || !code_off || !slot_first))
        return fail(c, PHANT_E_INVALID_ARG, "state_root: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    int32_t rc = phant::state_root_host(c->ws, c->stream, phant::StateIn{addrs, nonces, balances, code, code_off, slot_keys, slot_vals, slot_first, n}, out, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_state_witness(phant_ctx* c, const uint8_t* addrs, const uint64_t* nonces, const uint8_t* balances, const uint8_t* code,
                            const uint64_t* code_off, const uint8_t* slot_keys, const uint8_t* slot_vals, const uint32_t* slot_first,
                            uint32_t n, const uint8_t* wkeys, const uint32_t* wkey_off, const uint8_t* wkey_flags, uint32_t n_wkeys,
                            phant_exec_witness** out, uint8_t state_root_out[32]) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (out) *out = nullptr;
    if (!out || !state_root_out) return fail(c, PHANT_E_INVALID_ARG, "state_witness: out / state_root_out is null");
    if (n && (!addrs || !nonces || !balances || !code_off || !slot_first)) return fail(c, PHANT_E_INVALID_ARG, "state_witness: null pointer");
    if (n_wkeys && (!wkeys || !wkey_off)) return fail(c, PHANT_E_INVALID_ARG, "state_witness: wkeys / wkey_off is null");
    std::unique_ptr<phant_exec_witness> w(new (std::nothrow) phant_exec_witness());
    if (!w) return fail(c, PHANT_E_OOM, "state_witness: out of host memory");
    DeviceGuard g(c->device);
    std::string err;
    const int32_t rc = phant::state_witness_host(c->ws, c->stream, phant::StateIn{addrs, nonces, balances, code, code_off, slot_keys, slot_vals, slot_first, n},
                                                 phant::ProveQueries{wkeys, wkey_off, nullptr, wkey_flags, n_wkeys}, w->w, state_root_out, err);
    if (rc) return fail(c, rc, err.c_str());
    *out = w.release();
    return PHANT_OK;
}

int32_t phant_state_proofs(phant_ctx* c, const uint8_t* addrs, const uint64_t* nonces, const uint8_t* balances, const uint8_t* code,
                           const uint64_t* code_off, const uint8_t* slot_keys, const uint8_t* slot_vals, const uint32_t* slot_first, uint32_t n,
                           const uint8_t* wkeys, const uint32_t* wkey_off, uint32_t n_wkeys, phant_witness** out, uint8_t state_root_out[32]) {
    if (!c) return PHANT_E_INVALID_ARG;
    if (out) *out = nullptr;
    if (!out || !state_root_out) return fail(c, PHANT_E_INVALID_ARG, "state_proofs: out / state_root_out is null");
    if (n && (!addrs || !nonces || !balances || !code_off || !slot_first)) return fail(c, PHANT_E_INVALID_ARG, "state_proofs: null pointer");
    if (n_wkeys && (!wkeys || !wkey_off)) return fail(c, PHANT_E_INVALID_ARG, "state_proofs: wkeys / wkey_off is null");
    std::unique_ptr<phant_witness> w(new (std::nothrow) phant_witness());
    if (!w) return fail(c, PHANT_E_OOM, "state_proofs: out of host memory");
    DeviceGuard g(c->device);
    std::string err;
    const int32_t rc = phant::state_proofs_host(c->ws, c->stream, phant::StateIn{addrs, nonces, balances, code, code_off, slot_keys, slot_vals, slot_first, n},
                                                phant::ProveQueries{wkeys, wkey_off, nullptr, nullptr, n_wkeys}, w->w, state_root_out, err);
    if (rc) return fail(c, rc, err.c_str());
    *out = w.release();
    return PHANT_OK;
}

int32_t phant_state_root_dev(phant_ctx* c, const uint8_t* d_addrs, const uint64_t* d_nonces, const uint8_t* d_balances,
                             const uint8_t* d_code, const uint64_t* d_code_off, uint64_t code_bytes, const uint8_t* d_slot_keys,
                             const uint8_t* d_slot_vals, const uint32_t* d_slot_first, uint32_t n_slots, uint32_t n, uint8_t* d_root) {
    if (!c || !d_root) return PHANT_E_INVALID_ARG;
    if (n && (!d_addrs || !d_nonces || !d_balances || !d_code_off || !d_slot_first || (code_bytes && !d_code) ||
              (n_slots && (!d_slot_keys || !d_slot_vals))))
        return fail(c, PHANT_E_INVALID_ARG, "state_root_dev: null pointer");
    if (((uintptr_t)d_slot_vals & 3u) || ((uintptr_t)d_balances & 3u) || ((uintptr_t)d_root & 3u))
        return fail(c, PHANT_E_INVALID_ARG, "state_root_dev: d_slot_vals / d_balances / d_root must be 4-byte aligned");
    DeviceGuard g(c->device);
    TimedRegion t(c);
    std::string err;
    const phant::StateIn in{d_addrs, d_nonces, d_balances, d_code, d_code_off, d_slot_keys, d_slot_vals, d_slot_first, n, n_slots, code_bytes};
    const int32_t rc = phant::state_root_dev(c->ws, c->stream, in, d_root, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_state_subtrie_nodes(phant_ctx* c, const uint8_t* addrs, const uint64_t* nonces, const uint8_t* balances,
                                  const uint8_t* code, const uint64_t* code_off, const uint8_t* slot_keys, const uint8_t* slot_vals,
                                  const uint32_t* slot_first, uint32_t n, uint8_t* roots, uint8_t* root_enc, uint32_t root_enc_cap,
                                  uint32_t* root_enc_len) {
    if (!c || !roots || !root_enc || !root_enc_len) return PHANT_E_INVALID_ARG;
    if (n && (!addrs || !nonces || !balances || !code_off || !slot_first))
        return fail(c, PHANT_E_INVALID_ARG, "state_subtrie_nodes: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    const phant::StateIn in{addrs, nonces, balances, code, code_off, slot_keys, slot_vals, slot_first, n};
    const int32_t rc = phant::state_subtrie_nodes_host(c->ws, c->stream, in, roots, phant::RootNodes{root_enc, root_enc_len, root_enc_cap}, err);
    if (rc) return fail(c, rc, err.c_str());
    return PHANT_OK;
}

int32_t phant_state_trie_leaves(phant_ctx* c, const uint8_t* addrs, const uint64_t* nonces, const uint8_t* balances,
                                const uint8_t* code, const uint64_t* code_off, const uint8_t* slot_keys,
                                const uint8_t* slot_vals, const uint32_t* slot_first, uint32_t n, uint8_t* keys,
                                uint8_t* vals, uint64_t vals_cap, uint64_t* val_off) {
    if (!c || !val_off) return PHANT_E_INVALID_ARG;
    if (n && (!addrs || !nonces || !balances || !code_off || !slot_first || !keys || !vals))
        return fail(c, PHANT_E_INVALID_ARG, "state_trie_leaves: null pointer");
    DeviceGuard g(c->device);
    std::string err;
    std::vector<uint8_t> k, v;
    std::vector<uint64_t> vo;
    int32_t rc = phant::state_leaves_host(c->ws, c->stream, phant::StateIn{addrs, nonces, balances, code, code_off, slot_keys, slot_vals, slot_first, n}, k, v, vo,
                                          err);
    if (rc) return fail(c, rc, err.c_str());
    if (v.size() > vals_cap) return fail(c, PHANT_E_INVALID_ARG, "state_trie_leaves: vals_cap too small (112 bytes per account suffice)");
    if (n) {
        std::memcpy(keys, k.data(), k.size());
        std::memcpy(vals, v.data(), v.size());
    }
    std::memcpy(val_off, vo.data(), vo.size() * 8);
    return PHANT_OK;
}

}  // namespace phant_impl

#include "capi_guard_capi.inc"
