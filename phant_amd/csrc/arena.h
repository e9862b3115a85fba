// arena.h -- grow-only device arenas owned by a phant_ctx, so that host-form
// calls do not pay hipMalloc/hipFree (which synchronise the device) per call.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <phant_platform.h>  // PHANT_ARENA_POISON / _UNPOISON: nothing in the library's own build

namespace phant {

struct DevArena {
    uint8_t* base = nullptr;
    size_t cap = 0, used = 0;
    bool overflowed = false;  // a take() beyond what reset() made room for (answered with nullptr)

    static size_t round(size_t n) { return (n + 255) / 256 * 256; }

    // Make room for `total` bytes and start allocating from the beginning.
    // Contents are dropped; the caller guarantees no kernel still uses them.
    hipError_t reset(size_t total) {
        used = 0;
        overflowed = false;
        if (base) PHANT_ARENA_UNPOISON(base, cap);
        if (total <= cap) return hipSuccess;
        if (base) {
            hipError_t e = hipFree(base);  // implies a device synchronise
            base = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        const size_t want = total + total / 4 + (1u << 20);
        hipError_t e = hipMalloc((void**)&base, want);
        if (e != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
    // nullptr when the arena was not reset for this much (a sizing bug upstream: the caller turns it into PHANT_E_DEVICE
    // instead of handing a kernel memory behind the allocation)
    template <class T>
    T* take(size_t count) {
        const size_t bytes = count * sizeof(T), dwords = (bytes + 3) / 4 * 4;  // (device loads are dword-granular)
        if (!base || round(bytes) > cap - used) {
            overflowed = true;
            return nullptr;
        }
        T* p = reinterpret_cast<T*>(base + used);
        PHANT_ARENA_POISON(base + used + dwords, round(bytes) - dwords);
        used += round(bytes);
        return p;
    }
    void release() {
        if (base) PHANT_ARENA_UNPOISON(base, cap);
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = used = 0;
    }
};

// Stands in for a DevArena to count what a list of take<T>() calls needs: the size to reset() the arena to before the same
// list runs against it.
struct ArenaSizer {
    size_t bytes = 0;
    template <class T>
    T* take(size_t count) {
        bytes += DevArena::round(count * sizeof(T));
        return nullptr;
    }
};

// Switches of the trie hasher and of the state root's key sort (per ctx; set through include/phant_gpu_diag.h's phant_diag_set by
// tests and tools, never read from the environment).  -1 / 0 / false = the library's own choice (trie_plan.h: the constants, resolve_choices).
struct TrieTune {
    bool no_side = false;            // never run the deepest bins on the helper stream beside the leaves (A/B)
    int64_t side_min_keys = -1;      // ... from this many keys on (tests)
    int64_t ahead_max_keys = -1;     // the leaves are queued ahead of the host's sizing up to this many keys (tests)
    int64_t side_lds = -1;           // idle dynamic LDS of the bulk leaf kernel while bins run beside it
    int64_t fallback_grid = -1;      // workgroups of a bin's fallback pass (tests)
    int32_t slot_blocks = 0;         // != 0: every bin in slots of this many rate blocks (A/B)
    bool no_coop = false;            // never the node-per-half-wave / node-per-wave kernels for thin bins (A/B)
    int64_t coop_max = -1;           // ... up to this many nodes
    bool no_wave = false;            // the half-wave kernel for every thin bin (A/B)
    bool join_in_stream = false;     // the helper stream joined by an event in the main stream instead of by hand (A/B)
    bool sort_no_fallback = false;   // state root: an undecided device sort is an error instead of a host sort (tests)
    int64_t sort_prefix_bits = -1;   // state root: the device sort on this many key bits, ties left undecided (tests)
    int64_t sort_repair_bits = -1;   // ... ties repaired (tests)
    int64_t small_max_keys = -1;     // up to this many keys a call takes the two-launch pass (trie_build.hip: small_head_kernel; 0: never)
};

// What the trie hasher's last call on a ctx did (include/phant_gpu_diag.h: phant_trie_stats): host integers the launcher had in its
// hands anyway, written as it goes; nothing on the device is touched for them.  The misfit counters stay where the kernels count
// them (the t1 arena, at misfit_off), like the scratch blob's cursor, and are read when somebody asks.
struct TrieStats {
    uint32_t pass = 0;          // 0: no kernel pass (no call yet, no keys, or refused before one was chosen), 1: the small pass, 2: the general one
    uint32_t ahead = 0;         // the leaves were queued ahead of the host's sizing
    int32_t deep_from = -1;     // the depth from which the bins ran on the helper stream (-1: none did)
    uint32_t bins = 0;          // non-empty depth bins
    uint32_t max_bin = 0;       // nodes of the largest
    uint32_t by_class[5] = {};  // bins launched a wave per node, a node per half wave, a lane per node in 1- / 2- / 4-block slots
    uint32_t side_bins = 0;     // ... of all those, on the helper stream
    uint32_t leaf_big = 0;      // leaf_big_kernel ran
    uint32_t n_rep = 0;         // branch nodes (the general pass; the small pass does not count them)
    uint32_t n = 0;             // keys
    bool has_misfit = false, has_cursor = false;
    size_t misfit_off = 0;      // of the 512 per-depth misfit counters inside t1
    size_t cursor_off = 0;      // of the scratch blob's cursor (the bytes the nodes that did not fit an LDS slot took there) inside t1
};

// The arenas a ctx lends to the host-form entry points.
struct Workspaces {
    TrieTune tune;
    TrieStats trie_stats;
    DevArena io;  // staged inputs / outputs of the current call
    DevArena t1;  // trie builder: per-key / per-boundary arrays
    DevArena t2;  // trie builder: slot tables + encoding scratch
    DevArena pv;  // prover (trie_prove.hip.h): marks, sizes, offsets -- next to t1 / t2, which hold the build it reads
    DevArena pvo; // prover, host form: the node blob and its offsets on their way out (the per-proof form: the set the proofs are cut from)
    DevArena pvb; // prover, per-proof form: the set index of every output node; host form: the proofs on their way out
    DevArena txa; // block_transactions: the rows of the authorization tuples, sized in the middle of a call (whose other arrays stay in `io`)
    // Pinned mirror of the first STAGE_BYTES of `io` for SMALL host-form calls: the caller's pageable arrays are packed into
    // it at the offsets their device copies have in the arena and cross the bus in ONE copy (a pageable hipMemcpyAsync costs
    // ~25 us a piece, and a call has five to nine); it is mapped into the device's address space, so small results can be
    // written straight into it.  Only by calls that end with a stream synchronisation (the next call overwrites it).
    static constexpr size_t STAGE_BYTES = 8u << 20;
    uint8_t* stage = nullptr;
    hipError_t ensure_stage() {
        return stage ? hipSuccess : hipHostMalloc(reinterpret_cast<void**>(&stage), STAGE_BYTES, hipHostMallocDefault);
    }
    // A few pinned, device-visible words for what a pass reads back in the middle of a call (the trie builder's counters): a
    // copy into pageable memory costs ~25 us, a kernel that stores its flags here costs nothing beyond the synchronisation.
    // Coherent (fine-grained) whatever HIP_HOST_COHERENT says: the trie builder's host side reads what a kernel stored here
    // WHILE that kernel runs (order_kernel).
    static constexpr size_t MAILBOX_WORDS = 2048;
    // Who owns which words: the trie builder and its prover everything below MAILBOX_RECEIPTS (trie_prove.hip.h asserts that
    // they end in front of it), block_receipts the MAILBOX_RECEIPTS_WORDS behind it -- so the builder's passes, which rewrite
    // their own window on every call, never touch the control words a receipts call has read or is about to read.
    static constexpr size_t MAILBOX_RECEIPTS = 1536, MAILBOX_RECEIPTS_WORDS = 8;
    // ... and header_chain (headers.hip.h) the MAILBOX_HEADERS_WORDS behind those
    static constexpr size_t MAILBOX_HEADERS = MAILBOX_RECEIPTS + MAILBOX_RECEIPTS_WORDS, MAILBOX_HEADERS_WORDS = 8;
    // ... and block_transactions (transactions.hip.h) the MAILBOX_TXS_WORDS behind those
    static constexpr size_t MAILBOX_TXS = MAILBOX_HEADERS + MAILBOX_HEADERS_WORDS, MAILBOX_TXS_WORDS = 8;
    // ... and block_txs_prestate (txstate.hip.h) the MAILBOX_TXST_WORDS behind those
    static constexpr size_t MAILBOX_TXST = MAILBOX_TXS + MAILBOX_TXS_WORDS, MAILBOX_TXST_WORDS = 4;
    // ... and block_access_lists (access_lists.hip.h) the MAILBOX_AL_WORDS behind those
    static constexpr size_t MAILBOX_AL = MAILBOX_TXST + MAILBOX_TXST_WORDS, MAILBOX_AL_WORDS = 8;
    // ... and block_settle (settle.hip.h) the MAILBOX_SETTLE_WORDS behind those
    static constexpr size_t MAILBOX_SETTLE = MAILBOX_AL + MAILBOX_AL_WORDS, MAILBOX_SETTLE_WORDS = 8;
    // ... and phant_mpt_verify_ranges (capi.hip) the MAILBOX_RANGES_WORDS behind those
    static constexpr size_t MAILBOX_RANGES = MAILBOX_SETTLE + MAILBOX_SETTLE_WORDS, MAILBOX_RANGES_WORDS = 4;
    // ... and block_receipt_segments (receipt_segments.hip.h) the MAILBOX_RSEG_WORDS behind those
    static constexpr size_t MAILBOX_RSEG = MAILBOX_RANGES + MAILBOX_RANGES_WORDS, MAILBOX_RSEG_WORDS = 8;
    // ... and block_requests (requests.hip.h) the MAILBOX_QREQ_WORDS behind those
    static constexpr size_t MAILBOX_QREQ = MAILBOX_RSEG + MAILBOX_RSEG_WORDS, MAILBOX_QREQ_WORDS = 4;
    // ... and block_log_filters / log_filters_bloom (filters.hip.h) the MAILBOX_LF_WORDS behind those
    static constexpr size_t MAILBOX_LF = MAILBOX_QREQ + MAILBOX_QREQ_WORDS, MAILBOX_LF_WORDS = 4;
    // ... and block_fee_history (fee_history.hip.h) the MAILBOX_FH_WORDS behind those
    static constexpr size_t MAILBOX_FH = MAILBOX_LF + MAILBOX_LF_WORDS, MAILBOX_FH_WORDS = 4;
    static_assert(MAILBOX_FH + MAILBOX_FH_WORDS <= MAILBOX_WORDS, "the receipts', the headers' and the transactions' control words fit the pinned mailbox");
    uint32_t* mailbox = nullptr;
    hipError_t ensure_mailbox() {
        if (mailbox) return hipSuccess;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&mailbox), MAILBOX_WORDS * 4, hipHostMallocCoherent);
        if (e == hipSuccess)  // (the handshake words are compared with a tag counted up from what is found here: start from zero)
            for (size_t i = 0; i < MAILBOX_WORDS; ++i) mailbox[i] = 0u;
        return e;
    }
    // A call's control words into its part of the mailbox (`at`: one of the MAILBOX_* offsets above): one copy and a stream
    // synchronisation, behind which mailbox[at ..] holds them.
    hipError_t read_words(size_t at, const uint32_t* d_words, size_t words, hipStream_t st) {
        const hipError_t e = hipMemcpyAsync(mailbox + at, d_words, 4 * words, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
    // a helper stream + events for the trie builder's deepest bins, which run next to the bulk of the leaves
    hipStream_t side = nullptr;
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    hipError_t ensure_side() {
        if (side) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&side_fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&side_join, hipEventDisableTiming);
        return e;
    }
    // the small pass's persistent words (trie_build.hip: the call's flags, a count of workgroups), zeroed when allocated and by
    // every call's last workgroup.  small_dirty: a call left its kernels on a way other than that one (a failed launch, a stream in
    // error) -- the next small call zeroes the words itself before it launches.
    uint32_t* small_state = nullptr;
    bool small_dirty = false;
    hipError_t ensure_small(size_t bytes) {
        if (small_state) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&small_state), bytes);
        if (e != hipSuccess) return e;
        e = hipMemset(small_state, 0, bytes);
        if (e != hipSuccess) {  // (never words nobody has zeroed)
            (void)hipFree(small_state);
            small_state = nullptr;
        }
        return e;
    }
    hipError_t rezero_small(size_t bytes, hipStream_t st) {
        hipError_t e = hipStreamSynchronize(st);  // (whatever of the call that went wrong is still running writes them)
        if (e == hipSuccess) e = hipMemset(small_state, 0, bytes);
        if (e == hipSuccess) small_dirty = false;
        return e;
    }
    // the pinned twin of a device address inside `io`
    template <class T>
    T* staged(T* d) const {
        return reinterpret_cast<T*>(stage + (reinterpret_cast<const uint8_t*>(d) - io.base));
    }
    void release() {
        io.release();
        t1.release();
        t2.release();
        pv.release();
        pvo.release();
        pvb.release();
        txa.release();
        if (stage) (void)hipHostFree(stage);
        stage = nullptr;
        if (mailbox) (void)hipHostFree(mailbox);
        mailbox = nullptr;
        if (small_state) (void)hipFree(small_state);
        small_state = nullptr;
        if (side_fork) (void)hipEventDestroy(side_fork);
        if (side_join) (void)hipEventDestroy(side_join);
        if (side) (void)hipStreamDestroy(side);
        side = nullptr;
        side_fork = side_join = nullptr;
    }
};

}  // namespace phant
