// filters_check.h -- what phant_block_log_filters[_dev] and phant_log_filters_bloom[_dev] refuse before anything is copied, launched or
// written (include/phant_gpu.h: the paragraph on PHANT_E_INVALID_ARG): the structs, the NULL inputs, the counts without their parents,
// the device form's alignment, and -- in the host form -- the firsts of the rows and of the filters and the filters' ranges.  Plain host
// C++, nothing of HIP: capi.hip and filters.hip.h call it, and tests/native/filters_check_main.cpp runs it as a stand-alone program under
// AddressSanitizer + UBSan over arrays of exactly their sizes.
#pragma once
#include "segment_checks.h"

namespace phant {
namespace lf {

// the filters' struct and pointers, both calls and both forms: "" or what is wrong
inline const char* check_filter_args(const phant_log_filters* f, bool dev) {
    if (!f) return "filters is null";
    if (f->struct_size != sizeof(phant_log_filters)) return "wrong struct_size of the filters";
    if (f->reserved != 0u) return "the filters' reserved is not 0";
    if (f->n_filters == 0u) return f->n_addr || f->n_topic ? "entries without a filter" : "";
    if (f->n_filters > 0x3fffffffu) return "more than 2^30 - 1 filters";
    if (!f->addr_first || !f->topic_first) return "null addr_first / topic_first of the filters";
    if ((f->n_addr && !f->addr) || (f->n_topic && !f->topic)) return "null addr / topic";
    if (dev && (((uintptr_t)f->addr_first | (uintptr_t)f->topic_first | (uintptr_t)f->block_lo | (uintptr_t)f->block_hi) & 3u)) return "misaligned array of the filters";
    return "";
}

// phant_block_log_filters: the structs and pointers, both forms
inline const char* check_match_args(const phant_logmatch_in* in, const phant_log_filters* f, const phant_logmatch_out* out, bool dev) {
    if (!in || !out) return "in / out is null";
    if (in->struct_size != sizeof(phant_logmatch_in) || out->struct_size != sizeof(phant_logmatch_out)) return "wrong struct_size";
    if (in->reserved != 0u || in->reserved2 != 0u || out->reserved != 0u || out->reserved2 != 0u) return "reserved is not 0";
    if (const char* const what = check_filter_args(f, dev); *what) return what;
    if (in->n_blocks == 0u) return in->n || in->n_logs || in->n_topics ? "rows without a block" : "";
    if (!in->block_first) return "null block_first";
    if (in->n ? !in->log_first : in->n_logs != 0u) return in->n ? "null log_first" : "logs without a receipt";
    if (in->n_logs ? !in->address || !in->topic_first : in->n_topics != 0u) return in->n_logs ? "null address / topic_first" : "topics without a log";
    if (in->n_topics && !in->topics) return "null topics";
    if (dev) {  // (kernels read the firsts as words; the outputs arrive by copies of bytes)
        const uintptr_t w4 = (uintptr_t)in->block_first | (uintptr_t)in->log_first | (uintptr_t)in->topic_first | (uintptr_t)out->filter_first |
                             (uintptr_t)out->match_log | (uintptr_t)out->filter_count;
        if (w4 & 3u) return "misaligned array";
    }
    return "";
}

// phant_log_filters_bloom: the pointers, both forms
inline const char* check_bloom_args(const uint8_t* blooms, uint32_t n_blooms, const phant_log_filters* f, const uint64_t* may, const uint32_t* may_count, bool dev) {
    if (const char* const what = check_filter_args(f, dev); *what) return what;
    if (n_blooms && !blooms) return "null blooms";
    if (dev && (((uintptr_t)may & 7u) || ((uintptr_t)may_count & 3u))) return "misaligned array";
    return "";
}

// the host form's filters (check_filter_args has passed, n_filters != 0): their firsts, and every range inside [0, n_blocks]
inline int32_t check_filters_host(const char* call, const phant_log_filters& f, uint32_t n_blocks, std::string& err) {
    if (const int32_t rc = seg::check_firsts_host(call, "the filters' addr_first", "n_addr", f.addr_first, f.n_filters, f.n_addr, err)) return rc;
    if (const int32_t rc = seg::check_firsts_host(call, "the filters' topic_first", "n_topic", f.topic_first, 4u * f.n_filters, f.n_topic, err)) return rc;
    for (uint32_t i = 0; i < f.n_filters; ++i) {
        const uint32_t lo = f.block_lo ? f.block_lo[i] : 0u, hi = f.block_hi ? f.block_hi[i] : n_blocks;
        if (lo > hi) return err = std::string(call) + ": a filter's block_lo is above its block_hi", PHANT_E_INVALID_ARG;
        if (hi > n_blocks) return err = std::string(call) + ": a filter's block_hi is above the number of blocks", PHANT_E_INVALID_ARG;
    }
    return PHANT_OK;
}

// the host form's rows (check_match_args has passed, n_blocks != 0)
inline int32_t check_rows_host(const char* call, const phant_logmatch_in& in, std::string& err) {
    if (const int32_t rc = seg::check_firsts_host(call, "block_first", "n", in.block_first, in.n_blocks, in.n, err)) return rc;
    if (in.n)
        if (const int32_t rc = seg::check_firsts_host(call, "log_first", "n_logs", in.log_first, in.n, in.n_logs, err)) return rc;
    if (in.n_logs)
        if (const int32_t rc = seg::check_firsts_host(call, "topic_first", "n_topics", in.topic_first, in.n_logs, in.n_topics, err)) return rc;
    return PHANT_OK;
}

// n_filters x ceil(items / 64) words and ballots in one call: below 2^31
inline bool too_many_words(uint32_t n_filters, uint32_t items) { return (uint64_t)n_filters * (((uint64_t)items + 63u) / 64u) >= 0x80000000ull; }

// the entries of the sets that go through the table (host form: the filters' firsts are host memory and checked)
inline uint64_t large_entries_host(const phant_log_filters& f, uint32_t linear_max) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < f.n_filters; ++i)
        if (f.addr_first[i + 1u] - f.addr_first[i] > linear_max) total += f.addr_first[i + 1u] - f.addr_first[i];
    for (uint32_t i = 0; i < 4u * f.n_filters; ++i)
        if (f.topic_first[i + 1u] - f.topic_first[i] > linear_max) total += f.topic_first[i + 1u] - f.topic_first[i];
    return total;
}

}  // namespace lf
}  // namespace phant
