// requests_check.h -- what phant_block_requests[_dev] refuses before anything is copied, launched or written (include/phant_gpu.h: the
// paragraph on PHANT_E_INVALID_ARG): the structs, the NULL inputs, the counts without their parents, the device form's alignment, and -- in
// the host form -- the firsts and offsets themselves.  Plain host C++, nothing of HIP: capi.hip and requests.hip.h call it, and
// tests/native/requests_check_main.cpp runs it as a stand-alone program under AddressSanitizer + UBSan over arrays of exactly their sizes.
#pragma once
#include "segment_checks.h"

namespace phant {
namespace qreq {

// the structs and pointers, both forms: "" or what is wrong
inline const char* check_args(const phant_requests_in* in, const phant_requests_out* out, bool dev) {
    if (!in || !out) return "in / out is null";
    if (in->struct_size != sizeof(phant_requests_in) || out->struct_size != sizeof(phant_requests_out)) return "wrong struct_size";
    if (in->reserved != 0u || out->reserved != 0u) return "reserved is not 0";
    if (in->n_blocks == 0u) return in->n || in->n_logs || in->n_topics || in->n_req ? "rows without a block" : "";
    if (!in->block_first) return "null block_first";
    if (in->n ? !in->log_first : in->n_logs != 0u) return in->n ? "null log_first" : "logs without a receipt";
    if (in->n_logs ? !in->address || !in->topic_first || !in->data_at || !in->data_len : in->n_topics != 0u)
        return in->n_logs ? "null address / topic_first / data_at / data_len" : "topics without a log";
    if (in->n_topics && !in->topics) return "null topics";
    if (in->rc_bytes && !in->receipts) return "null receipts";
    if (in->n_req && (!in->req_block_first || !in->req_type || !in->req_off)) return "null req_block_first / req_type / req_off";
    if (dev && in->n_req && in->req_total && !in->req_bytes) return "null req_bytes";
    if (dev) {  // (kernels read the firsts and offsets as words; the outputs arrive by copies of bytes)
        const uintptr_t w8 = (uintptr_t)in->data_at | (uintptr_t)in->req_off;
        const uintptr_t w4 = (uintptr_t)in->block_first | (uintptr_t)in->log_first | (uintptr_t)in->topic_first | (uintptr_t)in->data_len |
                             (uintptr_t)in->req_block_first | (uintptr_t)out->deposit_log | (uintptr_t)out->deposit_first | (uintptr_t)out->block_flags;
        if ((w8 & 7u) || (w4 & 3u)) return "misaligned array";
    }
    return "";
}

// the host form's firsts and offsets (check_args has passed, n_blocks != 0): PHANT_OK, or the code with the reason in err
inline int32_t check_host(const phant_requests_in& in, std::string& err) {
    const char* const call = "block_requests";
    if (const int32_t rc = seg::check_firsts_host(call, "block_first", "n", in.block_first, in.n_blocks, in.n, err)) return rc;
    if (in.n)
        if (const int32_t rc = seg::check_firsts_host(call, "log_first", "n_logs", in.log_first, in.n, in.n_logs, err)) return rc;
    if (in.n_logs)
        if (const int32_t rc = seg::check_firsts_host(call, "topic_first", "n_topics", in.topic_first, in.n_logs, in.n_topics, err)) return rc;
    if (!in.n_req) return PHANT_OK;
    if (const int32_t rc = seg::check_firsts_host(call, "req_block_first", "n_req", in.req_block_first, in.n_blocks, in.n_req, err)) return rc;
    if (const int32_t rc = seg::check_offsets_host(call, "req_off", "request", in.req_off, in.n_req, err)) return rc;
    if (in.req_off[in.n_req] && !in.req_bytes) return err = std::string(call) + ": null req_bytes", PHANT_E_INVALID_ARG;
    return PHANT_OK;
}

}  // namespace qreq
}  // namespace phant
