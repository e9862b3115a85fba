// feehist_check.h -- what phant_block_fee_history[_dev] refuses before anything is copied, launched or written (include/phant_gpu.h: the
// paragraph on PHANT_E_INVALID_ARG): the structs, the NULL inputs, the device form's alignment, the percentiles (host memory in both forms)
// and -- in the host form -- block_first and the cap on a block's rows; and the one test of the selection that the device and the host
// share (reaches).  Plain host C++, nothing of HIP: capi.hip and fee_history.hip.h call it, and tests/native/feehist_check_main.cpp runs
// it as a stand-alone program under AddressSanitizer + UBSan over arrays of exactly their sizes.
#pragma once
#include "segment_checks.h"
#include "wide_uint.h"

namespace phant {
namespace fh {

// S >= floor(G p / 10000) without a division: 10000 (S + 1) > G p, in 128 bits (S, G: 96 bits in three limbs; p <= 10000)
PHANT_WIDE_FN bool reaches(const uint32_t* S, const uint32_t* G, uint32_t p) {
    uint32_t lhs[4] = {S[0], S[1], S[2], 0u}, rhs[4] = {G[0], G[1], G[2], 0u};
    const uint32_t one[4] = {1u, 0u, 0u, 0u};
    wide::add<4>(lhs, one);
    wide::mul_small<4>(lhs, 10000u);
    wide::mul_small<4>(rhs, p);
    return wide::less<4>(rhs, lhs);
}

// the structs and pointers, both forms: "" or what is wrong
inline const char* check_args(const phant_fee_history_in* in, const phant_fee_history_out* out, bool dev) {
    if (!in || !out) return "in / out is null";
    if (in->struct_size != sizeof(phant_fee_history_in) || out->struct_size != sizeof(phant_fee_history_out)) return "wrong struct_size";
    if (in->reserved != 0u || out->reserved != 0u) return "reserved is not 0";
    if (in->n_percentiles && !in->percentile) return "null percentile";
    if (in->n_blocks == 0u) return in->n ? "rows without a block" : "";
    if (!in->block_first) return "null block_first";
    if (in->n && (!in->price || !in->gas_used)) return "null price / gas_used";
    if (dev) {  // (kernels read and write them as words; the host form's arrive by copies of bytes)
        if (((uintptr_t)in->block_first | (uintptr_t)out->order | (uintptr_t)out->block_flags) & 3u) return "misaligned array";
        if (((uintptr_t)in->gas_used | (uintptr_t)out->block_gas_used) & 7u) return "misaligned array";
    }
    return "";
}

// the percentiles (check_args has passed): basis points
inline const char* check_percentiles(const phant_fee_history_in& in) {
    for (uint32_t k = 0; k < in.n_percentiles; ++k)
        if (in.percentile[k] > 10000u) return "a percentile above 10000 basis points";
    return "";
}

// a reward per (block, percentile) in one call: below 2^31 of them
inline bool too_many_rewards(uint32_t n_blocks, uint32_t n_percentiles) { return (uint64_t)n_blocks * n_percentiles >= 0x80000000ull; }

// the cap a ctx's PHANT_DIAG_FEEHIST_BLOCK_MAX leaves: 0 or anything beyond the product's value is the product's value
inline uint32_t block_max_of(int64_t diag) { return diag > 0 && diag < (int64_t)PHANT_FEEHIST_BLOCK_MAX ? (uint32_t)diag : PHANT_FEEHIST_BLOCK_MAX; }

// the host form's block_first (check_args has passed, n_blocks != 0): from 0 to n, never backwards, no block above the cap
inline int32_t check_rows_host(const char* call, const phant_fee_history_in& in, uint32_t block_max, std::string& err) {
    if (const int32_t rc = seg::check_firsts_host(call, "block_first", "n", in.block_first, in.n_blocks, in.n, err)) return rc;
    for (uint32_t b = 0; b < in.n_blocks; ++b)
        if (in.block_first[b + 1u] - in.block_first[b] > block_max) return err = std::string(call) + ": a block of more than " + std::to_string(block_max) + " rows", PHANT_E_UNSUPPORTED;
    return PHANT_OK;
}

}  // namespace fh
}  // namespace phant
