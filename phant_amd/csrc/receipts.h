// receipts.h -- a block's receipts on the device (internal; kernels and host side in receipts.hip.h, the public surface is
// phant_block_receipts / phant_block_receipts_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// One block's receipts as struct-of-arrays, the lists that ride along and where the answers go.  Host form: every pointer is
// host memory.  Device form: every array is device memory; `lists` / `list_off` / `list_n` / `list_bytes` themselves are host
// arrays (of device pointers and counts).  Any output may be null.
struct ReceiptsArgs {
    const uint8_t* tx_type = nullptr;      // n
    const uint8_t* status = nullptr;       // n
    const uint64_t* cum_gas = nullptr;     // n
    const uint32_t* log_first = nullptr;   // n + 1: 0 .. n_logs
    const uint8_t* address = nullptr;      // n_logs x 20
    const uint32_t* topic_first = nullptr; // n_logs + 1: 0 .. n_topics
    const uint64_t* data_off = nullptr;    // n_logs + 1: 0 .. data_bytes
    const uint8_t* topics = nullptr;       // n_topics x 32
    const uint8_t* data = nullptr;
    uint32_t n = 0, n_logs = 0, n_topics = 0;
    uint64_t data_bytes = 0;
    const uint8_t* const* lists = nullptr;
    const uint64_t* const* list_off = nullptr;
    const uint32_t* list_n = nullptr;
    const uint64_t* list_bytes = nullptr;  // device form: what list_off[l][list_n[l]] must be
    uint32_t n_lists = 0, receipts_at = 0;
    uint8_t* receipts_root = nullptr;      // 32
    uint8_t* logs_bloom = nullptr;         // 256: the block's
    uint8_t* blooms = nullptr;             // n x 256
    uint8_t* encoded = nullptr;            // the receipts back to back in index order, encoded_cap bytes of room
    uint64_t* encoded_off = nullptr;       // encoded_off_cap entries of room, n + 1 are written
    uint8_t* roots_out = nullptr;          // (n_lists + 1) x 32
    uint64_t encoded_cap = 0;
    uint32_t encoded_off_cap = 0;
    uint64_t encoded_len = 0;              // out: always written
};

int32_t block_receipts(Workspaces& ws, hipStream_t st, ReceiptsArgs& a, bool device_form, std::string& err);

// The receipts of a chain segment from raw messages (receipt_segments.hip.h; phant_block_receipt_segments[_dev]): in / out as they came,
// every array host memory in the host form and device memory in the device form; the scalars of `out` are written on PHANT_OK.
int32_t block_receipt_segments(Workspaces& ws, hipStream_t st, const phant_rcpt_segs_in& in, phant_rcpt_segs_out& out, bool device_form, std::string& err);

// The execution requests of a chain segment (requests.hip.h; phant_block_requests[_dev]): the deposits rebuilt from the log rows of
// block_receipt_segments, every block's requests_hash; in / out as they came, checked by requests_check.h's check_args.
int32_t block_requests(Workspaces& ws, hipStream_t st, const phant_requests_in& in, phant_requests_out& out, bool device_form, std::string& err);

}  // namespace phant
