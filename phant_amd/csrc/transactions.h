// transactions.h -- a block's transactions on the device (internal; kernels and host side in transactions.hip.h, the public surface
// is phant_block_transactions / phant_block_transactions_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form; base_fee is host memory in
// both); out: where the answers go, first_bad always written on PHANT_OK.  gtable: the context's multiples of G, or null when the
// call does not recover.  The caller has checked struct sizes, flag bits, NULL arguments and alignment.
int32_t block_transactions(Workspaces& ws, hipStream_t st, const phant_txs_in& in, phant_txs_out& out, bool device_form,
                           const uint32_t* gtable, std::string& err);

}  // namespace phant
