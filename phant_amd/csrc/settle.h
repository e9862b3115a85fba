// settle.h -- a block of plain transfers settled on the device (internal; kernels and host side in settle.hip.h, the public surface is
// phant_block_settle / phant_block_settle_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form); out: where the answers go.
// The caller has checked struct sizes, the fork, reserved, NULL arguments, the counts, coinbase_row and alignment.  On PHANT_OK the
// scalars of `out` are written.
int32_t block_settle(Workspaces& ws, hipStream_t st, const phant_settle_in& in, phant_settle_out& out, bool device_form, std::string& err);

}  // namespace phant
