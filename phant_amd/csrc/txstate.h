// txstate.h -- a block's transactions against the pre-state (internal; kernels and host side in txstate.hip.h, the public surface is
// phant_block_txs_prestate / phant_block_txs_prestate_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form); out: where the answers go.
// salt: the key of the address table's slot function (per ctx).  The caller has checked struct sizes, the fork, reserved, NULL
// arguments and alignment.  On PHANT_OK out.first_bad and out.n_undetermined are written.
int32_t block_txs_prestate(Workspaces& ws, hipStream_t st, const phant_txstate_in& in, phant_txstate_out& out, bool device_form,
                           const uint32_t salt[2], std::string& err);

}  // namespace phant
