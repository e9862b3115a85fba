// access_lists.h -- a block's access lists against the pre-state tables (internal; kernels and host side in access_lists.hip.h, the
// public surface is phant_block_access_lists / phant_block_access_lists_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form), n != 0; out: where the
// answers go.  salt: the key of the tables' slot functions (per ctx).  The caller has checked struct sizes, reserved, NULL arguments,
// the counts' bounds and alignment.  On PHANT_OK the five results of `out` are written.
int32_t block_access_lists(Workspaces& ws, hipStream_t st, const phant_access_in& in, phant_access_out& out, bool device_form,
                           const uint32_t salt[2], std::string& err);

}  // namespace phant
