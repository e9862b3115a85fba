// headers.h -- block headers on the device (internal; kernels and host side in headers.hip.h, the public surface is
// phant_header_chain / phant_header_chain_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form); out: where the
// answers go, first_bad and enc_len always written on PHANT_OK.  The caller has checked struct sizes and alignment.
int32_t header_chain(Workspaces& ws, hipStream_t st, const phant_headers_in& in, phant_headers_out& out, bool device_form, std::string& err);

}  // namespace phant
