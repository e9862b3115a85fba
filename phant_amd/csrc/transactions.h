// transactions.h -- a block's transactions on the device (internal; kernels and host side in transactions.hip.h, the public surface
// is phant_block_transactions[_ex] / phant_block_transactions[_ex]_dev in include/phant_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/phant_gpu.h"
#include "arena.h"

namespace phant {

// in: the caller's struct as it came (host pointers in the host form, device pointers in the device form; base_fee is host memory in
// both); out: where the answers go, first_bad always written on PHANT_OK.  gtable: the context's multiples of G, or null when the
// call does not recover.  The caller has checked struct sizes, flag bits, the fork, NULL arguments and alignment.  phant_block_transactions
// is this with fork = PHANT_TXS_FORK_LONDON and none of the new outputs.  On PHANT_OK out.base.first_bad, out.n_auth and
// out.blob_gas_used are written.
int32_t block_transactions(Workspaces& ws, hipStream_t st, const phant_txs_ex_in& in, phant_txs_ex_out& out, bool device_form,
                           const uint32_t* gtable, std::string& err);

// The bodies of a chain segment (bodies.hip.h; phant_block_bodies[_dev]): in / out as they came, every array host memory in the host form
// and device memory in the device form.  The caller has checked struct sizes, flag bits, the fork, NULL arguments and alignment, and
// n_blocks != 0.  On PHANT_OK out.first_bad_block and the scalars of out.txs are written.
int32_t block_bodies(Workspaces& ws, hipStream_t st, const phant_bodies_in& in, phant_bodies_out& out, bool device_form, const uint32_t* gtable,
                     std::string& err);

}  // namespace phant
