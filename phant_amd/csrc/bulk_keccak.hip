// bulk_keccak.hip -- the other bulk users of keccak256 next to the trie path:
// same sponge-per-lane kernel as keccak_batch.hip, different packing of what goes in and what comes out.
//
//   logs bloom      src/types/receipt.zig:37-63  one lane per bloom item (a log's address or topic): hash it,
//                   take the three 11-bit indices addToBloom takes, OR the bits into the receipt's 2048-bit
//                   bloom with 32-bit atomics (blooms are zeroed by the launcher)
//   sender address  src/signer/signer.zig:77-78  one lane per 64-byte public key: the last 20 digest bytes
//
// Transaction hashes (src/types/transaction.zig:183-187,223-228,256-261: keccak256 of the EIP-2718 bytes) and
//   sender recovery  src/signer/signer.zig:40-79 / src/crypto/ecdsa.zig:19-21  one lane per signature: the public key
//                   (secp256k1.hip.h), hashed while it is in registers
//   receipts        src/types/receipt.zig:13-63 + src/blockchain/blockchain.zig:76-90  blooms, encodings, the block's bloom and
//                   the receipts root of a block in one call (receipts.hip.h)
//   block headers   src/types/block.zig:51-69 + src/blockchain/blockchain.zig:100-145  encodings, hashes and validateBlockHeader of
//                   whole chain segments in one call (headers.hip.h)
//   transactions    src/types/transaction.zig:152-273 + src/blockchain/blockchain.zig:237-260,345-381  decode, both hashes, senders,
//                   intrinsic gas and the state-free rules of a block's transactions in one call (transactions.hip.h, behind
//                   ecrecover_kernel below, which it launches)
//   block bodies    the transactions of a whole chain segment through those steps in one call, the rules under each block's own
//                   parameters, and the blocks' transactions and withdrawals tries as one forest (bodies.hip.h)
//   receipt segments  the receipts of a whole chain segment from raw consensus or eth/69 messages: strict decode, blooms, the consensus
//                   encodings, per-block verdicts and the blocks' receipts tries as one forest (receipt_segments.hip.h)
//   requests        the deposit requests of a chain segment rebuilt from its receipts' logs (EIP-6110) and every block's requests_hash
//                   (EIP-7685), the one user of SHA-256 (requests.hip.h, sha256.hip.h)
//   log filters     which logs of a chain segment each of many filters selects, exactly over the decoded rows and as a screen over
//                   2048-bit blooms (filters.hip.h)
//   fee history     per block of a chain segment the priority fee at chosen percentiles of its gas used, from the bodies' price rows
//                   and the receipts' gas rows (fee_history.hip.h)
// code hashes (src/blockchain/vm.zig:284-298; keccak256("") for an account without code is exactly its
// `empty_hash`) need no kernel of their own: they are phant_keccak256_batch over the respective byte strings.
#include "absorb.hip.h"
#include "launch.h"
#include "secp256k1.hip.h"
#include "receipts.hip.h"
#include "headers.hip.h"

namespace phant {

__global__ void __launch_bounds__(256)
logs_bloom_kernel(const uint8_t* __restrict__ items, const uint64_t* __restrict__ item_off,
                  const uint32_t* __restrict__ item_receipt, uint32_t n_items, uint32_t n_receipts,
                  uint32_t* __restrict__ blooms /* n_receipts x 64 dwords, zeroed */) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_items) return;
    const uint32_t r = item_receipt[k];
    if (r >= n_receipts) return;  // (ignored, as in the oracle)
    const uint64_t b = item_off[k], e = item_off[k + 1];
    Sponge s;
    keccak256_global(s, items + b, e >= b ? e - b : 0, items + item_off[n_items]);
    bloom_add_digest(s, blooms + 64ull * r);  // (receipts.hip.h)
}

__global__ void __launch_bounds__(256)
sender_address_kernel(const uint8_t* __restrict__ pubkeys, uint64_t stride, uint32_t n,
                      uint32_t* __restrict__ out /* n x 5 dwords */) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    Sponge s;
    keccak256_global(s, pubkeys + stride * i, 64, pubkeys + stride * (n - 1u) + 64);
    uint32_t* o = out + 5ull * i;  // digest bytes 12..31
    o[0] = s.hi[1];
    o[1] = s.lo[2];
    o[2] = s.hi[2];
    o[3] = s.lo[3];
    o[4] = s.hi[3];
}

// ---- secp256k1 (secp256k1.hip.h) ----
// entry j of the table = j G, affine, as 16 little-endian limbs; one lane per entry, once per context
__global__ void __launch_bounds__(64)
secp_gtable_kernel(uint32_t* __restrict__ gtable) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= secp::GTABLE_ENTRIES) return;
    uint32_t* e = gtable + 16u * j;
    if (j == 0) {
        for (int i = 0; i < 16; ++i) e[i] = 0u;
        return;
    }
    const secp::Jac g = secp::jac_from_affine(secp::const_gx(), secp::const_gy());
    secp::Jac acc = secp::jac_infinity();
    for (int bit = 7; bit >= 0; --bit) {
        acc = secp::jac_double(acc);
        if ((j >> bit) & 1u) acc = secp::jac_add(acc, g, true);
    }
    secp::U256 x, y;
    secp::jac_to_affine(acc, x, y);
    for (int i = 0; i < 8; ++i) e[i] = x.v[i], e[8 + i] = y.v[i];
}

// One lane per signature.  pre_status (may be null): a non-zero byte is the lane's verdict already (phant_tx_senders: a
// transaction the host could not decode).  A lane that fails leaves zeroed outputs.  Rows are read and written byte by byte: no
// alignment is asked of any array.
__global__ void __launch_bounds__(64)
ecrecover_kernel(const uint8_t* __restrict__ hashes, const uint8_t* __restrict__ r, const uint8_t* __restrict__ s,
                 const uint8_t* __restrict__ recid, const uint8_t* __restrict__ pre_status, uint32_t n, uint32_t flags,
                 const uint32_t* __restrict__ gtable, uint8_t* __restrict__ pubkeys, uint8_t* __restrict__ addresses,
                 uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    uint8_t st = pre_status ? pre_status[i] : secp::SIG_OK;
    secp::U256 qx = secp::u256_zero(), qy = secp::u256_zero();
    if (st == secp::SIG_OK) {
        st = secp::recover(secp::load_be32(hashes + 32ull * i), secp::load_be32(r + 32ull * i), secp::load_be32(s + 32ull * i),
                           recid[i], flags, gtable, qx, qy);
        if (st != secp::SIG_OK) qx = secp::u256_zero(), qy = secp::u256_zero();
    }
    if (status) status[i] = st;
    if (pubkeys) {
        secp::store_be32(pubkeys + 64ull * i, qx);
        secp::store_be32(pubkeys + 64ull * i + 32, qy);
    }
    if (addresses) {
        uint8_t* a = addresses + 20ull * i;
        if (st != secp::SIG_OK) {
            for (int k = 0; k < 20; ++k) a[k] = 0;
        } else {
            Sponge sp;
            secp::pubkey_digest(sp, qx, qy);
            const uint32_t w[5] = {sp.hi[1], sp.lo[2], sp.hi[2], sp.lo[3], sp.hi[3]};  // digest bytes 12..31
            for (int k = 0; k < 20; ++k) a[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// phant_diag_secp_op (include/phant_gpu_diag.h): one primitive per lane.  A point row is x || y || flag (65 bytes); the point
// operations lift their affine inputs to Jacobian coordinates with Z = 3 (and Z = 2 for the second operand of the general
// addition), so that the formulas see the denominators they see in the ladder.
PHANT_DEV secp::Jac diag_point(const uint8_t* __restrict__ row, uint32_t z) {
    if (row[64]) return secp::jac_infinity();
    const secp::U256 zz = secp::u256_small(z * z), zzz = secp::u256_small(z * z * z);
    secp::Jac p;
    p.x = secp::fe_mul(secp::load_be32(row), zz);
    p.y = secp::fe_mul(secp::load_be32(row + 32), zzz);
    p.z = secp::u256_small(z);
    return p;
}

__global__ void __launch_bounds__(64)
secp_op_kernel(uint32_t op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    if (op <= 5u) {
        const secp::U256 x = secp::load_be32(a + 32ull * i);
        const secp::U256 y = (op == 0u || op == 4u) ? secp::load_be32(b + 32ull * i) : x;
        secp::U256 res;
        if (op == 0u) res = secp::fe_mul(x, y);
        else if (op == 1u) res = secp::fe_sqr(x);
        else if (op == 2u) res = secp::fe_inv(x);
        else if (op == 3u) {
            const bool sq = secp::fe_sqrt(res, x);
            out[33ull * i + 32] = sq ? 1 : 0;
            secp::store_be32(out + 33ull * i, res);
            return;
        } else if (op == 4u) res = secp::sc_mul(x, y);
        else res = secp::sc_inv(x);
        secp::store_be32(out + 32ull * i, res);
        return;
    }
    const secp::Jac p = diag_point(a + 65ull * i, 3u);
    secp::Jac q;
    if (op == 6u) q = secp::jac_double(p);
    else if (op == 7u) q = secp::jac_add(p, diag_point(b + 65ull * i, 2u), false);
    else q = b[65ull * i + 64] ? p : secp::jac_add(p, diag_point(b + 65ull * i, 1u), true);  // (the mixed form takes no infinity)
    uint8_t* o = out + 65ull * i;
    secp::U256 x = secp::u256_zero(), y = secp::u256_zero();
    const bool inf = secp::jac_is_infinity(q);
    if (!inf) secp::jac_to_affine(q, x, y);
    secp::store_be32(o, x);
    secp::store_be32(o + 32, y);
    o[64] = inf ? 1 : 0;
}

// ---- a witness in its "index" form (witness.h): the proof nodes' hex digits still sit in the JSON text ----
// One wave per node: byte k of node i = the two hex digits at json[node_src[i] + 2k].  Anything that is not a
// hex digit sets err[0] and lowers err[1] to the first such node (both zero / 0xffffffff initialised by the
// launcher); the decoded bytes of such a node are unspecified and the caller rejects the witness.
PHANT_DEV uint32_t hex_nibble(uint32_t c, uint32_t& bad) {
    const uint32_t digit = c - '0', alpha = (c | 0x20u) - 'a';
    bad |= (digit > 9u && alpha > 5u) ? 1u : 0u;
    return digit <= 9u ? digit : alpha + 10u;
}

__global__ void __launch_bounds__(256)
hex_decode_kernel(const uint8_t* __restrict__ json, const uint64_t* __restrict__ node_src,
                  const uint64_t* __restrict__ node_off, uint32_t total_nodes, uint8_t* __restrict__ nodes,
                  uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= total_nodes) return;
    const uint64_t b = node_off[i], e = node_off[i + 1];
    const uint8_t* src = json + node_src[i];
    uint32_t bad = 0;
    for (uint64_t k = lane; k < e - b; k += 64u) {
        const uint32_t hi = hex_nibble(src[2u * k], bad), lo = hex_nibble(src[2u * k + 1u], bad);
        nodes[b + k] = (uint8_t)((hi << 4) | lo);
    }
    if (bad) {
        atomicOr(&err[0], 1u);
        atomicMin(&err[1], i);
    }
}

// the proven values (leaf payloads) of a batch, compacted for the host's consistency check: value i (at most
// `cap` bytes of it) at out + i * cap
__global__ void __launch_bounds__(256)
gather_values_kernel(const uint8_t* __restrict__ nodes, const uint64_t* __restrict__ value_off,
                     const uint32_t* __restrict__ value_len, uint32_t n, uint32_t cap, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = value_len[i] < cap ? value_len[i] : cap;
    const uint8_t* v = nodes + value_off[i];
    for (uint32_t k = 0; k < len; ++k) out[(uint64_t)i * cap + k] = v[k];
}

hipError_t launch_hex_decode(const uint8_t* d_json, const uint64_t* d_node_src, const uint64_t* d_node_off,
                             uint32_t total_nodes, uint8_t* d_nodes, uint32_t* d_err, hipStream_t st) {
    static const uint32_t init[2] = {0u, 0xffffffffu};
    hipError_t e = hipMemcpyAsync(d_err, init, 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess || total_nodes == 0) return e;
    hipLaunchKernelGGL(hex_decode_kernel, dim3((total_nodes + 3u) / 4u), dim3(256), 0, st, d_json, d_node_src, d_node_off,
                       total_nodes, d_nodes, d_err);
    return hipGetLastError();
}

hipError_t launch_gather_values(const uint8_t* d_nodes, const uint64_t* d_value_off, const uint32_t* d_value_len,
                                uint32_t n, uint32_t cap, uint8_t* d_out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_values_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_nodes, d_value_off, d_value_len,
                       n, cap, d_out);
    return hipGetLastError();
}

hipError_t launch_logs_bloom(const uint8_t* d_items, const uint64_t* d_item_off, const uint32_t* d_item_receipt,
                             uint32_t n_items, uint32_t n_receipts, uint8_t* d_blooms, hipStream_t st) {
    if (n_receipts == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_blooms, 0, 256ull * n_receipts, st);
    if (e != hipSuccess || n_items == 0) return e;
    hipLaunchKernelGGL(logs_bloom_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, st, d_items, d_item_off,
                       d_item_receipt, n_items, n_receipts, reinterpret_cast<uint32_t*>(d_blooms));
    return hipGetLastError();
}

hipError_t launch_sender_addresses(const uint8_t* d_pubkeys, uint64_t stride, uint32_t n, uint8_t* d_out,
                                   hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sender_address_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_pubkeys, stride, n,
                       reinterpret_cast<uint32_t*>(d_out));
    return hipGetLastError();
}

hipError_t launch_secp_gtable(uint32_t* d_gtable, hipStream_t st) {
    hipLaunchKernelGGL(secp_gtable_kernel, dim3(secp::GTABLE_ENTRIES / 64u), dim3(64), 0, st, d_gtable);
    return hipGetLastError();
}

hipError_t launch_ecrecover(const uint8_t* d_hashes, const uint8_t* d_r, const uint8_t* d_s, const uint8_t* d_recid,
                            const uint8_t* d_pre_status, uint32_t n, uint32_t flags, const uint32_t* d_gtable,
                            uint8_t* d_pubkeys, uint8_t* d_addresses, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ecrecover_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, d_hashes, d_r, d_s, d_recid, d_pre_status, n,
                       flags, d_gtable, d_pubkeys, d_addresses, d_status);
    return hipGetLastError();
}

hipError_t launch_secp_op(uint32_t op, const uint8_t* d_a, const uint8_t* d_b, uint32_t n, uint8_t* d_out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(secp_op_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, op, d_a, d_b, n, d_out);
    return hipGetLastError();
}

}  // namespace phant

#include "transactions.hip.h"
#include "bodies.hip.h"
#include "receipt_segments.hip.h"
#include "requests.hip.h"
#include "filters.hip.h"
#include "fee_history.hip.h"
#include "txstate.hip.h"
#include "settle.hip.h"
#include "access_lists.hip.h"
