// transactions.hip.h -- a block's transactions end to end on the device (included by bulk_keccak.hip): the strict decode of
// src/types/transaction.zig:152-273, both hashes of every transaction (Tx.hash and the signing hash of src/signer/signer.zig:81-188),
// the sender (secp256k1.hip.h), src/blockchain/blockchain.zig:355-381 `calculateIntrinsicCost` and the state-free rules of
// `checkTransaction` / `validateTransaction` (:237-260, :345-353).  The raw bytes are read by kernels only, and no signing preimage is
// ever written anywhere: the signing sponge takes it from where it lies in the transaction.
//
//   tx_check_args_kernel  device form only: tx_off runs from 0 to tx_bytes, never backwards, no transaction of 4 GiB; a lane per
//                         entry, and the host reads the verdict before any other kernel indexes with the offsets
//   tx_decode_kernel      a lane per transaction: tx::decode (below; its access-list walk is serial in its lane), the field rows, r / s /
//                         recid for the recovery, and the PLAN of the signing preimage:
//                             prefix (type byte, new list header: <= 10 bytes)  ||  raw[body_begin, body_end)  ||  suffix (EIP-155: rlp(chain_id),
//                             0x80, 0x80: <= 11 bytes)
//   tx_hash_kernel        a lane per transaction, two runs of one sponge loop: the raw bytes (with the calldata's non-zero bytes counted
//                         on the dwords the sponge has loaded anyway), then the plan.  Block k of the signing sponge starts at raw offset
//                         body_begin + 136 k - prefix_len: its first and last blocks mix bytes from registers with bytes from memory
//   (ecrecover_kernel)    bulk_keccak.hip's, with PHANT_RECOVER_LOW_S; a transaction the decode refused arrives with its verdict in
//                         pre_status and never reaches the curve arithmetic
//   tx_rules_kernel       a lane per transaction: intrinsic gas, the fee rules, gas_limit x gas_price + value in 320 bits, flags, and the
//                         least flagged index by one atomic
// phant_block_transactions_ex adds the blob transaction of EIP-4844 and the set-code transaction of EIP-7702 to the
// decode, their rows and rules to the kernels above, and for the authorization tuples of a call, once the decode has counted them:
//   (exclusive scan)      radix_sort.hip's, over the tuples per transaction: auth_first
//   tx_auth_rows_kernel   a lane per transaction: its tuples' fields into the rows from auth_first[i] on
//   tx_auth_hash_kernel   a lane per tuple: keccak256(0x05 || rlp([chain_id, address, nonce])), one block built in registers
//   (ecrecover_kernel)    over the tuples' rows: the authorities
// phant_block_bodies (bodies.hip.h) runs the same kernels over the transactions of a whole chain segment: the rules
// are tx::rules_row for both rules kernels, and the host driver's steps are tx::call_begin / call_carve / call_kernels / call_outputs.
//
// Plain C++ plus the builtins the sponge uses: tests/emu.py compiles this file for the host.  With PHANT_TX_DECODE_ONLY defined only
// tx::decode and what it needs are declared, without any HIP header: tests/native/tx_decode_main.cpp builds it as a program of its own.
#pragma once
#include <stdint.h>

#include "rlp.h"

#ifdef PHANT_TX_DECODE_ONLY
#define TX_HD inline
#else
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/phant_gpu.h"
#include "absorb.hip.h"
#include "launch.h"
#include "secp256k1.hip.h"
#include "segment_lists.hip.h"
#include "staging.h"
#include "transactions.h"
#define TX_HD __host__ __device__ inline
#endif

namespace phant {
namespace tx {

// the decode's verdicts: PHANT_SIG_OK, PHANT_SIG_BAD_TX, PHANT_SIG_BAD_V; of an authorization tuple also PHANT_AUTH_CHAIN_ID and
// PHANT_AUTH_NONCE_MAX (include/phant_gpu.h)
enum : uint8_t { ST_OK = 0, ST_BAD_TX = 6, ST_BAD_V = 7, ST_AUTH_CHAIN_ID = 8, ST_AUTH_NONCE_MAX = 9 };
// which typed transactions a call decodes: PHANT_TXS_FORK_*
enum : uint32_t { FORK_LONDON = 0, FORK_CANCUN = 1, FORK_PRAGUE = 2 };

// a string item's payload inside the transaction
struct Span {
    uint32_t at, len;
};

// What one transaction decodes to.  Positions are relative to the transaction's first byte (a transaction is shorter than 4 GiB).
struct Decoded {
    uint8_t status;  // ST_*; with ST_BAD_TX nothing else is defined
    uint8_t type;    // 0 .. 4
    uint8_t recid;   // ST_OK only
    uint8_t eip155;  // legacy, v = 35 + 2 chain_id + {0, 1}
    uint8_t create;  // `to` is empty
    uint64_t chain_id_field, nonce, gas_limit;  // chain_id_field: typed transactions
    Span priority, gas_price, value, to, data, al, r, s;  // al: the access list's payload; priority = gas_price for types 0 and 1
    uint32_t al_addresses, al_keys;
    Span blob_fee, hashes, auths;  // type 3: max_fee_per_blob_gas, the versioned hashes' payload; type 4: the authorization list's payload
    uint32_t blobs, tuples;        // how many of each
    // the signing preimage = prefix || raw[body_begin, body_end) || suffix (ST_OK only)
    uint32_t body_begin, body_end;
    uint8_t prefix_len, suffix_len;
    uint8_t prefix[12], suffix[12];  // 10 and 11 bytes used
};

// One canonical RLP item (rlp.h's decoder) at p[pos ..) with everything up to `end` left: its payload [pay, pend), which ends the item.
TX_HD bool rlp_item(const uint8_t* p, uint32_t pos, uint32_t end, uint32_t& pay, uint32_t& pend, bool& is_list) {
    RlpItem it;
    if (pos >= end || !rlp_decode(MemBytes{p}, pos, end - pos, it)) return false;
    pay = it.pay, pend = it.pay + it.len, is_list = it.is_list != 0u;
    return true;
}

// a string of at most max_bytes bytes without a leading zero
TX_HD bool uint_ok(const uint8_t* p, uint32_t pay, uint32_t pend, bool is_list, uint32_t max_bytes) {
    return !is_list && pend - pay <= max_bytes && (pend == pay || p[pay] != 0u);
}
TX_HD uint64_t be_u64(const uint8_t* p, uint32_t pay, uint32_t pend) {
    uint64_t v = 0;
    for (uint32_t k = pay; k < pend; ++k) v = v << 8 | p[k];
    return v;
}

// [[address20, [key32, ...]], ...] inside [pay, pend), nothing else inside a tuple; serial in its lane
TX_HD bool access_list(const uint8_t* p, uint32_t pay, uint32_t pend, uint32_t& addresses, uint32_t& keys) {
    addresses = keys = 0;
    uint32_t pos = pay;
    while (pos < pend) {
        uint32_t tp, te, ip, ie;
        bool list;
        if (!rlp_item(p, pos, pend, tp, te, list) || !list) return false;  // the tuple
        if (!rlp_item(p, tp, te, ip, ie, list) || list || ie - ip != 20u) return false;  // the address
        uint32_t kp, ke;
        if (!rlp_item(p, ie, te, kp, ke, list) || !list || ke != te) return false;  // the keys, and nothing after
        ++addresses;
        while (kp < ke) {
            if (!rlp_item(p, kp, ke, ip, ie, list) || list || ie - ip != 32u) return false;
            ++keys;
            kp = ie;
        }
        pos = te;
    }
    return true;
}

// [hash32, ...] inside [pay, pend): every item is 0xa0 and 32 bytes
TX_HD bool hash_list(const uint8_t* p, uint32_t pay, uint32_t pend, uint32_t& hashes) {
    hashes = 0;
    for (uint32_t pos = pay; pos < pend; pos += 33u, ++hashes) {
        uint32_t ip, ie;
        bool list;
        if (!rlp_item(p, pos, pend, ip, ie, list) || list || ie - ip != 32u) return false;
    }
    return true;
}

// One authorization tuple of EIP-7702.
struct Auth {
    Span chain_id, address, nonce, y_parity, r, s;
};
// [chain_id <= 32, address 20, nonce <= 8, y_parity <= 1, r <= 32, s <= 32] at p[pos ..) with everything up to `end` left, canonical
// integers, nothing else inside -> where the tuple ends
TX_HD bool auth_tuple(const uint8_t* p, uint32_t pos, uint32_t end, Auth& a, uint32_t& next) {
    uint32_t tp, te, ip, ie;
    bool list;
    if (!rlp_item(p, pos, end, tp, te, list) || !list) return false;
    if (!rlp_item(p, tp, te, ip, ie, list) || !uint_ok(p, ip, ie, list, 32u)) return false;
    a.chain_id.at = ip, a.chain_id.len = ie - ip;
    if (!rlp_item(p, ie, te, ip, ie, list) || list || ie - ip != 20u) return false;
    a.address.at = ip, a.address.len = 20u;
    if (!rlp_item(p, ie, te, ip, ie, list) || !uint_ok(p, ip, ie, list, 8u)) return false;
    a.nonce.at = ip, a.nonce.len = ie - ip;
    if (!rlp_item(p, ie, te, ip, ie, list) || !uint_ok(p, ip, ie, list, 1u)) return false;
    a.y_parity.at = ip, a.y_parity.len = ie - ip;
    if (!rlp_item(p, ie, te, ip, ie, list) || !uint_ok(p, ip, ie, list, 32u)) return false;
    a.r.at = ip, a.r.len = ie - ip;
    if (!rlp_item(p, ie, te, ip, ie, list) || !uint_ok(p, ip, ie, list, 32u) || ie != te) return false;
    a.s.at = ip, a.s.len = ie - ip;
    next = te;
    return true;
}
// [tuple, ...] inside [pay, pend); serial in its lane
TX_HD bool auth_list(const uint8_t* p, uint32_t pay, uint32_t pend, uint32_t& tuples) {
    tuples = 0;
    for (uint32_t pos = pay; pos < pend; ++tuples) {
        Auth a;
        if (!auth_tuple(p, pos, pend, a, pos)) return false;
    }
    return true;
}

// The item kinds of a transaction in the order of a type-2 list; type 1 has no PRIORITY, type 0 neither CHAIN_ID nor ACCESS_LIST.
// Type 3 has BLOB_FEE and BLOB_HASHES, type 4 AUTH_LIST between the access list and the signature.
enum : uint32_t { K_CHAIN_ID, K_NONCE, K_PRIORITY, K_GAS_PRICE, K_GAS, K_TO, K_VALUE, K_DATA, K_ACCESS_LIST, K_V, K_R, K_S, K_END, K_BLOB_FEE,
                  K_BLOB_HASHES, K_AUTH_LIST };
TX_HD uint32_t kind_of(uint32_t type, uint32_t idx) {
    uint32_t k;
    if (type >= 2u) {
        const uint32_t extra = type == 3u ? 2u : type == 4u ? 1u : 0u;  // the items between the access list and v
        if (idx <= K_ACCESS_LIST) return idx;
        if (idx <= K_ACCESS_LIST + extra) return type == 4u ? (uint32_t)K_AUTH_LIST : idx == K_ACCESS_LIST + 1u ? (uint32_t)K_BLOB_FEE : (uint32_t)K_BLOB_HASHES;
        k = idx - extra;
    } else if (type == 1u) {
        k = idx < 2u ? idx : idx + 1u;
    } else {
        k = idx == 0u ? (uint32_t)K_NONCE : idx <= 5u ? idx + 2u : idx + 3u;
    }
    return k < K_END ? k : (uint32_t)K_END;
}

// Transaction p[0, len) -> d, with exactly the verdicts of host_rlp.cpp::tx_signing_parts (which phant_tx_senders decodes with):
// canonical RLP, the item count of the type, integers without leading zeros and within their widths, `to` empty or 20 bytes, a
// well-formed access list, nothing behind the list.  Every read stays inside p[0, len).  Types 3 (EIP-4844, from FORK_CANCUN) and 4
// (EIP-7702, from FORK_PRAGUE), which that decode does not know, with the same strictness: versioned hashes of exactly 32 bytes,
// authorization tuples as auth_tuple reads them; a type the fork does not enable is ST_BAD_TX.
TX_HD void decode(const uint8_t* p, uint32_t len, uint64_t chain_id, uint32_t fork, Decoded& d) {
    d.status = ST_BAD_TX;
    d.type = d.recid = d.eip155 = d.create = 0;
    d.chain_id_field = d.nonce = d.gas_limit = 0;
    d.al_addresses = d.al_keys = d.blobs = d.tuples = 0;
    d.body_begin = d.body_end = 0;
    d.prefix_len = d.suffix_len = 0;
    const Span none = {0u, 0u};
    d.priority = d.gas_price = d.value = d.to = d.data = d.al = d.r = d.s = d.blob_fee = d.hashes = d.auths = none;
    if (len == 0u) return;
    uint32_t start = 0;
    if (p[0] < 0x80u) {  // EIP-2718: a type byte in front of the list
        d.type = p[0];
        if (d.type == 0u || d.type > 2u + fork || d.type > 4u) return;
        start = 1u;
    }
    uint32_t pay, pend;
    bool is_list;
    if (!rlp_item(p, start, len, pay, pend, is_list) || !is_list || pend != len) return;
    Span v = none;
    uint32_t v_full = 0, idx = 0, pos = pay;
    while (pos < pend) {
        const uint32_t kind = kind_of(d.type, idx);
        uint32_t ip, ie;
        bool il;
        if (kind == K_END || !rlp_item(p, pos, pend, ip, ie, il)) return;
        const Span sp = {ip, ie - ip};
        switch (kind) {
        case K_CHAIN_ID:
            if (!uint_ok(p, ip, ie, il, 8u)) return;
            d.chain_id_field = be_u64(p, ip, ie);
            break;
        case K_NONCE:
            if (!uint_ok(p, ip, ie, il, 8u)) return;
            d.nonce = be_u64(p, ip, ie);
            break;
        case K_GAS:
            if (!uint_ok(p, ip, ie, il, 8u)) return;
            d.gas_limit = be_u64(p, ip, ie);
            break;
        case K_PRIORITY:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.priority = sp;
            break;
        case K_GAS_PRICE:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.gas_price = sp;
            break;
        case K_VALUE:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.value = sp;
            break;
        case K_TO:
            if (il || (sp.len != 0u && sp.len != 20u)) return;
            d.to = sp, d.create = sp.len == 0u;
            break;
        case K_DATA:
            if (il) return;
            d.data = sp;
            break;
        case K_ACCESS_LIST:
            if (!il || !access_list(p, ip, ie, d.al_addresses, d.al_keys)) return;
            d.al = sp;
            break;
        case K_BLOB_FEE:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.blob_fee = sp;
            break;
        case K_BLOB_HASHES:
            if (!il || !hash_list(p, ip, ie, d.blobs)) return;
            d.hashes = sp;
            break;
        case K_AUTH_LIST:
            if (!il || !auth_list(p, ip, ie, d.tuples)) return;
            d.auths = sp;
            break;
        case K_V:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            v = sp, v_full = pos;
            break;
        case K_R:
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.r = sp;
            break;
        default:  // K_S
            if (!uint_ok(p, ip, ie, il, 32u)) return;
            d.s = sp;
            break;
        }
        pos = ie, ++idx;
    }
    if (kind_of(d.type, idx) != K_END) return;  // too few items
    if (d.type < 2u) d.priority = d.gas_price;
    // v: a value of more than 9 bytes matches nothing below (35 + 2 chain_id + 1 < 2^66); 72 bits as (hi, lo)
    d.status = ST_BAD_V;
    if (v.len > 9u) return;
    const uint32_t v_hi = v.len == 9u ? p[v.at] : 0u;
    const uint64_t v_lo = be_u64(p, v.len == 9u ? v.at + 1u : v.at, v.at + v.len);
    if (d.type == 0u) {
        const uint64_t twice = chain_id << 1, b_lo = twice + 35u;
        const uint32_t b_hi = (uint32_t)(chain_id >> 63) + (b_lo < twice ? 1u : 0u);
        const uint64_t c_lo = b_lo + 1u;
        const uint32_t c_hi = b_hi + (c_lo == 0u ? 1u : 0u);
        if (v_hi == 0u && (v_lo == 27u || v_lo == 28u)) d.recid = (uint8_t)(v_lo - 27u);
        else if (v_hi == b_hi && v_lo == b_lo) d.recid = 0, d.eip155 = 1;
        else if (v_hi == c_hi && v_lo == c_lo) d.recid = 1, d.eip155 = 1;
        else return;
    } else {
        if (v_hi != 0u || v_lo > 1u) return;
        d.recid = (uint8_t)v_lo;
    }
    d.status = ST_OK;
    // the signed list: the items in front of v, verbatim, (chain_id, 0, 0 for EIP-155,) under a header of their own
    d.body_begin = pay, d.body_end = v_full;
    if (d.eip155) {
        uint32_t t = put_uint(d.suffix, chain_id);
        d.suffix[t++] = 0x80u, d.suffix[t++] = 0x80u;
        d.suffix_len = (uint8_t)t;
    }
    uint32_t h = 0;
    if (d.type) d.prefix[h++] = d.type;
    h += put_hdr(d.prefix + h, 0xc0u, (uint64_t)(d.body_end - d.body_begin) + d.suffix_len);
    d.prefix_len = (uint8_t)h;
}
// types 0 - 2 only: what phant_block_transactions decodes
TX_HD void decode(const uint8_t* p, uint32_t len, uint64_t chain_id, Decoded& d) { decode(p, len, chain_id, FORK_LONDON, d); }

}  // namespace tx
}  // namespace phant

#ifndef PHANT_TX_DECODE_ONLY
namespace phant {
namespace tx {

using In = phant_txs_in;
using Out = phant_txs_out;

// the call's control words (32-bit, device memory, zeroed): [0] = seg::F_*, [1] = n - (the least flagged index) or 0, [2] = the authorization
// tuples of the call, [4 .. 5] = its versioned hashes as one 64-bit counter
constexpr size_t CTL_WORDS = 8;
constexpr uint32_t ERROR_BITS = PHANT_TX_ERROR_BITS_EX;  // (a call without types 3 and 4 never sets a bit above PHANT_TX_IS_CREATE)
constexpr uint64_t GAS_PER_BLOB = 131072u, AUTH_COST = 25000u, FLOOR_PER_TOKEN = 10u;

// the call's outputs in the order they lie in the arena, the ones most callers want first (the host form fetches one span that ends
// behind the last wanted one): X(member, element type, elements per transaction)
#define TX_OUTPUTS(X)                                                                                                              \
    X(flags, uint32_t, 1) X(tx_hash, uint8_t, 32) X(sender, uint8_t, 20) X(sig_status, uint8_t, 1) X(sig_hash, uint8_t, 32)           \
    X(intrinsic_gas, uint64_t, 1) X(effective_gas_price, uint8_t, 32) X(upfront_cost, uint8_t, 32) X(type, uint8_t, 1)                 \
    X(nonce, uint64_t, 1) X(gas_limit, uint64_t, 1) X(chain_id, uint64_t, 1) X(gas_price, uint8_t, 32) X(priority_fee, uint8_t, 32)    \
    X(value, uint8_t, 32) X(to, uint8_t, 20) X(data_off, uint64_t, 1) X(data_len, uint32_t, 1) X(al_off, uint64_t, 1)                  \
    X(al_len, uint32_t, 1) X(al_addresses, uint32_t, 1) X(al_keys, uint32_t, 1) X(sig, uint8_t, 65)
// ... of phant_txs_ex_out, behind those: a row per transaction (auth_first has one more) ...
#define TX_EX_OUTPUTS(X) X(floor_gas, uint64_t, 1) X(blobs, uint32_t, 1) X(blob_off, uint64_t, 1) X(max_fee_per_blob_gas, uint8_t, 32)
// ... and a row per authorization tuple, in an arena of their own that is sized once the tuples are counted
#define TX_AUTH_OUTPUTS(X)                                                                                                              \
    X(auth_status, uint8_t, 1) X(authority, uint8_t, 20) X(auth_hash, uint8_t, 32) X(auth_chain_id, uint8_t, 32) X(auth_address, uint8_t, 20) \
    X(auth_nonce, uint64_t, 1) X(auth_sig, uint8_t, 65)

// what tx_decode_kernel leaves for tx_hash_kernel: 48 bytes a transaction, read as three 16-byte loads
struct __attribute__((aligned(16))) Plan {
    uint32_t body_begin, body_end, lens;  // lens = prefix_len | suffix_len << 8 | (the decode's verdict) << 16
    uint32_t data_at, data_len;           // the calldata inside the transaction (0, 0 when it did not decode)
    uint32_t prefix[3], suffix[3];
    uint32_t pad;
};
static_assert(sizeof(Plan) == 48, "three 16-byte loads");

// the device arrays of a call (Out's members point into the arena), r / s / recid / the decode's verdicts for ecrecover_kernel
struct Dev {
    Out o;
    phant_txs_ex_out x;  // (its per-transaction arrays; base and the per-authorization ones are not used)
    Plan* plan;
    uint8_t *r, *s, *recid, *pre_status;
    uint32_t *auth_at, *auth_len;  // the authorization list's payload inside its transaction
    uint32_t* ctl;
};
// the per-authorization device arrays: the caller's rows, r / s / y_parity / the tuple's own verdict for ecrecover_kernel
struct AuthDev {
    phant_txs_ex_out x;
    uint8_t *r, *s, *recid, *pre_status;
};
struct Rules {
    uint32_t base_fee[8], blob_base_fee[8];  // little-endian limbs
    uint32_t have_base_fee, have_gas_limit, have_blob_base_fee, fork;
    uint64_t block_gas_limit;
};

// Device form only: what a caller can lie about, a lane per entry, before any kernel indexes with it.
__global__ void __launch_bounds__(256) tx_check_args_kernel(const uint64_t* __restrict__ tx_off, uint32_t n, uint64_t tx_bytes, uint32_t* __restrict__ ctl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = seg::off_flags(tx_off, i, n, tx_bytes);
    if (f) atomicOr(ctl, f);
}

TX_HD void put_be32(uint8_t* row, const uint8_t* p, Span sp) {
    for (uint32_t k = 0; k < 32u; ++k) row[k] = k < 32u - sp.len ? (uint8_t)0 : p[sp.at + k - (32u - sp.len)];
}
TX_HD uint32_t pack4(const uint8_t* b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }

__global__ void __launch_bounds__(64) tx_decode_kernel(const uint8_t* __restrict__ txs, const uint64_t* __restrict__ tx_off, uint32_t n,
                                                        uint64_t chain_id, uint32_t fork, Dev dv) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = tx_off[i];
    const uint32_t len = (uint32_t)(tx_off[i + 1u] - b);  // (checked: below 4 GiB)
    const uint8_t* const p = txs + b;
    Decoded d;
    decode(p, len, chain_id, fork, d);
    const bool dec = d.status != ST_BAD_TX, ok = d.status == ST_OK;
    const Span none = {0u, 0u};
    const Out& o = dv.o;
    uint32_t f = PHANT_TX_UNDECODABLE;
    if (dec) {
        f = (ok ? 0u : PHANT_TX_BAD_V) | (d.create ? PHANT_TX_IS_CREATE : 0u) | (d.type && d.chain_id_field != chain_id ? PHANT_TX_CHAIN_ID : 0u);
        if (d.type >= 3u && d.create) f |= PHANT_TX_NO_TO;
        if (d.type == 3u) {
            if (d.blobs == 0u) f |= PHANT_TX_BLOB_NONE;
            for (uint32_t k = 0; k < d.blobs; ++k)  // (serial in its lane, like the access list)
                if (p[d.hashes.at + 33u * k + 1u] != 0x01u) f |= PHANT_TX_BLOB_VERSION;
        }
        if (d.type == 4u && d.tuples == 0u) f |= PHANT_TX_AUTH_NONE;
    }
    o.flags[i] = f;
    // the rows of types 3 and 4, the tuple count (block_transactions scans the counts into auth_first), the call's totals
    const uint32_t blobs = dec ? d.blobs : 0u, tuples = dec ? d.tuples : 0u;
    put_be32(dv.x.max_fee_per_blob_gas + 32ull * i, p, dec ? d.blob_fee : none);
    dv.x.blob_off[i] = dec && d.type == 3u ? b + d.hashes.at : 0u;
    dv.x.blobs[i] = blobs;
    dv.x.auth_first[i] = tuples;
    if (i == 0u) dv.x.auth_first[n] = 0u;
    dv.auth_at[i] = dec ? d.auths.at : 0u;
    dv.auth_len[i] = dec ? d.auths.len : 0u;
    if (tuples) atomicAdd(dv.ctl + 2, tuples);
    if (blobs) atomicAdd(reinterpret_cast<unsigned long long*>(dv.ctl + 4), (unsigned long long)blobs);
    o.type[i] = dec ? d.type : (uint8_t)0;
    o.nonce[i] = dec ? d.nonce : 0u;
    o.gas_limit[i] = dec ? d.gas_limit : 0u;
    o.chain_id[i] = !dec ? 0u : d.type ? d.chain_id_field : d.eip155 ? chain_id : 0u;
    put_be32(o.gas_price + 32ull * i, p, dec ? d.gas_price : none);
    put_be32(o.priority_fee + 32ull * i, p, dec ? d.priority : none);
    put_be32(o.value + 32ull * i, p, dec ? d.value : none);
    for (uint32_t k = 0; k < 20u; ++k) o.to[20ull * i + k] = dec && d.to.len ? p[d.to.at + k] : (uint8_t)0;
    o.data_off[i] = dec ? b + d.data.at : 0u;
    o.data_len[i] = dec ? d.data.len : 0u;
    o.al_off[i] = dec && d.type ? b + d.al.at : 0u;
    o.al_len[i] = dec ? d.al.len : 0u;
    o.al_addresses[i] = dec ? d.al_addresses : 0u;
    o.al_keys[i] = dec ? d.al_keys : 0u;
    // r, s, recid: for ecrecover_kernel (rows of 32 / 32 / 1) and as the caller's 65-byte row
    put_be32(dv.r + 32ull * i, p, ok ? d.r : none);
    put_be32(dv.s + 32ull * i, p, ok ? d.s : none);
    dv.recid[i] = ok ? d.recid : (uint8_t)0;
    dv.pre_status[i] = d.status;
    uint8_t* const sg = o.sig + 65ull * i;
    for (uint32_t k = 0; k < 32u; ++k) sg[k] = dv.r[32ull * i + k], sg[32u + k] = dv.s[32ull * i + k];
    sg[64] = dv.recid[i];
    Plan pl;
    pl.body_begin = d.body_begin, pl.body_end = d.body_end;
    pl.lens = (uint32_t)d.prefix_len | (uint32_t)d.suffix_len << 8 | (uint32_t)d.status << 16;
    pl.data_at = dec ? d.data.at : 0u, pl.data_len = dec ? d.data.len : 0u;
    for (uint32_t k = 0; k < 12u; ++k) {
        if (k >= d.prefix_len) d.prefix[k] = 0;
        if (k >= d.suffix_len) d.suffix[k] = 0;
    }
    for (uint32_t k = 0; k < 3u; ++k) pl.prefix[k] = pack4(d.prefix + 4u * k), pl.suffix[k] = pack4(d.suffix + 4u * k);
    pl.pad = 0;
    dv.plan[i] = pl;
}

// ---- the two hashes: one sponge loop over   prefix (registers) || body (memory) || suffix (registers)
struct __attribute__((packed, aligned(1))) PackedU32 { uint32_t x; };
PHANT_DEV uint32_t load32(const uint8_t* __restrict__ p) { return reinterpret_cast<const PackedU32*>(p)->x; }
// byte q (< 12) of three dwords, without indexing registers by a variable
PHANT_DEV uint32_t byte_of(const uint32_t (&w)[3], uint32_t q) {
    const uint32_t d = q < 4u ? w[0] : q < 8u ? w[1] : w[2];
    return (d >> (8u * (q & 3u))) & 0xffu;
}
struct Message {
    const uint8_t* body;  // message byte j, pl <= j < pl + bl, is body[j - pl]
    uint32_t pl, bl;
    uint64_t total;       // pl + bl + the suffix's bytes (64 bits: a transaction may be a few bytes short of 4 GiB)
    uint32_t prefix[3], suffix[3];
};
PHANT_DEV uint32_t message_byte(const Message& m, uint64_t j) {
    if (j < m.pl) return byte_of(m.prefix, (uint32_t)j);
    if (j - m.pl < m.bl) return m.body[j - m.pl];
    return j < m.total ? byte_of(m.suffix, (uint32_t)(j - m.pl - m.bl)) : 0u;
}
// the dword at message offset j (a multiple of 4): one load where it lies in the body, else byte by byte; zero behind the message
PHANT_DEV uint32_t message_dword(const Message& m, uint64_t j) {
    if (j >= m.total) return 0u;
    if (j >= m.pl && m.bl >= 4u && j - m.pl <= m.bl - 4u) return load32(m.body + (j - m.pl));
    return message_byte(m, j) | message_byte(m, j + 1u) << 8 | message_byte(m, j + 2u) << 16 | message_byte(m, j + 3u) << 24;
}
// bit 7 of every non-zero byte
PHANT_DEV uint32_t nonzero_bytes(uint32_t d) { return (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u; }
// the non-zero bytes of the block d (which starts `rel` bytes behind the calldata's first byte, modulo 2^32) that are calldata
PHANT_DEV uint32_t count_nonzero(const uint32_t (&d)[RATE_DWORDS], uint32_t rel, uint32_t data_len) {
    uint32_t c = 0;
    if (rel < data_len && data_len - rel >= RATE) {  // the whole block is calldata
#pragma unroll
        for (int i = 0; i < (int)RATE_DWORDS; ++i) c += (uint32_t)__popc(nonzero_bytes(d[i]));
    } else if (rel < data_len || rel > 0u - RATE) {  // it begins or ends inside this block
#pragma unroll
        for (int i = 0; i < (int)RATE_DWORDS; ++i) {
            const uint32_t q = rel + 4u * (uint32_t)i;
            const uint32_t mask = (q < data_len ? 0x80u : 0u) | (q + 1u < data_len ? 0x8000u : 0u) | (q + 2u < data_len ? 0x800000u : 0u) |
                                  (q + 3u < data_len ? 0x80000000u : 0u);
            c += (uint32_t)__popc(nonzero_bytes(d[i]) & mask);
        }
    }
    return c;
}

// the Keccak-256 of message m in s; -> the non-zero bytes of the calldata, which starts at message offset data_at
PHANT_DEV uint32_t hash_message(Sponge& s, const Message& m, uint32_t data_at, uint32_t data_len) {
    sponge_zero(s);
    uint32_t nonzero = 0;
    for (uint64_t j = 0;; j += RATE) {
        const uint64_t left = m.total - j;
        uint32_t d[RATE_DWORDS];
        if (j >= m.pl && m.bl >= RATE && j - m.pl <= m.bl - RATE) {
            load_block_wide(d, m.body + (j - m.pl));
        } else {
#pragma unroll
            for (int i = 0; i < (int)RATE_DWORDS; ++i) d[i] = message_dword(m, j + 4u * (uint64_t)i);
        }
        if (data_len) nonzero += count_nonzero(d, (uint32_t)j - data_at, data_len);
        if (left >= RATE) xor_block(s, d);
        else absorb_loaded_final(s, d, (uint32_t)left);
        keccak_f1600(s);
        if (left < RATE) break;
    }
    return nonzero;
}

__global__ void __launch_bounds__(64) tx_hash_kernel(const uint8_t* __restrict__ txs, const uint64_t* __restrict__ tx_off, uint32_t n,
                                                      const Plan* __restrict__ plan, uint8_t* __restrict__ tx_hash, uint8_t* __restrict__ sig_hash,
                                                      uint64_t* __restrict__ nonzero_out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = tx_off[i];
    const Plan pl = plan[i];
    Message m;
    m.body = txs + b, m.pl = 0u, m.bl = (uint32_t)(tx_off[i + 1u] - b), m.total = m.bl;
#pragma unroll
    for (int k = 0; k < 3; ++k) m.prefix[k] = m.suffix[k] = 0u;
    Sponge s;
    nonzero_out[i] = hash_message(s, m, pl.data_at, pl.data_len);  // (the rules kernel turns the count into the intrinsic gas)
    store_digest(s, tx_hash + 32ull * i);
    if ((pl.lens >> 16) == ST_OK) {
        m.body = txs + b + pl.body_begin, m.pl = pl.lens & 0xffu, m.bl = pl.body_end - pl.body_begin;
        m.total = (uint64_t)m.pl + m.bl + ((pl.lens >> 8) & 0xffu);
#pragma unroll
        for (int k = 0; k < 3; ++k) m.prefix[k] = pl.prefix[k], m.suffix[k] = pl.suffix[k];
        (void)hash_message(s, m, 0u, 0u);
    } else {
        sponge_zero(s);
    }
    store_digest(s, sig_hash + 32ull * i);
}

// ---- the authorization tuples of the type-4 transactions (EIP-7702)
// A lane per transaction walks its own tuples a second time and writes each one's fields into the rows from auth_first[i] on (n_auth
// rows in all): what the caller reads, and r / s / y_parity / the tuple's own verdict for the recovery.
__global__ void __launch_bounds__(64) tx_auth_rows_kernel(const uint8_t* __restrict__ txs, const uint64_t* __restrict__ tx_off, uint32_t n,
                                                           uint64_t chain_id, Dev dv, AuthDev ad, uint32_t n_auth) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t first = dv.x.auth_first[i], count = dv.x.auth_first[i + 1u] - first;
    if (count == 0u) return;
    const uint8_t* const p = txs + tx_off[i];
    uint32_t pos = dv.auth_at[i];
    const uint32_t end = pos + dv.auth_len[i];
    for (uint32_t k = 0; k < count; ++k) {
        const uint64_t j = (uint64_t)first + k;
        Auth a;
        if (j >= n_auth || !auth_tuple(p, pos, end, a, pos)) return;  // (neither happens: the decode accepted and counted these tuples)
        put_be32(ad.x.auth_chain_id + 32u * j, p, a.chain_id);
        for (uint32_t q = 0; q < 20u; ++q) ad.x.auth_address[20u * j + q] = p[a.address.at + q];
        const uint64_t nonce = be_u64(p, a.nonce.at, a.nonce.at + a.nonce.len);
        ad.x.auth_nonce[j] = nonce;
        put_be32(ad.r + 32u * j, p, a.r);
        put_be32(ad.s + 32u * j, p, a.s);
        const uint8_t y = a.y_parity.len ? p[a.y_parity.at] : (uint8_t)0;
        ad.recid[j] = y;
        const bool foreign = a.chain_id.len > 8u || (a.chain_id.len != 0u && be_u64(p, a.chain_id.at, a.chain_id.at + a.chain_id.len) != chain_id);
        ad.pre_status[j] = foreign ? ST_AUTH_CHAIN_ID : nonce == ~0ull ? ST_AUTH_NONCE_MAX : y > 1u ? ST_BAD_V : ST_OK;
        uint8_t* const sg = ad.x.auth_sig + 65u * j;
        for (uint32_t q = 0; q < 32u; ++q) sg[q] = ad.r[32u * j + q], sg[32u + q] = ad.s[32u * j + q];
        sg[64] = y;
    }
}

// What an authority signs, keccak256(0x05 || rlp([chain_id, address, nonce])): at most 1 + 2 + (33 + 21 + 9) = 66 bytes, one block.
struct AuthMessage {
    const uint8_t *chain_id, *address;  // the rows of 32 and of 20 bytes
    uint64_t nonce;
    uint32_t cl, nl;           // the significant bytes of chain_id and of nonce
    uint32_t ce, ne, hl, pay;  // the bytes of their encodings, of the list header, of the list's payload
};
// Byte j of that message.  The encoding is never written anywhere, so rlp.h's writers do not apply: this states the layout a second
// time, for the lengths rlp.h has computed (tx_auth_hash_kernel), and stays here.
PHANT_DEV uint32_t auth_message_byte(const AuthMessage& m, uint32_t j) {
    if (j == 0u) return 0x05u;
    if (j <= m.hl) return m.hl == 1u ? 0xc0u + m.pay : j == 1u ? 0xf8u : m.pay;
    uint32_t q = j - 1u - m.hl;
    if (q < m.ce) {
        if (m.ce == 1u) return m.cl ? m.chain_id[31] : 0x80u;
        return q == 0u ? 0x80u + m.cl : m.chain_id[32u - m.cl + q - 1u];
    }
    q -= m.ce;
    if (q < 21u) return q == 0u ? 0x94u : m.address[q - 1u];
    q -= 21u;
    if (q >= m.ne) return 0u;
    if (m.ne == 1u) return m.nl ? (uint32_t)(m.nonce & 0xffu) : 0x80u;
    return q == 0u ? 0x80u + m.nl : (uint32_t)(m.nonce >> (8u * (m.nl - q))) & 0xffu;
}

// A lane per tuple: the message is built in registers from the tuple's rows and written nowhere.
__global__ void __launch_bounds__(64) tx_auth_hash_kernel(AuthDev ad, uint32_t n_auth) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= n_auth) return;
    AuthMessage m;
    m.chain_id = ad.x.auth_chain_id + 32ull * j, m.address = ad.x.auth_address + 20ull * j, m.nonce = ad.x.auth_nonce[j];
    m.cl = be_bytes(m.chain_id, 32u);
    m.nl = uint_bytes(m.nonce);
    m.ce = (uint32_t)str_len(m.cl, m.chain_id[31]);
    m.ne = uint_len(m.nonce);
    m.pay = m.ce + 21u + m.ne;
    m.hl = hdr_len(m.pay);  // (two bytes only with a chain id of 24 bytes or more)
    const uint32_t total = 1u + m.hl + m.pay;
    uint32_t d[RATE_DWORDS];
#pragma unroll
    for (int i = 0; i < (int)RATE_DWORDS; ++i) {
        const uint32_t at = 4u * (uint32_t)i;
        d[i] = i >= 17 ? 0u
                       : auth_message_byte(m, at) | auth_message_byte(m, at + 1u) << 8 | auth_message_byte(m, at + 2u) << 16 | auth_message_byte(m, at + 3u) << 24;
    }
    Sponge s;
    sponge_zero(s);
    absorb_loaded_final(s, d, total);
    keccak_f1600(s);
    store_digest(s, ad.x.auth_hash + 32ull * j);
}

// ---- the rules: 256-bit integers as eight 32-bit limbs, little-endian
TX_HD void load_u256(const uint8_t* be, uint32_t w[8]) {
    for (int k = 0; k < 8; ++k) {
        const uint8_t* p = be + 28 - 4 * k;
        w[k] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    }
}
TX_HD void store_u256(uint8_t* be, const uint32_t w[8]) {
    for (int k = 0; k < 8; ++k) {
        uint8_t* p = be + 28 - 4 * k;
        p[0] = (uint8_t)(w[k] >> 24), p[1] = (uint8_t)(w[k] >> 16), p[2] = (uint8_t)(w[k] >> 8), p[3] = (uint8_t)w[k];
    }
}
TX_HD bool less_u256(const uint32_t a[8], const uint32_t b[8]) {
    for (int k = 7; k >= 0; --k)
        if (a[k] != b[k]) return a[k] < b[k];
    return false;
}

// The rules of transaction i under the block parameters ru, stated ONCE: tx_rules_kernel has ru from its arguments, bodies.hip.h's
// body_rules_kernel builds it from the per-block arrays of a chain segment.  Writes the row's rule outputs -> its flags.
// sig_status: the recovery's verdicts, or null (PHANT_TXS_NO_RECOVERY)
PHANT_DEV uint32_t rules_row(uint32_t i, const Rules& ru, const Dev& dv, const uint8_t* __restrict__ sig_status) {
    const Out& o = dv.o;
    uint32_t f = o.flags[i];
    uint32_t eff[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cost[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t intrinsic = 0, floor_gas = 0;
    if (!(f & PHANT_TX_UNDECODABLE)) {
        const bool create = (f & PHANT_TX_IS_CREATE) != 0u;
        const uint32_t type = o.type[i], data_len = o.data_len[i];
        const uint64_t gas_limit = o.gas_limit[i], nonzero = o.intrinsic_gas[i];  // (the hash kernel's count)
        if (sig_status && sig_status[i] != PHANT_SIG_OK && sig_status[i] != PHANT_SIG_BAD_V) f |= PHANT_TX_SIGNATURE;
        const uint64_t tuples = dv.x.auth_first[i + 1u] - dv.x.auth_first[i];  // (scanned by now, or all zero)
        intrinsic = 21000u + 4u * ((uint64_t)data_len - nonzero) + 16u * nonzero + 2400u * (uint64_t)o.al_addresses[i] + 1900u * (uint64_t)o.al_keys[i] +
                    AUTH_COST * tuples;
        if (create) intrinsic += 32000u + 2u * (((uint64_t)data_len + 31u) / 32u);
        if (ru.fork >= FORK_PRAGUE) {  // EIP-7623: a token is a zero byte, four a non-zero one
            floor_gas = 21000u + FLOOR_PER_TOKEN * (((uint64_t)data_len - nonzero) + 4u * nonzero);
            if (gas_limit < floor_gas) f |= PHANT_TX_FLOOR_GAS;
        }
        uint32_t price[8], prio[8], value[8];
        load_u256(o.gas_price + 32ull * i, price);
        load_u256(o.priority_fee + 32ull * i, prio);
        load_u256(o.value + 32ull * i, value);
        if (ru.have_base_fee) {
            if (type >= 2u && less_u256(price, prio)) f |= PHANT_TX_PRIORITY_ABOVE_MAX;
            if (less_u256(price, ru.base_fee)) f |= PHANT_TX_FEE_BELOW_BASE;
            if (!(f & (PHANT_TX_PRIORITY_ABOVE_MAX | PHANT_TX_FEE_BELOW_BASE))) {
                if (type >= 2u) {  // min(priority, max_fee - base_fee) + base_fee
                    uint32_t room[8];
                    uint64_t c = 0;
                    for (int k = 0; k < 8; ++k) {
                        const uint64_t t = (uint64_t)price[k] - ru.base_fee[k] - c;
                        room[k] = (uint32_t)t, c = (t >> 32) & 1u;
                    }
                    const bool take_prio = less_u256(prio, room);
                    c = 0;
                    for (int k = 0; k < 8; ++k) {
                        c += (uint64_t)(take_prio ? prio[k] : room[k]) + ru.base_fee[k];
                        eff[k] = (uint32_t)c, c >>= 32;
                    }
                } else {
                    for (int k = 0; k < 8; ++k) eff[k] = price[k];
                }
            }
        }
        if (ru.have_gas_limit && gas_limit > ru.block_gas_limit) f |= PHANT_TX_GAS_ABOVE_BLOCK;
        if (intrinsic > gas_limit) f |= PHANT_TX_INTRINSIC_GAS;
        if (o.nonce[i] == ~0ull) f |= PHANT_TX_NONCE_MAX;
        if (create && data_len > 2u * 0x6000u) f |= PHANT_TX_INITCODE_SIZE;
        // type 3: max_fee_per_blob_gas against the block's blob base fee, and the blob gas (below 2^49: a transaction is shorter than 4 GiB)
        uint32_t blob_fee[8];
        load_u256(dv.x.max_fee_per_blob_gas + 32ull * i, blob_fee);
        if (type == 3u && ru.have_blob_base_fee && less_u256(blob_fee, ru.blob_base_fee)) f |= PHANT_TX_BLOB_FEE_BELOW_BASE;
        const uint64_t blob_gas = GAS_PER_BLOB * (uint64_t)dv.x.blobs[i];
        // gas_limit x getGasPrice() + value + blob_gas x max_fee_per_blob_gas: column k of the schoolbook products is
        // price[k] g0 + price[k - 1] g1 + blob_fee[k] h0 + blob_fee[k - 1] h1
        const uint32_t g0 = (uint32_t)gas_limit, g1 = (uint32_t)(gas_limit >> 32), h0 = (uint32_t)blob_gas, h1 = (uint32_t)(blob_gas >> 32);
        uint64_t carry = 0;
        uint32_t over = 0;
        for (int k = 0; k < 10; ++k) {
            const uint64_t a = k < 8 ? (uint64_t)price[k] * g0 : 0ull, b = (k >= 1 && k <= 8) ? (uint64_t)price[k - 1] * g1 : 0ull;
            const uint64_t c = k < 8 ? (uint64_t)blob_fee[k] * h0 : 0ull, e = (k >= 1 && k <= 8) ? (uint64_t)blob_fee[k - 1] * h1 : 0ull;
            const uint64_t lo = (carry & 0xffffffffull) + (a & 0xffffffffull) + (b & 0xffffffffull) + (c & 0xffffffffull) + (e & 0xffffffffull) +
                                (k < 8 ? value[k] : 0u);
            if (k < 8) cost[k] = (uint32_t)lo;
            else over |= (uint32_t)lo;
            carry = (carry >> 32) + (a >> 32) + (b >> 32) + (c >> 32) + (e >> 32) + (lo >> 32);
        }
        if (over || carry) {
            f |= PHANT_TX_COST_OVERFLOW;
            for (int k = 0; k < 8; ++k) cost[k] = 0u;
        }
    }
    o.flags[i] = f;
    o.intrinsic_gas[i] = intrinsic;
    dv.x.floor_gas[i] = floor_gas;
    store_u256(o.effective_gas_price + 32ull * i, eff);
    store_u256(o.upfront_cost + 32ull * i, cost);
    return f;
}

__global__ void __launch_bounds__(64) tx_rules_kernel(uint32_t n, Rules ru, Dev dv, const uint8_t* __restrict__ sig_status) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = rules_row(i, ru, dv, sig_status);
    if (f & ERROR_BITS) atomicMax(dv.ctl + 1, n - i);
}

// what the host form refuses before anything is copied
inline int32_t check_host(const In& in, std::string& err) {
    return seg::check_offsets_host("block_transactions", "tx_off", "transaction", in.tx_off, in.n, err);
}

// A call between its steps, which phant_block_transactions[_ex] (below) and phant_block_bodies (bodies.hip.h) both go through:
//   call_begin    what the host form refuses, the bytes, whether a tuple can occur
//   call_carve    the call's part of the `io` arena: control words and outputs in front (one span goes back), the internal arrays,
//                 (host form) offsets and bytes last
//   call_kernels  decode, hash, (the authorization tuples,) recover: every launch in front of the rules
//   call_outputs  every output named for CallOutputs
struct Call {
    Dev d;
    AuthDev ad;
    uint32_t* d_scan;
    const uint8_t* d_txs;
    const uint64_t* d_off;
    uint64_t bytes;
    uint32_t n, n_auth;
    bool maybe_tuples;
};

inline int32_t call_begin(Call& c, const In& in, uint32_t fork, bool dev, std::string& err) {
    std::memset(&c, 0, sizeof c);
    c.n = in.n, c.d_txs = in.txs, c.d_off = in.tx_off, c.bytes = in.tx_bytes;
    // can the call hold an authorization tuple?  The host form sees every transaction's first byte; the device form cannot know
    c.maybe_tuples = fork >= FORK_PRAGUE && dev;
    if (!dev) {
        const int32_t rc = check_host(in, err);
        if (rc) return rc;
        c.bytes = in.tx_off[in.n];
        if (fork >= FORK_PRAGUE)
            for (uint32_t i = 0; i < in.n && !c.maybe_tuples; ++i) c.maybe_tuples = in.tx_off[i + 1u] > in.tx_off[i] && in.txs[in.tx_off[i]] == 4u;
    }
    if (c.maybe_tuples && c.bytes / 27u > 0xffffffffull) return err = "block_transactions: more bytes than 2^32 authorization tuples take", PHANT_E_UNSUPPORTED;
    return PHANT_OK;
}

template <class IO>
void call_carve(IO& io, Call& c, bool dev) {
    Dev& d = c.d;
    const uint32_t n = c.n;
    d.ctl = io.template take<uint32_t>(CTL_WORDS);
#define X(m, T, e) d.o.m = io.template take<T>((size_t)n * e);
    TX_OUTPUTS(X)
#undef X
    d.x.auth_first = io.template take<uint32_t>((size_t)n + 1);
#define X(m, T, e) d.x.m = io.template take<T>((size_t)n * e);
    TX_EX_OUTPUTS(X)
#undef X
    d.plan = io.template take<Plan>((size_t)n);
    d.r = io.template take<uint8_t>(32 * (size_t)n);
    d.s = io.template take<uint8_t>(32 * (size_t)n);
    d.recid = io.template take<uint8_t>((size_t)n);
    d.pre_status = io.template take<uint8_t>((size_t)n);
    d.auth_at = io.template take<uint32_t>((size_t)n);
    d.auth_len = io.template take<uint32_t>((size_t)n);
    if (c.maybe_tuples) c.d_scan = io.template take<uint32_t>(scan_scratch_entries(n + 1u));
    if (!dev) {
        c.d_off = io.template take<uint64_t>((size_t)n + 1);
        c.d_txs = io.template take<uint8_t>((size_t)c.bytes + 16);
    }
}

inline int32_t call_kernels(Workspaces& ws, hipStream_t st, Call& c, uint64_t chain_id, uint32_t fork, bool recover, const uint32_t* gtable,
                            std::string& err) {
    Dev& d = c.d;
    AuthDev& ad = c.ad;
    const uint32_t n = c.n, grid64 = (n + 63u) / 64u;
    const uint8_t* const d_txs = c.d_txs;
    const uint64_t* const d_off = c.d_off;
    uint32_t* const d_scan = c.d_scan;
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_TXS;
    hipLaunchKernelGGL(tx_decode_kernel, dim3(grid64), dim3(64), 0, st, d_txs, d_off, n, chain_id, fork, d);
    CALL_TRY("block_transactions", hipGetLastError());
    hipLaunchKernelGGL(tx_hash_kernel, dim3(grid64), dim3(64), 0, st, d_txs, d_off, n, d.plan, d.o.tx_hash, d.o.sig_hash, d.o.intrinsic_gas);
    CALL_TRY("block_transactions", hipGetLastError());
    const uint32_t low_s = PHANT_RECOVER_LOW_S;  // validateSignatureFields
    uint32_t n_auth = 0;
    if (c.maybe_tuples) {
        CALL_TRY("block_transactions", ws.read_words(Workspaces::MAILBOX_TXS, d.ctl, CTL_WORDS, st));
        n_auth = mb[2];
    }
    c.n_auth = n_auth;
    if (n_auth) {
        // the rows of the tuples, now that they are counted, in an arena of their own (the call's other arrays stay where they are)
        auto carve_auth = [&](auto& io) {
#define X(m, T, e) ad.x.m = io.template take<T>((size_t)n_auth * e);
            TX_AUTH_OUTPUTS(X)
#undef X
            ad.r = io.template take<uint8_t>(32 * (size_t)n_auth);
            ad.s = io.template take<uint8_t>(32 * (size_t)n_auth);
            ad.recid = io.template take<uint8_t>((size_t)n_auth);
            ad.pre_status = io.template take<uint8_t>((size_t)n_auth);
        };
        // (no synchronisation before the arena grows -- the stream is idle: the control words were just read)
        if (const int32_t rc = lay_out_status(lay_out_arena(ws.txa, st, carve_auth, true), "block_transactions", "authorizations", err)) return rc;
        CALL_TRY("block_transactions", launch_exclusive_scan_u32(d.x.auth_first, n + 1u, d_scan, st));
        hipLaunchKernelGGL(tx_auth_rows_kernel, dim3(grid64), dim3(64), 0, st, d_txs, d_off, n, chain_id, d, ad, n_auth);
        CALL_TRY("block_transactions", hipGetLastError());
        hipLaunchKernelGGL(tx_auth_hash_kernel, dim3((n_auth + 63u) / 64u), dim3(64), 0, st, ad, n_auth);
        CALL_TRY("block_transactions", hipGetLastError());
        if (recover)
            CALL_TRY("block_transactions", launch_ecrecover(ad.x.auth_hash, ad.r, ad.s, ad.recid, ad.pre_status, n_auth, low_s, gtable, nullptr, ad.x.authority, ad.x.auth_status, st));
    }
    if (recover) CALL_TRY("block_transactions", launch_ecrecover(d.o.sig_hash, d.r, d.s, d.recid, d.pre_status, n, low_s, gtable, nullptr, d.o.sender, d.o.sig_status, st));
    return PHANT_OK;
}

// how many outputs a call names at most (bodies.hip.h adds its own to them)
#define X(m, T, e) +1
constexpr int CALL_OUTPUTS = 0 TX_AUTH_OUTPUTS(X) TX_OUTPUTS(X) TX_EX_OUTPUTS(X) + 1;
#undef X
static_assert(CALL_OUTPUTS <= CallOutputs::CAP, "the longest list of outputs fits");

// the rows of the tuples (at most auth_cap of them) lie in their own arena: copies of their own in both forms
inline void call_outputs(CallOutputs& outs, const Call& c, const phant_txs_ex_out& xout, uint32_t auth_cap) {
    const Dev& d = c.d;
    const AuthDev& ad = c.ad;
    const phant_txs_out& out = xout.base;
    const uint32_t n = c.n;
    const size_t auth_rows = std::min(c.n_auth, auth_cap);
#define X(m, T, e) outs.add(xout.m, ad.x.m, auth_rows * e * sizeof(T));
    TX_AUTH_OUTPUTS(X)
#undef X
#define X(m, T, e) outs.add(out.m, d.o.m, (size_t)n * e * sizeof(T));
    TX_OUTPUTS(X)
#undef X
    outs.add(xout.auth_first, d.x.auth_first, 4 * ((size_t)n + 1));
#define X(m, T, e) outs.add(xout.m, d.x.m, (size_t)n * e * sizeof(T));
    TX_EX_OUTPUTS(X)
#undef X
}

}  // namespace tx

int32_t block_transactions(Workspaces& ws, hipStream_t st, const phant_txs_ex_in& xin, phant_txs_ex_out& xout, bool dev, const uint32_t* gtable,
                           std::string& err) {
    using namespace tx;
    const phant_txs_in& in = xin.base;
    phant_txs_out& out = xout.base;
    const uint32_t n = in.n, fork = xin.fork;
    const bool recover = !(in.flags & PHANT_TXS_NO_RECOVERY);
    CALL_TRY("block_transactions", ws.ensure_mailbox());
    static_assert(CTL_WORDS <= Workspaces::MAILBOX_TXS_WORDS, "the control words fit their part of the mailbox");
    volatile uint32_t* const mb = ws.mailbox + Workspaces::MAILBOX_TXS;
    Call c;
    if (const int32_t rc = call_begin(c, in, fork, dev, err)) return rc;
    if (const int32_t rc = lay_out_status(lay_out_arena(ws.io, st, [&](auto& io) { call_carve(io, c, dev); }), "block_transactions", "workspace", err)) return rc;
    Dev& d = c.d;
    CALL_TRY("block_transactions", hipMemsetAsync(d.ctl, 0, 4 * CTL_WORDS, st));

    // ---- in: (host form) offsets and bytes in ONE copy through the pinned stage where they fit it; (device form) the offsets' check
    const uint32_t grid256 = (n + 255u) / 256u, grid64 = (n + 63u) / 64u;
    if (!dev) {
        StagedInputs ins(ws, st, c.d_off, c.d_txs + c.bytes);
        ins.put(c.d_off, in.tx_off, 8 * ((size_t)n + 1));
        ins.put(c.d_txs, in.txs, (size_t)c.bytes);
        CALL_TRY("block_transactions", ins.finish());
    } else {
        hipLaunchKernelGGL(tx_check_args_kernel, dim3(grid256), dim3(256), 0, st, c.d_off, n, c.bytes, d.ctl);
        CALL_TRY("block_transactions", hipGetLastError());
        CALL_TRY("block_transactions", ws.read_words(Workspaces::MAILBOX_TXS, d.ctl, CTL_WORDS, st));
        if (mb[0] & seg::F_INVALID) return err = "block_transactions_dev: tx_off does not run from 0 to tx_bytes, or goes backwards", PHANT_E_INVALID_ARG;
        if (mb[0] & seg::F_TOO_LONG) return err = "block_transactions_dev: a transaction of 4 GiB or more", PHANT_E_UNSUPPORTED;
    }

    // ---- decode, hash, (the authorization tuples,) recover, rules
    Rules ru;
    std::memset(&ru, 0, sizeof ru);
    if (in.base_fee) load_u256(in.base_fee, ru.base_fee), ru.have_base_fee = 1u;
    if (xin.blob_base_fee) load_u256(xin.blob_base_fee, ru.blob_base_fee), ru.have_blob_base_fee = 1u;
    ru.have_gas_limit = (in.flags & PHANT_TXS_HAVE_GAS_LIMIT) ? 1u : 0u;
    ru.block_gas_limit = in.block_gas_limit;
    ru.fork = fork;
    if (const int32_t rc = call_kernels(ws, st, c, in.chain_id, fork, recover, gtable, err)) return rc;
    hipLaunchKernelGGL(tx_rules_kernel, dim3(grid64), dim3(64), 0, st, n, ru, d, recover ? d.o.sig_status : nullptr);
    CALL_TRY("block_transactions", hipGetLastError());

    // ---- out: the control words and everything up to the last wanted output (one span in the host form while it fits the pinned stage)
    CallOutputs outs(ws, st, dev, d.ctl, d.ctl, Workspaces::MAILBOX_TXS, CTL_WORDS);
    call_outputs(outs, c, xout, xin.auth_cap);
    CALL_TRY("block_transactions", outs.deliver());
    const volatile uint32_t* const ctl = outs.ctl();
    out.first_bad = n - ctl[1];
    xout.n_auth = ctl[2];
    xout.blob_gas_used = GAS_PER_BLOB * ((uint64_t)ctl[4] | (uint64_t)ctl[5] << 32);
    return PHANT_OK;
}

#undef TX_OUTPUTS
#undef TX_EX_OUTPUTS
#undef TX_AUTH_OUTPUTS

}  // namespace phant
#endif  // PHANT_TX_DECODE_ONLY
#undef TX_HD
