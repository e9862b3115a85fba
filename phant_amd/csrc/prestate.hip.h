// prestate.hip.h -- the pre-state of an execution witness (phant_exec_witness_prestate), the kernels between and behind the two walks
// of the node-set pipeline.  Included by mpt_verify_nodeset.hip (its keyed slot mix, ns::home_hash, keys the code table too).
//
//   account_decode_kernel  a lane per account: its proven leaf strictly as canonical rlp([nonce, balance, storageRoot, codeHash])
//                          (nonce <= 8 bytes, balance <= 32, neither with a leading zero, both hashes exactly 32 bytes, nothing
//                          behind the list) into the struct-of-arrays; an ABSENT account gets the empty account.  The storage root
//                          it writes IS the root table of the storage walk (no host round trip between the two walks).  A leaf
//                          that is no account body: PHANT_PROOF_BAD_VALUE.
//   slot_decode_kernel     a lane per slot: rlp(minimal big-endian integer), 1 to 32 bytes, non-zero, into a 32-byte word;
//                          ABSENT = zero; a slot under an account that is neither PRESENT nor ABSENT: PHANT_PROOF_MISMATCH.
//   code_hash_kernel       a half wave per code (coop_sponge.hip.h's 25-lane sponge: 17 lanes absorb 8 bytes of a rate block
//                          each): contract code runs to 24 576 bytes = 181 permutations in series, the longest chain of the
//                          call -- on a helper stream, next to the node-set kernels.  Lane 0 of the half puts the digest into a
//                          small table keyed by it that keeps the LOWEST code index (duplicate codes).  Form 1: a lane per code
//                          (keccak256_global), for the A/B of DESIGN.md.
//   code_match_kernel      a lane per account: a PRESENT account whose codeHash is not keccak256("") looks its digest up.
//   code_unused_kernel     a lane per code: its digest was matched by no account.
#pragma once
#include <phant_platform.h>

#include "coop_sponge.hip.h"
#include "launch.h"
#include "rlp.h"
#include "../../include/phant_gpu.h"

namespace phant {
namespace pre {

// empty_mpt_root and keccak256(""), as the little-endian words a digest is compared in
PHANT_DEV uint32_t empty_root_word(uint32_t w) {
    constexpr uint32_t R[8] = {0x171fe856u, 0xa655cc1bu, 0xe64583ffu, 0x6ef8c092u, 0x1be0485bu, 0xc0ad6c99u, 0xb52f6201u, 0x21b463e3u};
    return R[w];
}
PHANT_DEV uint32_t empty_code_word(uint32_t w) {
    constexpr uint32_t K[8] = {0x0146d2c5u, 0x3c23f786u, 0xb27d7e92u, 0xc003c7dcu, 0x53b600e5u, 0x3b2782cau, 0x04d8fa7bu, 0x70a4855du};
    return K[w];
}
PHANT_DEV void put_word(uint8_t* p, uint32_t w, uint32_t v) {
    for (uint32_t b = 0; b < 4u; ++b) p[4u * w + b] = (uint8_t)(v >> (8u * b));
}
PHANT_DEV uint32_t get_word(const uint8_t* p, uint32_t w) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4u; ++b) v |= (uint32_t)p[4u * w + b] << (8u * b);
    return v;
}

__global__ void __launch_bounds__(256) account_decode_kernel(const phant::PrestateArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    uint32_t st = a.acc_status[i];
    uint8_t* const bal = a.balances + 32ull * i;
    uint8_t* const sr = a.storage_roots + 32ull * i;
    uint8_t* const ch = a.code_hashes + 32ull * i;
    uint64_t nonce = 0;
    bool decoded = false;
    if (st == PHANT_PROOF_PRESENT) {
        const uint8_t* const v = a.nodes + a.acc_voff[i];
        const uint32_t len = a.acc_vlen[i];
        // the body: one list that is the whole value (rlp.h's decoder: canonical or refused), four strings inside it
        const MemBytes vb{v};
        RlpItem body;
        bool ok = rlp_decode(vb, 0u, len, body) && body.is_list && body.total == len;
        uint32_t p = ok ? body.pay : 0u;
        uint32_t cb[4] = {0, 0, 0, 0}, cl[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 4u && ok; ++k) {
            RlpItem it;
            ok = rlp_decode(vb, p, len - p, it) && !it.is_list;
            if (ok) cb[k] = it.pay, cl[k] = it.len, p += it.total;
        }
        ok = ok && p == len;                                               // nothing behind the fourth item
        ok = ok && cl[0] <= 8u && (cl[0] == 0u || v[cb[0]] != 0u);         // nonce: u64, minimal
        ok = ok && cl[1] <= 32u && (cl[1] == 0u || v[cb[1]] != 0u);        // balance: u256, minimal
        ok = ok && cl[2] == 32u && cl[3] == 32u;                           // storageRoot, codeHash
        if (ok) {
            for (uint32_t t = 0; t < cl[0]; ++t) nonce = nonce << 8 | v[cb[0] + t];
            for (uint32_t t = 0; t < 32u; ++t) bal[t] = t < 32u - cl[1] ? 0u : v[cb[1] + t - (32u - cl[1])];
            for (uint32_t t = 0; t < 32u; ++t) {
                sr[t] = v[cb[2] + t];
                ch[t] = v[cb[3] + t];
            }
            decoded = true;
        } else {
            st = PHANT_PROOF_BAD_VALUE;
        }
    }
    if (!decoded) {  // absent: the empty account; failed: the same values, and its slots are not anchored (slot_decode_kernel)
        for (uint32_t t = 0; t < 32u; ++t) bal[t] = 0u;
        for (uint32_t w = 0; w < 8u; ++w) {
            put_word(sr, w, empty_root_word(w));
            put_word(ch, w, empty_code_word(w));
        }
    }
    a.nonces[i] = nonce;
    a.acc_status[i] = (uint8_t)st;
    if (!(st == PHANT_PROOF_PRESENT || st == PHANT_PROOF_ABSENT)) atomicAdd(&a.counters[PRE_CNT_FAILED], 1u);
}

__global__ void __launch_bounds__(256) slot_decode_kernel(const phant::PrestateArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.ns) return;
    const uint32_t ast = a.acc_status[a.slot_account[j]];
    uint32_t st = a.slot_status[j];
    uint8_t* const out = a.slot_vals + 32ull * j;
    uint32_t cb = 0, cl = 0;
    const uint8_t* v = a.nodes;
    if (!(ast == PHANT_PROOF_PRESENT || ast == PHANT_PROOF_ABSENT)) {
        st = PHANT_PROOF_MISMATCH;  // walked from a storage root nothing commits to
    } else if (st == PHANT_PROOF_PRESENT) {
        v = a.nodes + a.slot_voff[j];
        const uint32_t len = a.slot_vlen[j];
        RlpItem it;
        const bool ok = rlp_decode(MemBytes{v}, 0u, len, it) && !it.is_list && it.total == len && it.len >= 1u && it.len <= 32u && v[it.pay] != 0u;
        if (ok) cb = it.pay, cl = it.len;
        else st = PHANT_PROOF_BAD_VALUE;
    }
    if (st != PHANT_PROOF_PRESENT) cl = 0;
    for (uint32_t t = 0; t < 32u; ++t) out[t] = t < 32u - cl ? 0u : v[cb + t - (32u - cl)];
    a.slot_status[j] = (uint8_t)st;
    if (!(st == PHANT_PROOF_PRESENT || st == PHANT_PROOF_ABSENT)) atomicAdd(&a.counters[PRE_CNT_FAILED], 1u);
}

// Code k's digest into the table: a slot names 1 + a code index or is free; a slot whose code has the same digest takes the
// lower index.  The digest of the code a slot names was written (and fenced) by that code's lane before its compare-and-swap;
// it is read here by atomics, past any cache line this CU may hold from before.
PHANT_DEV void code_insert(const phant::PrestateArgs& a, uint32_t k, const uint32_t (&d)[8]) {
    uint32_t slot = ns::home_hash(d[0], d[1], a.salt0, a.salt1) & a.mask;
    for (;;) {  // the table has >= 2 nc slots: terminates
        const uint32_t old = atomicCAS(&a.table[slot], 0u, k + 1u);
        if (old == 0u) break;
        __threadfence();
        uint32_t* const o = a.code_dig + 8ull * (old - 1u);
        uint32_t diff = 0;
        for (uint32_t w = 0; w < 8u; ++w) diff |= atomicAdd(&o[w], 0u) ^ d[w];
        if (diff == 0u) {  // (the slot may have taken a lower index of the same digest meanwhile: the digest is the same)
            atomicMin(&a.table[slot], k + 1u);
            break;
        }
        slot = (slot + 1u) & a.mask;
    }
    a.code_slot[k] = slot;
}

// form 0: a half wave per code.  Both halves of a wave run as many permutations as the longer of their codes needs (the sponge's
// cross-lane steps stay inside a half; the round constants are read from the first half's lanes) and keep their own digest.
__global__ void __launch_bounds__(256) code_hash_kernel(const phant::PrestateArgs a, const bool few) {
    struct __attribute__((packed, aligned(1))) U64 { unsigned long long v; };
    const uint32_t tid = threadIdx.x, l = tid & 31u, base = tid & 32u;
    const uint32_t k = blockIdx.x * (blockDim.x >> 5) + (tid >> 5);
    const bool active = k < a.nc;
    uint64_t b = 0, len = 0;
    if (active) {
        b = a.code_off[k];
        len = a.code_off[k + 1] - b;
    }
    const uint8_t* const ptr = a.codes + b;
    const uint32_t nb = active ? (uint32_t)(len / RATE) + 1u : 0u;
    const uint32_t nb_other = __shfl(nb, (int)(base ^ 32u), 64);
    const uint32_t nb_max = nb > nb_other ? nb : nb_other;
    const CoopLane c = coop_lane(l, base, few);
    uint32_t lo = 0, hi = 0, dlo = 0, dhi = 0;
    for (uint32_t blk = 0; blk < nb_max; ++blk) {
        if (blk < nb && l < 17u) {
            const uint64_t off = (uint64_t)blk * RATE + 8u * l;
            unsigned long long w = 0;
            if (off + 8u <= len) {
                w = reinterpret_cast<const U64*>(ptr + off)->v;
            } else {
                for (uint32_t t = 0; t < 8u; ++t) {
                    const uint64_t q = off + t;
                    if (q < len) w |= (unsigned long long)ptr[q] << (8u * t);
                    else if (q == len) w |= 0x01ull << (8u * t);  // Keccak-256's domain byte
                }
            }
            if (blk + 1u == nb && l == 16u) w |= 0x80ull << 56;  // the end of pad10*1
            lo ^= (uint32_t)w;
            hi ^= (uint32_t)(w >> 32);
        }
        coop_permute(c, lo, hi);
        if (blk + 1u == nb) {
            dlo = lo;
            dhi = hi;
        }
    }
    uint32_t d[8];
    for (int w = 0; w < 4; ++w) {
        d[2 * w] = (uint32_t)__shfl((int)dlo, (int)base + w, 64);
        d[2 * w + 1] = (uint32_t)__shfl((int)dhi, (int)base + w, 64);
    }
    if (!active || l != 0u) return;
    for (uint32_t w = 0; w < 8u; ++w) a.code_dig[8ull * k + w] = d[w];
    __threadfence();  // the digest before the slot that names it
    code_insert(a, k, d);
}

// form 1: a lane per code
__global__ void __launch_bounds__(256) code_hash_lane_kernel(const phant::PrestateArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nc) return;
    const uint64_t b = a.code_off[k];
    Sponge s;
    keccak256_global(s, a.codes + b, a.code_off[k + 1] - b, a.codes + a.code_off[a.nc]);
    const uint32_t d[8] = {s.lo[0], s.hi[0], s.lo[1], s.hi[1], s.lo[2], s.hi[2], s.lo[3], s.hi[3]};
    for (uint32_t w = 0; w < 8u; ++w) a.code_dig[8ull * k + w] = d[w];
    __threadfence();
    code_insert(a, k, d);
}

__global__ void __launch_bounds__(256) code_match_kernel(const phant::PrestateArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    uint32_t idx = PHANT_CODE_NONE;
    if (a.acc_status[i] == PHANT_PROOF_PRESENT) {
        uint32_t want[8];
        bool empty = true;
        for (uint32_t w = 0; w < 8u; ++w) {
            want[w] = get_word(a.code_hashes + 32ull * i, w);
            empty = empty && want[w] == empty_code_word(w);
        }
        if (!empty) {
            uint32_t slot = ns::home_hash(want[0], want[1], a.salt0, a.salt1) & a.mask;
            for (;;) {
                const uint32_t e = a.table[slot];
                if (e == 0u) {
                    atomicAdd(&a.counters[PRE_CNT_MISSING_CODE], 1u);
                    break;
                }
                const uint32_t* const dg = a.code_dig + 8ull * (e - 1u);
                uint32_t diff = 0;
                for (uint32_t w = 0; w < 8u; ++w) diff |= dg[w] ^ want[w];
                if (diff == 0u) {
                    idx = e - 1u;
                    a.table_used[slot] = 1u;
                    break;
                }
                slot = (slot + 1u) & a.mask;
            }
        }
    }
    a.code_index[i] = idx;
}

__global__ void __launch_bounds__(256) code_unused_kernel(const phant::PrestateArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nc) return;
    if (a.table_used[a.code_slot[k]] == 0u) atomicAdd(&a.counters[PRE_CNT_UNUSED_CODES], 1u);
}

}  // namespace pre

// ---------------------------------------------------------------- host side
static uint32_t grid256(uint32_t n) { return n ? (n + 255u) / 256u : 1u; }

hipError_t launch_prestate_accounts(const PrestateArgs& a, hipStream_t st) {
    if (a.na) hipLaunchKernelGGL(pre::account_decode_kernel, dim3(grid256(a.na)), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_prestate_slots(const PrestateArgs& a, hipStream_t st) {
    if (a.ns) hipLaunchKernelGGL(pre::slot_decode_kernel, dim3(grid256(a.ns)), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_code_hash(const PrestateArgs& a, uint32_t form, hipStream_t st) {
    if (!a.nc) return hipGetLastError();
    if (form == 1u) {
        hipLaunchKernelGGL(pre::code_hash_lane_kernel, dim3(grid256(a.nc)), dim3(256), 0, st, a);
    } else {
        const uint32_t wgs = (a.nc + 7u) / 8u;  // eight codes per workgroup of four waves
        hipLaunchKernelGGL(pre::code_hash_kernel, dim3(wgs), dim3(256), 0, st, a, wgs * 4u <= 1024u);
    }
    return hipGetLastError();
}
hipError_t launch_code_match(const PrestateArgs& a, hipStream_t st) {
    if (a.na) hipLaunchKernelGGL(pre::code_match_kernel, dim3(grid256(a.na)), dim3(256), 0, st, a);
    if (a.nc) hipLaunchKernelGGL(pre::code_unused_kernel, dim3(grid256(a.nc)), dim3(256), 0, st, a);
    return hipGetLastError();
}
uint32_t code_table_slots(uint32_t nc) {  // a power of two, load <= 1/2
    uint32_t t = 64;
    while (t < 2ull * nc && t < (1u << 31)) t <<= 1;
    return t;
}

}  // namespace phant
