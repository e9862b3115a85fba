// sha256.hip.h -- FIPS 180-4 SHA-256, one message per lane: the execution layer's second hash function, which
// EIP-7685 commits a block's requests with (requests.hip.h) and phant_sha256_batch offers on its own.
//
// The eight state words and a rolling window of 16 schedule words stay in VGPRs; the 64 rounds are fully unrolled, so every index into
// the window is a compile-time constant and nothing goes to scratch.  As in keccak_f1600.hip.h every step is written with the
// instruction gfx950 has for it, through the builtins hipcc does not form from plain C:
//   rotr(x, r)            v_alignbit_b32(x, x, r)
//   Sigma0/1, sigma0/1    v_bitop3_b32 0x96 (the three-input XOR) over the rotated and shifted terms
//   Ch(e, f, g)           v_bitop3_b32 0xCA: (e & f) ^ (~e & g) = e ? f : g.  Truth-table bit (e*4 + f*2 + g): e = 0 copies g (bits 1 and 3),
//                         e = 1 copies f (bits 6 and 7) -> 0b11001010
//   Maj(a, b, c)          v_bitop3_b32 0xE8: set where at least two inputs are (bits 3, 5, 6, 7) -> 0b11101000
//   big-endian words      __builtin_bswap32 of little-endian loads (v_perm_b32)
// A round is 2 alignbit-triples + 2 bitop3 for the Sigmas, Ch, Maj and 7 adds; a schedule word 2 alignbit pairs + 2 shifts + 2 bitop3 + 3
// adds: about 2.1k VALU operations a 64-byte block.
#pragma once
#include "absorb.hip.h"

namespace phant {
namespace sha {

__constant__ uint32_t SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
    0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
    0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
    0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
    0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
    0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

PHANT_DEV uint32_t rotr(uint32_t x, uint32_t r) { return alignbit(x, x, r); }
PHANT_DEV uint32_t big_sigma0(uint32_t x) { return xor3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
PHANT_DEV uint32_t big_sigma1(uint32_t x) { return xor3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
PHANT_DEV uint32_t small_sigma0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
PHANT_DEV uint32_t small_sigma1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }
PHANT_DEV uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }
PHANT_DEV uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }

PHANT_DEV void init(uint32_t (&h)[8]) {
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
}

// one block: w = its 16 big-endian words (used up as the rolling window)
PHANT_DEV void compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = h[i];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        if (t >= 16) w[t & 15] += small_sigma1(w[(t - 2) & 15]) + w[(t - 7) & 15] + small_sigma0(w[(t - 15) & 15]);
        // the state is renamed, not moved: round t's a .. h are s[(0 - t) & 7] .. s[(7 - t) & 7]
        uint32_t &a = s[(0 - t) & 7], &b = s[(1 - t) & 7], &c = s[(2 - t) & 7], &d = s[(3 - t) & 7];
        uint32_t &e = s[(4 - t) & 7], &f = s[(5 - t) & 7], &g = s[(6 - t) & 7], &hh = s[(7 - t) & 7];
        const uint32_t t1 = hh + big_sigma1(e) + ch(e, f, g) + SHA256_K[t] + w[t & 15];
        const uint32_t t2 = big_sigma0(a) + maj(a, b, c);
        d += t1;
        hh = t1 + t2;  // (next round's a)
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] += s[i];
}

struct __attribute__((packed, aligned(1))) PackedU32 { uint32_t x; };

// The digest of [prefix_byte, when prefix_present] ++ p[0 .. len): out = the eight state words (word i = digest bytes 4i .. 4i + 3, big
// endian).  p has any alignment.  Nothing in front of p and nothing at or behind safe_end is read; safe_end >= p + len says how far a
// 16-byte load of the last block's window may run past the message.  The bit length is the 64-bit count of all bytes, the prefix
// included.
PHANT_DEV void sha256_stream(bool prefix_present, uint32_t prefix_byte, const uint8_t* __restrict__ p, uint64_t len, const uint8_t* __restrict__ safe_end,
                             uint32_t (&out)[8]) {
    const uint32_t pre = prefix_present ? 1u : 0u;
    const uint64_t total = len + pre, n_blocks = (total + 9u + 63u) / 64u;
    init(out);
    for (uint64_t k = 0; k < n_blocks; ++k) {
        const uint64_t done = 64u * k;
        // r: message bytes in this block -- 64 (a full one), 0 .. 63 (the pad byte follows them), -1 (the pad byte went into the block before)
        const int32_t r = done > total ? -1 : total - done >= 64u ? 64 : (int32_t)(total - done);
        const uint8_t* const q = p + done - pre;  // where the block's window lies: one in front of p for the first block behind a prefix
        const bool shifted = pre != 0u && k == 0u;
        uint32_t w[16];
        if (r > 0 && !shifted && (r == 64 || q + 64 <= safe_end)) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const PackedU32x4 v = *reinterpret_cast<const PackedU32x4*>(q + 16 * c);
                w[4 * c] = __builtin_bswap32(v.x), w[4 * c + 1] = __builtin_bswap32(v.y);
                w[4 * c + 2] = __builtin_bswap32(v.z), w[4 * c + 3] = __builtin_bswap32(v.w);
            }
        } else {  // whole words inside the message by one load each, the others by their bytes
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = r - 4 * j;  // message bytes from this word on
                uint32_t v = 0;
                if (m >= 4 && !(shifted && j == 0)) {
                    v = __builtin_bswap32(reinterpret_cast<const PackedU32*>(q + 4 * j)->x);
                } else if (m > 0) {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (b < m) v |= (shifted && j == 0 && b == 0 ? prefix_byte & 0xffu : (uint32_t)q[4 * j + b]) << (24 - 8 * b);
                }
                w[j] = v;
            }
        }
        if (r < 64) {  // what is behind the message: 0x80, zeros, and in the last block the length
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = r - 4 * j;
                const uint32_t keep = m >= 4 ? 0xffffffffu : m <= 0 ? 0u : ~(0xffffffffu >> (8 * (m & 3)));
                const uint32_t pad = m >= 0 && m < 4 ? 0x80000000u >> (8 * (m & 3)) : 0u;
                w[j] = (w[j] & keep) | pad;
            }
            if (k + 1u == n_blocks) w[14] = (uint32_t)(total >> 29), w[15] = (uint32_t)(total << 3);
        }
        compress(out, w);
    }
}

// the digest's 32 bytes at any address
PHANT_DEV void store_bytes(const uint32_t (&h)[8], uint8_t* __restrict__ out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<PackedU32*>(out + 4 * i)->x = __builtin_bswap32(h[i]);
}

}  // namespace sha
}  // namespace phant
