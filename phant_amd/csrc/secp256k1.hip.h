// secp256k1.hip.h -- secp256k1 public-key recovery, one signature per lane, for gfx950.
//
// What it computes: src/crypto/ecdsa.zig:19-21 `erecover` (SEC 1 section 4.1.6 over the curve of SEC 2 section 2.4.1) followed
// by src/signer/signer.zig:77-78, address = keccak256(pubkey[1..])[12..].
//
// Plain C++ on 8 x 32-bit little-endian limbs with 64-bit products (v_mad_u64_u32 on the device); no inline assembly and no
// builtin of its own, so that the host build of the test suite compiles this file as it is.  The data is public: nothing here is
// constant-time, and lanes of a wave diverge freely (a failed tuple's lane simply leaves).
//
//   field   mod p = 2^256 - 2^32 - 977.  Elements are always fully reduced (< p): the "is zero" / "is equal" tests of the point
//           addition are then limb comparisons.  mul / sqr accept ANY 256-bit operands; a product's high half is folded in with
//           2^32 + 977 twice, then one conditional subtraction.  Inversion and square root are the powers p - 2 and (p + 1) / 4
//           on the chain x^(2^k - 1), k = 2, 3, 6, 9, 11, 22, 44, 88, 176, 220, 223 (both exponents are 223 ones, a zero, 22 ones
//           and ten / eight low bits): 255 squarings and 15 / 13 multiplications.
//   scalars mod n = 2^256 - c, c < 2^129: a product's high half is folded in with c three times (385 -> 260 -> 257 -> 256 bits).
//           r^-1 is the power n - 2 by plain square-and-multiply (n has no structure to exploit).
//   points  Jacobian (X, Y, Z), infinity = (Z == 0).  jac_add is correct for EVERY pair: either operand at infinity, P + P (it
//           doubles) and P + (-P) (infinity).  None of these is argued away: a crafted (z, r, s) reaches them -- u1 = u2 with
//           R = G makes the very first addition of the ladder P + P (tests/test_gpu_secp.py::test_ladder_corner_cases).
//   ladder  Q = u1 G + u2 R, interleaved, most significant window first: 4 doublings per step, u2 in 4-bit windows against a
//           per-lane table of 1 R .. 15 R (Jacobian, 15 x 96 bytes of the lane's scratch memory: a table a lane indexes with a
//           value of its own cannot live in VGPRs), u1 in 8-bit windows against 1 G .. 255 G (affine, 16 KiB of device memory,
//           computed on the device once per context by secp_gtable_kernel from the generator of SEC 2).
//           = 256 doublings + at most 64 + 13 general / mixed additions with R's multiples + at most 32 mixed additions with G's.
#pragma once
#include "keccak_f1600.hip.h"

namespace phant {
namespace secp {

// status bytes (= PHANT_SIG_* of include/phant_gpu.h)
constexpr uint8_t SIG_OK = 0, SIG_BAD_RANGE = 1, SIG_HIGH_S = 2, SIG_BAD_RECID = 3, SIG_NOT_ON_CURVE = 4, SIG_INFINITY = 5;
constexpr uint32_t RECOVER_LOW_S = 1u;
constexpr uint32_t GTABLE_ENTRIES = 256;  // entry j = j G as x || y, 8 + 8 little-endian limbs (entry 0 unused)

struct U256 {
    uint32_t v[8];  // little-endian limbs
};
struct Jac {
    U256 x, y, z;
};

#define SECP_DEV __device__ inline

SECP_DEV U256 u256_const(uint32_t w7, uint32_t w6, uint32_t w5, uint32_t w4, uint32_t w3, uint32_t w2, uint32_t w1, uint32_t w0) {
    U256 r;  // (written most significant word first, as the standards print them)
    r.v[0] = w0, r.v[1] = w1, r.v[2] = w2, r.v[3] = w3, r.v[4] = w4, r.v[5] = w5, r.v[6] = w6, r.v[7] = w7;
    return r;
}
SECP_DEV U256 const_p() { return u256_const(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFC2Fu); }
SECP_DEV U256 const_n() { return u256_const(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xBAAEDCE6u, 0xAF48A03Bu, 0xBFD25E8Cu, 0xD0364141u); }
SECP_DEV U256 const_half_n() { return u256_const(0x7FFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x5D576E73u, 0x57A4501Du, 0xDFE92F46u, 0x681B20A0u); }
SECP_DEV U256 const_gx() { return u256_const(0x79BE667Eu, 0xF9DCBBACu, 0x55A06295u, 0xCE870B07u, 0x029BFCDBu, 0x2DCE28D9u, 0x59F2815Bu, 0x16F81798u); }
SECP_DEV U256 const_gy() { return u256_const(0x483ADA77u, 0x26A3C465u, 0x5DA4FBFCu, 0x0E1108A8u, 0xFD17B448u, 0xA6855419u, 0x9C47D08Fu, 0xFB10D4B8u); }

SECP_DEV U256 u256_zero() {
    U256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = 0;
    return r;
}
SECP_DEV U256 u256_small(uint32_t w) {
    U256 r = u256_zero();
    r.v[0] = w;
    return r;
}
SECP_DEV bool u256_is_zero(const U256& a) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t |= a.v[i];
    return t == 0;
}
SECP_DEV bool u256_eq(const U256& a, const U256& b) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t |= a.v[i] ^ b.v[i];
    return t == 0;
}
// a >= b
SECP_DEV bool u256_ge(const U256& a, const U256& b) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a.v[i] - b.v[i] - borrow;
        borrow = (d >> 32) & 1u;
    }
    return borrow == 0;
}
// r = a + b, returns the carry out
SECP_DEV uint32_t u256_add(U256& r, const U256& a, const U256& b) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.v[i] + b.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}
// r = a - b, returns the borrow out
SECP_DEV uint32_t u256_sub(U256& r, const U256& a, const U256& b) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a.v[i] - b.v[i] - borrow;
        r.v[i] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
    return (uint32_t)borrow;
}
// t[0..15] = a * b
SECP_DEV void mul256(uint32_t (&t)[16], const U256& a, const U256& b) {
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t acc = (uint64_t)a.v[i] * b.v[j] + t[i + j] + carry;  // (2^32-1)^2 + 2 (2^32-1) = 2^64 - 1
            t[i + j] = (uint32_t)acc;
            carry = acc >> 32;
        }
        t[i + 8] = (uint32_t)carry;
    }
}

// ---------------------------------------------------------------------------------------------------------- field mod p
// a value below 2^256 into [0, p)
SECP_DEV void fe_normalize(U256& r, uint32_t carry) {
    // carry: the value is 2^256 + r, and 2^256 = 2^32 + 977 (mod p); r is then far below p and nothing overflows
    if (carry) {
        uint64_t c = (uint64_t)r.v[0] + 977u;
        r.v[0] = (uint32_t)c;
        c = (c >> 32) + r.v[1] + 1u;
        r.v[1] = (uint32_t)c;
        c >>= 32;
#pragma unroll
        for (int i = 2; i < 8; ++i) {
            c += r.v[i];
            r.v[i] = (uint32_t)c;
            c >>= 32;
        }
    }
    const U256 p = const_p();
    if (u256_ge(r, p)) (void)u256_sub(r, r, p);
}
SECP_DEV U256 fe_reduce512(const uint32_t (&t)[16]) {
    // lo + hi * (2^32 + 977): limb i takes t[i] + 977 t[8 + i] + t[8 + i - 1]
    U256 r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)t[8 + i] * 977u + t[i] + (i ? t[8 + i - 1] : 0u);
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    const uint64_t ov = c + t[15];  // what stands at 2^256: below 2^34
    // ... folded in once more: ov * 977 at limb 0, ov at limb 1
    const uint64_t m = ov * 977u;
    c = (uint64_t)r.v[0] + (uint32_t)m;
    r.v[0] = (uint32_t)c;
    c = (c >> 32) + r.v[1] + (m >> 32) + (uint32_t)ov;
    r.v[1] = (uint32_t)c;
    c = (c >> 32) + r.v[2] + (ov >> 32);
    r.v[2] = (uint32_t)c;
    c >>= 32;
#pragma unroll
    for (int i = 3; i < 8; ++i) {
        c += r.v[i];
        r.v[i] = (uint32_t)c;
        c >>= 32;
    }
    fe_normalize(r, (uint32_t)c);
    return r;
}
SECP_DEV U256 fe_mul(const U256& a, const U256& b) {
    uint32_t t[16];
    mul256(t, a, b);
    return fe_reduce512(t);
}
SECP_DEV U256 fe_sqr(const U256& a) { return fe_mul(a, a); }
// a, b < p
SECP_DEV U256 fe_add(const U256& a, const U256& b) {
    U256 r;
    const uint32_t c = u256_add(r, a, b);
    fe_normalize(r, c);
    return r;
}
SECP_DEV U256 fe_sub(const U256& a, const U256& b) {
    U256 r;
    if (u256_sub(r, a, b)) (void)u256_add(r, r, const_p());
    return r;
}
SECP_DEV U256 fe_neg(const U256& a) { return fe_sub(u256_zero(), a); }
SECP_DEV U256 fe_dbl(const U256& a) { return fe_add(a, a); }
SECP_DEV U256 fe_sqr_n(U256 a, int n) {
    for (int i = 0; i < n; ++i) a = fe_sqr(a);
    return a;
}
// x^(2^223 - 1) and, on the way, x^3 (x2) and x^(2^22 - 1) (x22)
SECP_DEV U256 fe_pow_x223(const U256& x, U256& x2, U256& x22) {
    x2 = fe_mul(fe_sqr(x), x);
    const U256 x3 = fe_mul(fe_sqr(x2), x);
    const U256 x6 = fe_mul(fe_sqr_n(x3, 3), x3);
    const U256 x9 = fe_mul(fe_sqr_n(x6, 3), x3);
    const U256 x11 = fe_mul(fe_sqr_n(x9, 2), x2);
    x22 = fe_mul(fe_sqr_n(x11, 11), x11);
    const U256 x44 = fe_mul(fe_sqr_n(x22, 22), x22);
    const U256 x88 = fe_mul(fe_sqr_n(x44, 44), x44);
    const U256 x176 = fe_mul(fe_sqr_n(x88, 88), x88);
    const U256 x220 = fe_mul(fe_sqr_n(x176, 44), x44);
    return fe_mul(fe_sqr_n(x220, 3), x3);
}
// x^(p - 2): p - 2 = 223 ones, 0, 22 ones, 0000101101   (0 -> 0)
SECP_DEV U256 fe_inv(const U256& x) {
    U256 x2, x22;
    U256 t = fe_pow_x223(x, x2, x22);
    t = fe_mul(fe_sqr_n(t, 23), x22);
    t = fe_mul(fe_sqr_n(t, 5), x);
    t = fe_mul(fe_sqr_n(t, 3), x2);
    return fe_mul(fe_sqr_n(t, 2), x);
}
// x^((p + 1) / 4): (p + 1) / 4 = 223 ones, 0, 22 ones, 00001100; a root of x when x is a square (then returns true)
SECP_DEV bool fe_sqrt(U256& root, const U256& x) {
    U256 x2, x22;
    U256 t = fe_pow_x223(x, x2, x22);
    t = fe_mul(fe_sqr_n(t, 23), x22);
    t = fe_mul(fe_sqr_n(t, 6), x2);
    root = fe_sqr_n(t, 2);
    U256 xr = x;
    fe_normalize(xr, 0);
    return u256_eq(fe_sqr(root), xr);
}

// -------------------------------------------------------------------------------------------------------- scalars mod n
// out[0..LEN) = lo[0..8) + hi[0..NH) * c, c = 2^256 - n (5 limbs)
template <int NH, int LEN>
SECP_DEV void sc_fold(uint32_t (&out)[LEN], const uint32_t* lo, const uint32_t* hi) {
    const uint32_t c[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 0x1u};
#pragma unroll
    for (int i = 0; i < LEN; ++i) out[i] = i < 8 ? lo[i] : 0u;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (i + j < LEN) {
                const uint64_t acc = (uint64_t)hi[i] * c[j] + out[i + j] + carry;
                out[i + j] = (uint32_t)acc;
                carry = acc >> 32;
            }
        }
#pragma unroll
        for (int k = i + 5; k < LEN; ++k) {
            const uint64_t acc = (uint64_t)out[k] + carry;
            out[k] = (uint32_t)acc;
            carry = acc >> 32;
        }
    }
}
SECP_DEV U256 sc_reduce512(const uint32_t (&t)[16]) {
    uint32_t a[13], b[9], d[9], e[9];
    sc_fold<8, 13>(a, t, t + 8);  // < 2^386
    sc_fold<5, 9>(b, a, a + 8);   // < 2^260
    sc_fold<1, 9>(d, b, b + 8);   // < 2^256 + 2^133
    sc_fold<1, 9>(e, d, d + 8);   // d[8] = 1: the low part is below 2^133, and so is what comes out
    U256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = e[i];
    const U256 n = const_n();
    if (u256_ge(r, n)) (void)u256_sub(r, r, n);
    return r;
}
SECP_DEV U256 sc_mul(const U256& a, const U256& b) {
    uint32_t t[16];
    mul256(t, a, b);
    return sc_reduce512(t);
}
// a < n
SECP_DEV U256 sc_neg(const U256& a) {
    U256 r = u256_zero();
    if (!u256_is_zero(a)) (void)u256_sub(r, const_n(), a);
    return r;
}
// a^(n - 2), most significant bit first (0 -> 0)
SECP_DEV U256 sc_inv(const U256& a) {
    U256 e = const_n();
    e.v[0] -= 2u;  // (n ends in ...4141)
    U256 r = u256_small(1u);
    for (int i = 255; i >= 0; --i) {
        r = sc_mul(r, r);
        const uint32_t bit = e.v[7] >> 31;
#pragma unroll
        for (int k = 7; k > 0; --k) e.v[k] = (e.v[k] << 1) | (e.v[k - 1] >> 31);
        e.v[0] <<= 1;
        if (bit) r = sc_mul(r, a);
    }
    return r;
}

// ------------------------------------------------------------------------------------------------------------- points
SECP_DEV Jac jac_infinity() {
    Jac r;
    r.x = u256_small(1u), r.y = u256_small(1u), r.z = u256_zero();
    return r;
}
SECP_DEV bool jac_is_infinity(const Jac& p) { return u256_is_zero(p.z); }
SECP_DEV Jac jac_from_affine(const U256& x, const U256& y) {
    Jac r;
    r.x = x, r.y = y, r.z = u256_small(1u);
    return r;
}
// 2 P (a = 0).  Infinity stays infinity (Z3 = 2 Y Z); the curve has no point with Y = 0.
SECP_DEV Jac jac_double(const Jac& p) {
    const U256 a = fe_sqr(p.x), b = fe_sqr(p.y), c = fe_sqr(b);
    U256 d = fe_sub(fe_sub(fe_sqr(fe_add(p.x, b)), a), c);
    d = fe_dbl(d);
    const U256 e = fe_add(fe_dbl(a), a), f = fe_sqr(e);
    Jac r;
    r.x = fe_sub(f, fe_dbl(d));
    const U256 c8 = fe_dbl(fe_dbl(fe_dbl(c)));
    r.y = fe_sub(fe_mul(e, fe_sub(d, r.x)), c8);
    r.z = fe_dbl(fe_mul(p.y, p.z));
    return r;
}
// P + Q for every pair.  q_affine: Q's Z is 1 (and Q is no infinity): four multiplications and a squaring less.
SECP_DEV Jac jac_add(const Jac& p, const Jac& q, bool q_affine) {
    if (!q_affine && jac_is_infinity(q)) return p;
    if (jac_is_infinity(p)) return q;
    const U256 z1z1 = fe_sqr(p.z);
    U256 u1 = p.x, s1 = p.y, z2z2;
    if (!q_affine) {
        z2z2 = fe_sqr(q.z);
        u1 = fe_mul(p.x, z2z2);
        s1 = fe_mul(p.y, fe_mul(z2z2, q.z));
    }
    const U256 u2 = fe_mul(q.x, z1z1), s2 = fe_mul(q.y, fe_mul(z1z1, p.z));
    const U256 h = fe_sub(u2, u1), rr = fe_sub(s2, s1);
    if (u256_is_zero(h)) {
        if (u256_is_zero(rr)) return jac_double(p);  // the same point
        return jac_infinity();                       // opposite points
    }
    const U256 hh = fe_sqr(h), hhh = fe_mul(hh, h), v = fe_mul(u1, hh);
    Jac r;
    r.x = fe_sub(fe_sub(fe_sqr(rr), hhh), fe_dbl(v));
    r.y = fe_sub(fe_mul(rr, fe_sub(v, r.x)), fe_mul(s1, hhh));
    r.z = fe_mul(h, p.z);
    if (!q_affine) r.z = fe_mul(r.z, q.z);
    return r;
}
// (X / Z^2, Y / Z^3) of a point that is not infinity
SECP_DEV void jac_to_affine(const Jac& p, U256& x, U256& y) {
    const U256 zi = fe_inv(p.z), zi2 = fe_sqr(zi);
    x = fe_mul(p.x, zi2);
    y = fe_mul(p.y, fe_mul(zi2, zi));
}

// ------------------------------------------------------------------------------------------------------ bytes and hashes
SECP_DEV U256 load_be32(const uint8_t* __restrict__ p) {  // 32 big-endian bytes, any alignment
    U256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = p + 4 * (7 - i);
        r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    return r;
}
SECP_DEV void store_be32(uint8_t* __restrict__ p, const U256& a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint8_t* q = p + 4 * (7 - i);
        q[0] = (uint8_t)(a.v[i] >> 24), q[1] = (uint8_t)(a.v[i] >> 16), q[2] = (uint8_t)(a.v[i] >> 8), q[3] = (uint8_t)a.v[i];
    }
}
SECP_DEV uint32_t bswap32(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }
// keccak256(x || y) of a public key whose coordinates are in registers; the address is digest bytes 12..31
SECP_DEV void pubkey_digest(Sponge& s, const U256& x, const U256& y) {
    sponge_zero(s);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // message dword j = the byte-swapped limb 7 - j
        s.lo[i] = bswap32(x.v[7 - 2 * i]);
        s.hi[i] = bswap32(x.v[6 - 2 * i]);
        s.lo[4 + i] = bswap32(y.v[7 - 2 * i]);
        s.hi[4 + i] = bswap32(y.v[6 - 2 * i]);
    }
    s.lo[8] = 0x01u;         // pad: byte 64 ...
    s.hi[16] = 0x80000000u;  // ... byte 135
    keccak_f1600(s);
}

// -------------------------------------------------------------------------------------------------------- the recovery
// SEC 1 section 4.1.6 for one (z, r, s, recid), the checks in the order include/phant_gpu.h states.  qx, qy: the public key.
SECP_DEV uint8_t recover(const U256& z, const U256& r, const U256& s, uint32_t recid, uint32_t flags,
                         const uint32_t* __restrict__ gtable, U256& qx, U256& qy) {
    if (recid > 3u) return SIG_BAD_RECID;
    const U256 n = const_n(), p = const_p();
    if (u256_is_zero(r) || u256_ge(r, n) || u256_is_zero(s) || u256_ge(s, n)) return SIG_BAD_RANGE;
    if ((flags & RECOVER_LOW_S) && !u256_ge(const_half_n(), s)) return SIG_HIGH_S;
    U256 x = r;
    if (recid & 2u) {
        if (u256_add(x, r, n)) return SIG_BAD_RECID;  // beyond 2^256
    }
    if (u256_ge(x, p)) return SIG_BAD_RECID;
    U256 y;
    const U256 rhs = fe_add(fe_mul(fe_sqr(x), x), u256_small(7u));
    if (!fe_sqrt(y, rhs)) return SIG_NOT_ON_CURVE;
    if ((y.v[0] & 1u) != (recid & 1u)) y = fe_neg(y);

    U256 zr = z;  // z mod n (z < 2^256 < 2 n)
    if (u256_ge(zr, n)) (void)u256_sub(zr, zr, n);
    const U256 ri = sc_inv(r);
    U256 u1 = sc_neg(sc_mul(zr, ri)), u2 = sc_mul(s, ri);

    // 1 R .. 15 R
    Jac tab[15];
    const Jac rp = jac_from_affine(x, y);
    tab[0] = rp;
    tab[1] = jac_double(rp);
    for (int k = 2; k < 15; ++k) tab[k] = jac_add(tab[k - 1], rp, true);

    Jac acc = jac_infinity();
    for (int step = 63; step >= 0; --step) {
        for (int d = 0; d < 4; ++d) acc = jac_double(acc);
        const uint32_t w2 = u2.v[7] >> 28;
#pragma unroll
        for (int k = 7; k > 0; --k) u2.v[k] = (u2.v[k] << 4) | (u2.v[k - 1] >> 28);
        u2.v[0] <<= 4;
        if (w2) acc = jac_add(acc, tab[w2 - 1], false);
        if ((step & 1) == 0) {  // the low nibble of a byte of u1: its 8-bit window
            const uint32_t w1 = u1.v[7] >> 24;
#pragma unroll
            for (int k = 7; k > 0; --k) u1.v[k] = (u1.v[k] << 8) | (u1.v[k - 1] >> 24);
            u1.v[0] <<= 8;
            if (w1) {
                Jac g;
                const uint32_t* e = gtable + 16u * w1;
#pragma unroll
                for (int i = 0; i < 8; ++i) g.x.v[i] = e[i], g.y.v[i] = e[8 + i];
                g.z = u256_small(1u);
                acc = jac_add(acc, g, true);
            }
        }
    }
    if (jac_is_infinity(acc)) return SIG_INFINITY;
    jac_to_affine(acc, qx, qy);
    return SIG_OK;
}

}  // namespace secp
}  // namespace phant
