// rlp.h -- RLP's rules (Yellow Paper, appendix B), stated ONCE for every kernel and all host code under csrc/:
//   a single byte below 0x80 is its own encoding;
//   a string of up to 55 bytes: 0x80 + len, then the bytes;   longer: 0xb7 + (bytes of len), len big-endian, the bytes;
//   a list whose payload is up to 55 bytes: 0xc0 + len;        longer: 0xf7 + (bytes of len), len big-endian;
//   a length has no leading zero, and the long form is refused where the short one would do;
//   an integer is the string of its big-endian bytes without leading zeros (zero: the empty string).
// Three tuned forms stay with their callers and say so there: trie_build.hip's put_str_wide (its dword payload copy),
// state_root.hip's be_len32 (dword loads of an aligned value) and transactions.hip.h's auth_message_byte (byte j of an
// encoding that is never written).
//
// Plain C++ that needs <stdint.h> and <stddef.h> only: the same text is compiled for the device, for the host emulation of
// the kernels (tests/emu.py) and by a bare g++ for the stand-alone programs under tests/native/.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The one function qualifier.  In a HIP compilation (the compiler itself defines __host__ and __device__ there, whatever was
// included before this file) the inlining is forced: the hot callers are __forceinline__ themselves.
#if defined(__HIP__)
#define PHANT_RLP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PHANT_RLP_FN inline
#endif

namespace phant {

// ---- sizes
// significant bytes of v (0 for zero)
PHANT_RLP_FN uint32_t uint_bytes(uint64_t v) {
    uint32_t n = 0;
    while (v) {
        ++n;
        v >>= 8;
    }
    return n;
}
// significant bytes of the n-byte big-endian value at be (0 for zero): byte by byte, no alignment asked
PHANT_RLP_FN uint32_t be_bytes(const uint8_t* be, uint32_t n) {
    uint32_t nb = 0;
    for (uint32_t k = 0; k < n; ++k)  // (no early exit: with a constant n the loads are independent of each other)
        if (nb == 0u && be[k] != 0u) nb = n - k;
    return nb;
}
// bytes of the header in front of a payload (string or list)
PHANT_RLP_FN uint32_t hdr_len(uint64_t payload) { return payload <= 55 ? 1u : 1u + uint_bytes(payload); }
// bytes of an encoded unsigned integer
PHANT_RLP_FN uint32_t uint_len(uint64_t v) { return v < 0x80u ? 1u : 1u + uint_bytes(v); }
// bytes of an encoded string of `len` bytes whose first byte is `first` (looked at only when len == 1)
PHANT_RLP_FN uint64_t str_len(uint64_t len, uint32_t first) {
    if (len == 1 && first < 0x80u) return 1;
    return hdr_len(len) + len;
}

// ---- writers: each returns the bytes it wrote
// the header of a string (base 0x80) or of a list (base 0xc0) with `payload` bytes: at most 9 bytes
PHANT_RLP_FN uint32_t put_hdr(uint8_t* o, uint32_t base, uint64_t payload) {
    if (payload <= 55) {
        o[0] = (uint8_t)(base + payload);
        return 1u;
    }
    const uint32_t ll = uint_bytes(payload);
    *o++ = (uint8_t)(base + 55u + ll);
    for (int s = 8 * ((int)ll - 1); s >= 0; s -= 8) *o++ = (uint8_t)(payload >> s);
    return 1u + ll;
}
// The same header -> the byte behind it, for the trie builder's node writers, which carry one output pointer through a node.  It
// has a body of its own because neither form compiles well from the other: w + put_hdr(w, ..) costs the builder's leaf kernels 3 %
// more instructions, put_hdr_to(o, ..) - o the post-state's node writers as much.  tests/native/rlp_main.cpp holds the two
// against each other.
PHANT_RLP_FN uint8_t* put_hdr_to(uint8_t* w, uint32_t base, uint64_t payload) {
    if (payload <= 55) {
        *w++ = (uint8_t)(base + payload);
        return w;
    }
    const uint32_t ll = uint_bytes(payload);
    *w++ = (uint8_t)(base + 55u + ll);
    for (int s = 8 * ((int)ll - 1); s >= 0; s -= 8) *w++ = (uint8_t)(payload >> s);
    return w;
}
// an unsigned integer: at most 9 bytes
PHANT_RLP_FN uint32_t put_uint(uint8_t* o, uint64_t v) {
    if (v != 0u && v < 0x80u) {
        o[0] = (uint8_t)v;
        return 1u;
    }
    const uint32_t nb = uint_bytes(v);
    o[0] = (uint8_t)(0x80u + nb);
    for (uint32_t k = 0; k < nb; ++k) o[1u + k] = (uint8_t)(v >> (8u * (nb - 1u - k)));
    return 1u + nb;
}
// the string s[0, len), copied byte by byte (no alignment asked of either side)
PHANT_RLP_FN uint32_t put_str(uint8_t* o, const uint8_t* s, uint32_t len) {
    if (len == 1u && s[0] < 0x80u) {
        o[0] = s[0];
        return 1u;
    }
    const uint32_t h = put_hdr(o, 0x80u, len);
    for (uint32_t t = 0; t < len; ++t) o[h + t] = s[t];
    return h + len;
}
// the integer whose n big-endian bytes (leading zeros allowed) lie at be
PHANT_RLP_FN uint32_t put_minimal(uint8_t* o, const uint8_t* be, uint32_t n) {
    const uint32_t nb = be_bytes(be, n);
    return put_str(o, be + (n - nb), nb);
}

// ---- reader
// Where a decoded item lies.  Off: uint32_t in kernels (a node, a transaction: shorter than 4 GiB), size_t on the host.
template <class Off>
struct RlpItemOf {
    typedef Off off;
    Off pay;    // payload offset, counted from where the caller's offsets count from
    Off len;    // payload length
    Off total;  // header + payload
    uint32_t is_list;
};
typedef RlpItemOf<uint32_t> RlpItem;

// plain memory as a byte source
struct MemBytes {
    const uint8_t* p;
    PHANT_RLP_FN uint32_t byte(size_t o) const { return p[o]; }
};

// One canonical RLP item at offset `at` of the byte source `nd` (anything with byte(offset)) with `avail` bytes left; false:
// it is cut short or not canonical.  No byte at or behind at + avail is read, and every declared length is compared with
// what is left before it is added to anything (it can be 2^64 - 1).
template <class Bytes, class Off>
PHANT_RLP_FN bool rlp_decode(const Bytes& nd, typename RlpItemOf<Off>::off at, typename RlpItemOf<Off>::off avail, RlpItemOf<Off>& it) {
    if (avail == 0) return false;
    const uint32_t b = nd.byte(at);
    if (b < 0x80u) {
        it.pay = at;
        it.len = 1;
        it.total = 1;
        it.is_list = 0;
        return true;
    }
    if (b <= 0xb7u || (b >= 0xc0u && b <= 0xf7u)) {
        const uint32_t list = b >= 0xc0u;
        const uint32_t len = b - (list ? 0xc0u : 0x80u);
        if (1u + len > avail) return false;
        if (!list && len == 1u && nd.byte(at + 1) < 0x80u) return false;
        it.pay = at + 1;
        it.len = len;
        it.total = 1u + len;
        it.is_list = list;
        return true;
    }
    const uint32_t list = b >= 0xf8u;
    const uint32_t ll = b - (list ? 0xf7u : 0xb7u);  // 1..8
    if (1u + ll > avail) return false;
    if (nd.byte(at + 1) == 0) return false;  // leading zero in the length
    uint64_t len = 0;
    for (uint32_t i = 0; i < ll; ++i) len = (len << 8) | nd.byte(at + 1 + i);
    if (len <= 55) return false;  // short form was mandatory
    const uint32_t hdr = 1u + ll;
    if (len > (uint64_t)(avail - hdr)) return false;
    it.pay = at + hdr;
    it.len = (Off)len;
    it.total = hdr + (Off)len;
    it.is_list = list;
    return true;
}

}  // namespace phant
