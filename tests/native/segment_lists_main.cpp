// segment_lists_main.cpp -- TEST INFRASTRUCTURE: the trie-order functions of phant_amd/csrc/segment_lists.hip.h as a stand-alone host
// program over the emulated runtime's header (tests/native/shim); tests/test_segment_lists_native.py builds it with g++ under
// AddressSanitizer + UBSan and runs it as a child process.  For every list length n in 0 .. 0x102 and for 0xffff, 0x10000, 0x10001:
//   pos_of_index and index_of_pos are inverse permutations of 0 .. n - 1;
//   positions 0 .. n - 1 visit the indices in the bytewise order of their keys rlp(index), which this file encodes itself;
//   key_bytes_before(p) is the summed length of those keys over the positions below p, for every p <= n.
// Then key_bytes_before on each side of 0x1000000, where the keys grow to five bytes, against the count of keys of every length.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phant_amd/csrc/segment_lists.hip.h"

using namespace phant;

#define CHECK(cond, n, at)                                                                                     \
    do {                                                                                                       \
        if (!(cond)) {                                                                                         \
            std::fprintf(stderr, "%s:%d: %s (n = %u, at %u)\n", __FILE__, __LINE__, #cond, (unsigned)(n), (unsigned)(at)); \
            std::exit(1);                                                                                      \
        }                                                                                                      \
    } while (0)

// rlp(v) from the definition: a single byte 0x01 .. 0x7f is itself; otherwise 0x80 + the count of the big-endian bytes without leading
// zeros, then those bytes (zero: 0x80 alone)
static std::vector<uint8_t> key_of(uint32_t v) {
    if (v != 0u && v < 0x80u) return {(uint8_t)v};
    std::vector<uint8_t> be;
    for (; v; v >>= 8) be.insert(be.begin(), (uint8_t)v);
    be.insert(be.begin(), (uint8_t)(0x80u + be.size()));
    return be;
}

static void check_length(uint32_t n) {
    std::vector<std::vector<uint8_t>> key(n);
    std::vector<uint32_t> sorted(n), seen(n, 0u);
    for (uint32_t i = 0; i < n; ++i) key[i] = key_of(i), sorted[i] = i;
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });  // (vector's <: bytewise)
    uint64_t bytes = 0;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t i = seg::index_of_pos(p, n);
        CHECK(i < n, n, p);
        CHECK(seen[i]++ == 0u, n, p);
        CHECK(seg::pos_of_index(i, n) == p, n, p);
        CHECK(i == sorted[p], n, p);
        CHECK(seg::key_bytes_before(p) == bytes, n, p);
        bytes += key[i].size();
    }
    CHECK(seg::key_bytes_before(n) == bytes, n, n);
    for (uint32_t i = 0; i < n; ++i) CHECK(seg::pos_of_index(i, n) < n && seg::index_of_pos(seg::pos_of_index(i, n), n) == i, n, i);
}

// the keys of the positions below p >= 0x80 are those of the indices below p: 0x80 of one byte, then L bytes for an index of L - 1 bytes
static uint32_t closed_form(uint32_t p) {
    uint64_t bytes = 0x80u;
    for (uint32_t nb = 1; nb <= 4u; ++nb) {
        const uint64_t lo = nb == 1u ? 0x80u : 1ull << (8u * (nb - 1u)), hi = std::min<uint64_t>(p, 1ull << (8u * nb));
        if (hi > lo) bytes += (1u + nb) * (hi - lo);
    }
    return (uint32_t)bytes;  // (modulo 2^32, as the scanned lengths are)
}

int main() {
    uint32_t lengths = 0;
    for (uint32_t n = 0; n <= 0x102u; ++n, ++lengths) check_length(n);
    for (uint32_t n : {0xffffu, 0x10000u, 0x10001u}) check_length(n), ++lengths;
    uint32_t points = 0;
    for (uint32_t p : {0x80u, 0x81u, 0x100u, 0x101u, 0x10000u, 0x10001u, 0xffffffu, 0x1000000u, 0x1000001u, 0x1000002u, 0x7ffffffeu}) {
        CHECK(seg::key_bytes_before(p) == closed_form(p), 0, p);
        ++points;
    }
    CHECK(seg::key_bytes_before(0x1000001u) - seg::key_bytes_before(0x1000000u) == 5u, 0, 0x1000000u);
    CHECK(seg::key_bytes_before(0x1000000u) - seg::key_bytes_before(0xffffffu) == 4u, 0, 0xffffffu);
    std::printf("%u lengths, %u points\n", lengths, points);
    return 0;
}
