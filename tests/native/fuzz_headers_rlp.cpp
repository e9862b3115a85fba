// fuzz_headers_rlp.cpp -- memory safety and strictness of the host side of phant_headers_decode_rlp (phant_amd/csrc/host_rlp.cpp:
// header_decode): every truncation and every single-byte replacement (all 256 values at every position) of each seed header, each
// in an allocation of exactly its size so that AddressSanitizer sees one byte too far.  Every input is either refused -- its row
// zeroed, its n_fields 0 -- or re-encodes to itself: the encoder below is a plain restatement of src/types/block.zig:51-69 over
// the decoded fields.  Built by tests/test_headers_rlp_native.py with g++ -fsanitize=address,undefined.  Input file: records
// "len(4 LE) bytes"; prints how many variants decoded and a checksum of what they produced.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../include/phant_gpu.h"
#include "../../phant_amd/csrc/host_rlp.h"

static uint64_t ok = 0, refused = 0, sum = 0;

static void put_str(std::vector<uint8_t>& o, const uint8_t* p, size_t n) {
    if (n == 1 && p[0] < 0x80) return o.push_back(p[0]);
    if (n < 56) o.push_back((uint8_t)(0x80 + n));
    else {
        uint8_t be[8];
        size_t ll = 0;
        for (size_t l = n; l; l >>= 8) be[ll++] = (uint8_t)l;
        o.push_back((uint8_t)(0xb7 + ll));
        for (size_t q = 0; q < ll; ++q) o.push_back(be[ll - 1 - q]);
    }
    o.insert(o.end(), p, p + n);
}
static void put_be(std::vector<uint8_t>& o, const uint8_t* be, size_t width) {  // a minimal integer out of `width` big-endian bytes
    size_t z = 0;
    while (z < width && be[z] == 0) ++z;
    put_str(o, be + z, width - z);
}
static void put_u64(std::vector<uint8_t>& o, uint64_t v) {
    uint8_t be[8];
    for (int k = 0; k < 8; ++k) be[k] = (uint8_t)(v >> (8 * (7 - k)));
    put_be(o, be, 8);
}

struct Row {  // one header's worth of every array, each in an allocation of its own
    std::vector<uint8_t> h32[9], addr, bloom, nonce, fee, extra, n_fields;
    std::vector<uint64_t> ints[7];
    std::vector<uint32_t> extra_off;
    explicit Row(size_t extra_cap) : addr(20, 0xEE), bloom(256, 0xEE), nonce(8, 0xEE), fee(32, 0xEE), extra(extra_cap ? extra_cap : 1, 0xEE), n_fields(1, 0xEE), extra_off(2, 0) {
        for (auto& v : h32) v.assign(32, 0xEE);
        for (auto& v : ints) v.assign(1, 0xEEEEEEEEEEEEEEEEull);
    }
    phant::HeaderArrays arrays() {
        return phant::HeaderArrays{h32[0].data(), h32[1].data(), addr.data(), h32[2].data(), h32[3].data(), h32[4].data(), bloom.data(),
                                   ints[0].data(), ints[1].data(), ints[2].data(), ints[3].data(), ints[4].data(), extra.data(), extra_off.data(),
                                   h32[5].data(), nonce.data(), fee.data(), h32[6].data(), ints[5].data(), ints[6].data(), h32[7].data(),
                                   h32[8].data(), n_fields.data()};
    }
    std::vector<uint8_t> encode() const {
        std::vector<uint8_t> p;
        const unsigned nf = n_fields[0];
        for (int k : {0, 1}) put_str(p, h32[k].data(), 32);
        put_str(p, addr.data(), 20);
        for (int k : {2, 3, 4}) put_str(p, h32[k].data(), 32);
        put_str(p, bloom.data(), 256);
        for (int k = 0; k < 5; ++k) put_u64(p, ints[k][0]);
        put_str(p, extra.data(), extra_off[1]);
        put_str(p, h32[5].data(), 32);
        put_str(p, nonce.data(), 8);
        if (nf >= 16) put_be(p, fee.data(), 32);
        if (nf >= 17) put_str(p, h32[6].data(), 32);
        if (nf >= 19) put_u64(p, ints[5][0]), put_u64(p, ints[6][0]);
        if (nf >= 20) put_str(p, h32[7].data(), 32);
        if (nf >= 21) put_str(p, h32[8].data(), 32);
        std::vector<uint8_t> out;
        uint8_t be[8];
        size_t ll = 0;
        for (size_t l = p.size(); l; l >>= 8) be[ll++] = (uint8_t)l;
        if (p.size() < 56) out.push_back((uint8_t)(0xc0 + p.size()));
        else {
            out.push_back((uint8_t)(0xf7 + ll));
            for (size_t q = 0; q < ll; ++q) out.push_back(be[ll - 1 - q]);
        }
        out.insert(out.end(), p.begin(), p.end());
        return out;
    }
};

static void feed(const uint8_t* src, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(exact.get(), src, len);
    Row row(len);
    uint32_t extra_at = 0;
    const bool good = phant::header_decode(src ? exact.get() : nullptr, len, false, row.arrays(), 0, &extra_at);
    if (good) {
        ++ok;
        const unsigned nf = row.n_fields[0];
        if (nf != 15 && nf != 16 && nf != 17 && nf != 19 && nf != 20 && nf != 21) std::abort();
        if (extra_at != row.extra_off[1] || extra_at > len) std::abort();
        const std::vector<uint8_t> again = row.encode();
        if (again.size() != len || std::memcmp(again.data(), exact.get(), len) != 0) std::abort();  // encode(decode(x)) == x
        for (uint8_t b : again) sum = sum * 31 + b;
    } else {
        ++refused;
        if (row.n_fields[0] != 0 || extra_at != 0 || row.extra_off[1] != 0) std::abort();  // a refused item cannot be passed on
        for (const auto& v : row.h32)
            for (uint8_t b : v)
                if (b) std::abort();
        for (const auto& v : row.ints)
            if (v[0]) std::abort();
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t seeds = 0;
    for (size_t at = 0; at + 4 <= blob.size();) {
        uint32_t n;
        std::memcpy(&n, blob.data() + at, 4);
        at += 4;
        if (at + n > blob.size()) return 3;
        std::vector<uint8_t> h(blob.begin() + at, blob.begin() + at + n);
        at += n;
        ++seeds;
        const uint64_t before = ok;
        feed(h.data(), h.size());
        if (ok != before + 1) {
            std::printf("seed %zu does not decode\n", seeds);
            return 4;
        }
        for (size_t cut = 0; cut < h.size(); ++cut) feed(h.data(), cut);
        for (size_t pos = 0; pos < h.size(); ++pos) {
            const uint8_t keep = h[pos];
            for (int v = 0; v < 256; ++v) {
                if (v == keep) continue;
                h[pos] = (uint8_t)v;
                feed(h.data(), h.size());
            }
            h[pos] = keep;
        }
        feed(nullptr, 0);
    }
    std::printf("%zu seeds: %llu decoded, %llu refused, checksum %llx\n", seeds, (unsigned long long)ok, (unsigned long long)refused,
                (unsigned long long)sum);
    return 0;
}
