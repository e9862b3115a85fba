// tx_decode_main.cpp -- the device decode of a transaction (phant_amd/csrc/transactions.hip.h: tx::decode, compiled here for the
// host with PHANT_TX_DECODE_ONLY) against the host decode phant_tx_senders uses (phant_amd/csrc/host_rlp.cpp: tx_signing_parts):
// every truncation, every single-byte replacement by each of ten values, an appended byte and a length field of 2^64 - 1 at
// every item of each seed transaction, for four chain ids, each variant in an allocation of exactly its size so that
// AddressSanitizer sees one byte too far.  The two must agree on the verdict, r, s, recid and, byte for byte, on the signing
// preimage the plan describes.  Built by tests/test_tx_decode_native.py with g++ -fsanitize=address,undefined.  Input file:
// records "len(4 LE) bytes"; prints how many variants decoded.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../include/phant_gpu.h"
#include "../../phant_amd/csrc/host_rlp.h"
#define PHANT_TX_DECODE_ONLY
#include "../../phant_amd/csrc/transactions.hip.h"

static uint64_t ok = 0, bad_tx = 0, bad_v = 0;

static bool feed(const uint8_t* src, size_t len, uint64_t chain_id) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(exact.get(), src, len);
    const uint8_t* p = exact.get();
    std::vector<uint8_t> pre;
    uint8_t r[32] = {0}, s[32] = {0}, recid = 0;
    const uint8_t want = phant::tx_signing_parts(p, len, chain_id, pre, r, s, &recid);
    phant::tx::Decoded d;
    phant::tx::decode(p, (uint32_t)len, chain_id, d);
    if (d.status != want) return std::printf("verdict %u, the host's %u\n", d.status, want), false;
    ++(want == PHANT_SIG_OK ? ok : want == PHANT_SIG_BAD_TX ? bad_tx : bad_v);
    if (want != PHANT_SIG_OK) return true;
    std::vector<uint8_t> mine(d.prefix, d.prefix + d.prefix_len);
    if (d.body_begin > d.body_end || d.body_end > len || d.prefix_len > 10 || d.suffix_len > 11) return std::printf("plan out of range\n"), false;
    mine.insert(mine.end(), p + d.body_begin, p + d.body_end);
    mine.insert(mine.end(), d.suffix, d.suffix + d.suffix_len);
    if (mine != pre) return std::printf("preimage differs\n"), false;
    uint8_t r2[32] = {0}, s2[32] = {0};
    if (d.r.len > 32 || d.s.len > 32 || (size_t)d.r.at + d.r.len > len || (size_t)d.s.at + d.s.len > len) return std::printf("r / s out of range\n"), false;
    std::memcpy(r2 + 32 - d.r.len, p + d.r.at, d.r.len);
    std::memcpy(s2 + 32 - d.s.len, p + d.s.at, d.s.len);
    if (std::memcmp(r, r2, 32) || std::memcmp(s, s2, 32) || recid != d.recid) return std::printf("signature differs\n"), false;
    if ((size_t)d.data.at + d.data.len > len || (size_t)d.al.at + d.al.len > len || (d.to.len != 0 && d.to.len != 20)) return std::printf("span out of range\n"), false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    static const uint8_t values[10] = {0x00, 0x7f, 0x80, 0xb7, 0xb8, 0xbf, 0xc0, 0xf7, 0xf8, 0xff};
    static const uint64_t chains[4] = {1, 127, 128, ~0ull};
    size_t seeds = 0;
    for (size_t at = 0; at + 12 <= blob.size();) {
        uint32_t n;
        uint64_t chain_id;
        std::memcpy(&n, blob.data() + at, 4);
        std::memcpy(&chain_id, blob.data() + at + 4, 8);
        at += 12;
        if (at + n > blob.size()) return 3;
        std::vector<uint8_t> tx(blob.begin() + at, blob.begin() + at + n);
        at += n;
        ++seeds;
        const uint64_t before = ok;
        if (!feed(tx.data(), tx.size(), chain_id) || ok != before + 1) return std::printf("seed %zu does not decode\n", seeds), 4;
        bool good = true;
        for (uint64_t cid : chains) good = good && feed(tx.data(), tx.size(), cid);
        for (size_t cut = 0; cut < tx.size() && good; ++cut) good = feed(tx.data(), cut, chain_id);
        for (size_t pos = 0; pos < tx.size() && good; ++pos) {
            const uint8_t keep = tx[pos];
            for (uint8_t v : values) {
                if (v == keep) continue;
                tx[pos] = v;
                good = good && feed(tx.data(), tx.size(), chain_id);
            }
            tx[pos] = keep;
            // a length field of 2^64 - 1 from here on, as a string's and as a list's
            for (uint8_t head : {(uint8_t)0xbf, (uint8_t)0xff}) {
                std::vector<uint8_t> huge(tx.begin(), tx.begin() + pos);
                huge.push_back(head);
                huge.insert(huge.end(), 8, (uint8_t)0xff);
                huge.insert(huge.end(), tx.begin() + pos, tx.end());
                good = good && feed(huge.data(), huge.size(), chain_id);
            }
        }
        tx.push_back(0);
        good = good && feed(tx.data(), tx.size(), chain_id);
        if (!good) return std::printf("seed %zu\n", seeds), 5;
    }
    std::printf("%zu seeds: %llu decoded, %llu BAD_TX, %llu BAD_V\n", seeds, (unsigned long long)ok, (unsigned long long)bad_tx, (unsigned long long)bad_v);
    return 0;
}
