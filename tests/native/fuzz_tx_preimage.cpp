// fuzz_tx_preimage.cpp -- memory safety of the host side of phant_tx_senders (phant_amd/csrc/host_rlp.cpp: tx_signing_parts,
// the strict transaction decode and the preimage splice): every truncation and every single-byte replacement (all 256 values at
// every position) of each seed transaction, each in an allocation of exactly its size so that AddressSanitizer sees one byte
// too far.  Built by tests/test_tx_preimage_native.py with g++ -fsanitize=address,undefined.  Input file: records
// "len(4 LE) bytes"; prints how many variants decoded and a checksum of what they produced.
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

static uint64_t ok = 0, bad_tx = 0, bad_v = 0, sum = 0;

static void feed(const uint8_t* src, size_t len, uint64_t chain_id) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(exact.get(), src, len);
    std::vector<uint8_t> pre;
    uint8_t r[32], s[32], recid = 0xEE;
    const uint8_t st = phant::tx_signing_parts(exact.get(), len, chain_id, pre, r, s, &recid);
    if (st == PHANT_SIG_OK) {
        ++ok;
        if (recid > 1 || pre.empty() || pre.size() > len + 16) std::abort();  // the splice never grows beyond the tail it adds
        for (uint8_t b : pre) sum = sum * 31 + b;
        for (int i = 0; i < 32; ++i) sum = sum * 31 + r[i] + s[i];
    } else {
        if (!pre.empty() || (st != PHANT_SIG_BAD_TX && st != PHANT_SIG_BAD_V)) std::abort();  // nothing appended on failure
        ++(st == PHANT_SIG_BAD_TX ? bad_tx : bad_v);
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
        std::vector<uint8_t> tx(blob.begin() + at, blob.begin() + at + n);
        at += n;
        ++seeds;
        const uint64_t before = ok;
        feed(tx.data(), tx.size(), 1);
        if (ok != before + 1) {
            std::printf("seed %zu does not decode\n", seeds);
            return 4;
        }
        for (size_t cut = 0; cut < tx.size(); ++cut) feed(tx.data(), cut, 1);
        for (size_t pos = 0; pos < tx.size(); ++pos) {
            const uint8_t keep = tx[pos];
            for (int v = 0; v < 256; ++v) {
                if (v == keep) continue;
                tx[pos] = (uint8_t)v;
                feed(tx.data(), tx.size(), 1);
            }
            tx[pos] = keep;
        }
        feed(tx.data(), tx.size(), 0xFFFFFFFFFFFFFFFFull);
        feed(nullptr, 0, 1);
    }
    std::printf("%zu seeds: %llu decoded, %llu BAD_TX, %llu BAD_V, checksum %llx\n", seeds, (unsigned long long)ok,
                (unsigned long long)bad_tx, (unsigned long long)bad_v, (unsigned long long)sum);
    return 0;
}
