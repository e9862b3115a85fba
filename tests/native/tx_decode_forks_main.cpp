// tx_decode_forks_main.cpp -- the fork-taking device decode of a transaction (phant_amd/csrc/transactions.hip.h: tx::decode with a fork,
// compiled here for the host with PHANT_TX_DECODE_ONLY) against the verdicts of the definition (tests/tx_ref_forks.py), which
// tests/test_tx_decode_forks_native.py writes next to every entry of its corpus: the truncations, single-byte replacements and
// 2^64 - 1 lengths of type-3 and type-4 seeds.  Each entry is decoded in an allocation of exactly its size, so that AddressSanitizer
// sees one byte too far; the status, the tuple count and the blob count must be the definition's, every span must lie inside the
// transaction, and the second walk over the tuples (what tx_auth_rows_kernel does) must find as many as the decode counted.  Built with
// g++ -fsanitize=address,undefined.  Input file: records "len(4 LE) fork(4) chain_id(8) status(4) tuples(4) blobs(4) bytes"; prints how
// many entries decoded.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

#define PHANT_TX_DECODE_ONLY
#include "../../phant_amd/csrc/transactions.hip.h"

using namespace phant::tx;

static bool inside(Span s, size_t len) { return (size_t)s.at + s.len <= len; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    unsigned long long entries = 0, ok = 0, bad_tx = 0, bad_v = 0, tuples = 0, blobs = 0;
    for (size_t at = 0; at + 28 <= blob.size(); ++entries) {
        uint32_t head[7];
        std::memcpy(head, blob.data() + at, 28);
        const uint32_t len = head[0], fork = head[1], want_status = head[4], want_tuples = head[5], want_blobs = head[6];
        uint64_t chain_id;
        std::memcpy(&chain_id, head + 2, 8);
        at += 28;
        if (at + len > blob.size()) return 3;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
        if (len) std::memcpy(exact.get(), blob.data() + at, len);
        at += len;
        const uint8_t* p = exact.get();
        Decoded d;
        decode(p, len, chain_id, fork, d);
        if (d.status != want_status) return std::printf("entry %llu: verdict %u, the definition's %u\n", entries, d.status, want_status), 4;
        ++(d.status == ST_OK ? ok : d.status == ST_BAD_TX ? bad_tx : bad_v);
        if (d.status == ST_BAD_TX) continue;
        if (d.tuples != want_tuples || d.blobs != want_blobs)
            return std::printf("entry %llu: %u tuples, %u blobs; the definition's %u, %u\n", entries, d.tuples, d.blobs, want_tuples, want_blobs), 5;
        tuples += d.tuples, blobs += d.blobs;
        for (Span s : {d.priority, d.gas_price, d.value, d.to, d.data, d.al, d.r, d.s, d.blob_fee, d.hashes, d.auths})
            if (!inside(s, len)) return std::printf("entry %llu: span out of range\n", entries), 6;
        if (d.hashes.len != 33u * d.blobs) return std::printf("entry %llu: hashes of other than 33 bytes\n", entries), 6;
        uint32_t pos = d.auths.at, walked = 0;
        for (const uint32_t end = d.auths.at + d.auths.len; pos < end; ++walked) {
            Auth a;
            if (!auth_tuple(p, pos, end, a, pos)) return std::printf("entry %llu: the second walk fails\n", entries), 7;
            for (Span s : {a.chain_id, a.address, a.nonce, a.y_parity, a.r, a.s})
                if (!inside(s, len)) return std::printf("entry %llu: tuple span out of range\n", entries), 7;
        }
        if (walked != d.tuples) return std::printf("entry %llu: the second walk finds %u tuples\n", entries, walked), 7;
        if (d.status == ST_OK && (d.body_begin > d.body_end || d.body_end > len || d.prefix_len > 10 || d.suffix_len != 0 || d.prefix[0] != d.type))
            return std::printf("entry %llu: plan out of range\n", entries), 8;
        // the two-argument form knows neither type
        Decoded old;
        decode(p, len, chain_id, old);
        if (d.type >= 3u && old.status != ST_BAD_TX) return std::printf("entry %llu: decoded without a fork\n", entries), 9;
    }
    std::printf("%llu entries: %llu decoded, %llu BAD_TX, %llu BAD_V, %llu tuples, %llu blobs\n", entries, ok, bad_tx, bad_v, tuples, blobs);
    return 0;
}
