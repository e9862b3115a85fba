// bodies_decode_main.cpp -- the host splitter of phant_bodies_decode_rlp (phant_amd/csrc/host_rlp.cpp: body_split) against the verdicts of
// the definition (tests/bodies_ref.py: split), which tests/test_bodies_decode_native.py writes next to every entry of its corpus: the
// truncations, single-byte replacements and 2^64 - 1 lengths of a few seed blocks.  Each entry is split in an allocation of exactly its
// size, so that AddressSanitizer sees one byte too far, and its values are written into arrays of exactly the totals the counting pass
// reported.  Status, counts and every value byte must be the definition's; a refused entry must leave the totals alone.  Built with
// g++ -fsanitize=address,undefined.  Input file: records "len(4 LE) bodies_only(4) status(4) n_tx(4) n_wd(4) tx_bytes(4) wd_bytes(4) block
// bytes, tx values, wd values"; prints how many entries were split.
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::string blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    unsigned long long entries = 0, by_status[5] = {0, 0, 0, 0, 0}, txs = 0, wds = 0;
    for (size_t at = 0; at + 28 <= blob.size(); ++entries) {
        uint32_t head[7];
        std::memcpy(head, blob.data() + at, 28);
        const uint32_t len = head[0], bodies_only = head[1], want_status = head[2], want_n = head[3], want_wd = head[4], want_txb = head[5], want_wdb = head[6];
        at += 28;
        if (at + len + want_txb + want_wdb > blob.size()) return 3;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
        if (len) std::memcpy(exact.get(), blob.data() + at, len);
        const uint8_t* const want_tx_bytes = reinterpret_cast<const uint8_t*>(blob.data()) + at + len;
        const uint8_t* const want_wd_bytes = want_tx_bytes + want_txb;
        at += len + want_txb + want_wdb;
        phant::BodyTotals t{0, 0, 0, 0};
        const uint8_t st = phant::body_split(exact.get(), len, bodies_only == 0, t, nullptr);
        if (st != want_status) return std::printf("entry %llu: verdict %u, the definition's %u\n", entries, st, want_status), 4;
        if (st > 4) return 4;
        ++by_status[st];
        if (t.n != want_n || t.n_wd != want_wd || t.tx_bytes != want_txb || t.wd_bytes != want_wdb)
            return std::printf("entry %llu: totals %llu %llu %llu %llu\n", entries, (unsigned long long)t.n, (unsigned long long)t.n_wd,
                               (unsigned long long)t.tx_bytes, (unsigned long long)t.wd_bytes), 5;
        if (st != PHANT_SPLIT_OK) continue;
        // the writing pass into arrays of exactly the reported sizes, behind one earlier block's worth of rows
        std::unique_ptr<uint8_t[]> tx_out(new uint8_t[t.tx_bytes ? t.tx_bytes : 1]), wd_out(new uint8_t[t.wd_bytes ? t.wd_bytes : 1]);
        std::vector<uint64_t> tx_off(t.n + 1, ~0ull), wd_off(t.n_wd + 1, ~0ull);
        tx_off[0] = wd_off[0] = 0;
        const phant::BodySink sink{tx_out.get(), tx_off.data(), wd_out.get(), wd_off.data()};
        phant::BodyTotals w{0, 0, 0, 0};
        if (phant::body_split(exact.get(), len, bodies_only == 0, w, &sink) != PHANT_SPLIT_OK) return 6;
        if (w.n != t.n || w.n_wd != t.n_wd || w.tx_bytes != t.tx_bytes || w.wd_bytes != t.wd_bytes) return 6;
        if (tx_off[t.n] != t.tx_bytes || wd_off[t.n_wd] != t.wd_bytes) return std::printf("entry %llu: the offsets do not end at the totals\n", entries), 7;
        for (size_t k = 0; k < t.n; ++k)
            if (tx_off[k + 1] < tx_off[k]) return 7;
        if (std::memcmp(tx_out.get(), want_tx_bytes, t.tx_bytes) != 0 || std::memcmp(wd_out.get(), want_wd_bytes, t.wd_bytes) != 0)
            return std::printf("entry %llu: the values differ from the definition's\n", entries), 8;
        txs += t.n, wds += t.n_wd;
    }
    std::printf("%llu entries: %llu split, %llu BAD_RLP, %llu BAD_TX, %llu UNCLES, %llu BAD_WITHDRAWAL, %llu transactions, %llu withdrawals\n", entries,
                by_status[0], by_status[1], by_status[2], by_status[3], by_status[4], txs, wds);
    return 0;
}
