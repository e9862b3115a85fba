// receipts_decode_main.cpp -- the host splitter of phant_receipts_decode_rlp (phant_amd/csrc/host_rlp.cpp: receipts_split) against the
// verdicts of the definition (tests/receipts_seg_ref.py: split), which tests/test_receipts_decode_native.py writes next to every entry of
// its corpus: the truncations, single-byte replacements and 2^64 - 1 lengths of a few seed messages.  Each entry is split in an allocation
// of exactly its size, so that AddressSanitizer sees one byte too far, and its values are written into arrays of exactly the totals the
// counting pass reported.  Status, count and every value byte must be the definition's; a refused entry must leave the totals alone.
// Built with g++ -fsanitize=address,undefined.  Input file: records "len(4 LE) eth69(4) status(4) n(4) bytes(4) block bytes, values";
// prints how many entries were split.
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
    unsigned long long entries = 0, by_status[6] = {0, 0, 0, 0, 0, 0}, receipts = 0;
    for (size_t at = 0; at + 20 <= blob.size(); ++entries) {
        uint32_t head[5];
        std::memcpy(head, blob.data() + at, 20);
        const uint32_t len = head[0], eth69 = head[1], want_status = head[2], want_n = head[3], want_bytes = head[4];
        at += 20;
        if (at + len + want_bytes > blob.size()) return 3;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
        if (len) std::memcpy(exact.get(), blob.data() + at, len);
        const uint8_t* const want_values = reinterpret_cast<const uint8_t*>(blob.data()) + at + len;
        at += len + want_bytes;
        phant::ReceiptTotals t{0, 0};
        const uint8_t st = phant::receipts_split(exact.get(), len, eth69 != 0, t, nullptr);
        if (st != want_status) return std::printf("entry %llu: verdict %u, the definition's %u\n", entries, st, want_status), 4;
        if (st > 5) return 4;
        ++by_status[st];
        if (t.n != want_n || t.bytes != want_bytes) return std::printf("entry %llu: totals %llu %llu\n", entries, (unsigned long long)t.n, (unsigned long long)t.bytes), 5;
        if (st != PHANT_SPLIT_OK) continue;
        // the writing pass into arrays of exactly the reported sizes
        std::unique_ptr<uint8_t[]> out(new uint8_t[t.bytes ? t.bytes : 1]);
        std::vector<uint64_t> off(t.n + 1, ~0ull);
        off[0] = 0;
        const phant::ReceiptSink sink{out.get(), off.data()};
        phant::ReceiptTotals w{0, 0};
        if (phant::receipts_split(exact.get(), len, eth69 != 0, w, &sink) != PHANT_SPLIT_OK || w.n != t.n || w.bytes != t.bytes) return 6;
        if (off[t.n] != t.bytes) return std::printf("entry %llu: the offsets do not end at the total\n", entries), 7;
        for (size_t k = 0; k < t.n; ++k)
            if (off[k + 1] < off[k]) return 7;
        if (std::memcmp(out.get(), want_values, t.bytes) != 0) return std::printf("entry %llu: the values differ from the definition's\n", entries), 8;
        receipts += t.n;
    }
    std::printf("%llu entries: %llu split, %llu BAD_RLP, %llu BAD_RECEIPT, %llu receipts\n", entries, by_status[0], by_status[1], by_status[5], receipts);
    return 0;
}
