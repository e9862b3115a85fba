// txstate_main.cpp -- the per-row sender rule and the 288-bit arithmetic of phant_block_txs_prestate (phant_amd/csrc/txstate.hip.h:
// txst::sender_rule, add288 / sub288 / less288, load_be256 / store_be256, compiled here for the host alone) as a stand-alone program, meant to
// be built with -fsanitize=address,undefined and run over a corpus tests/test_txstate_native.py writes from the definition
// (tests/txstate_ref.py).  A record, little-endian:
//   u32 fork, i, rank, bits (1: the code hash is the empty one, 2: code_index is NONE, 4: the code is a designator, 8: authorized,
//   16: the balance is below spent + own);  u64 nonce, acc_nonce;  own[9], spent[9], incl[9] (u32 limbs: the row's cost, the sum before
//   it, both together);  balance (32 bytes big-endian);  expected: u32 flags, u64 expected_nonce, spent_before (32 bytes big-endian)
// Exit status 0: every record agrees.
#include <cstdio>
#include <cstring>
#include <vector>

#define PHANT_TXST_RULE_ONLY
#include "../../phant_amd/csrc/txstate.hip.h"

using namespace phant::txst;

struct __attribute__((packed)) Record {
    uint32_t fork, i, rank, bits;
    uint64_t nonce, acc_nonce;
    uint32_t own[9], spent[9], incl[9];
    uint8_t balance[32];
    uint32_t flags;
    uint64_t expected_nonce;
    uint8_t spent_before[32];
};

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    std::vector<uint8_t> blob;
    uint8_t buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + k);
    std::fclose(f);
    if (blob.size() % sizeof(Record)) return std::fprintf(stderr, "the corpus is no whole number of records\n"), 2;
    size_t entries = 0, flagged = 0, undetermined = 0, saturated = 0;
    for (size_t at = 0; at < blob.size(); at += sizeof(Record), ++entries) {
        Record rec;  // (a copy: the corpus has no alignment)
        std::memcpy(&rec, blob.data() + at, sizeof rec);
        uint32_t sum[9], back[9];
        std::memcpy(sum, rec.spent, sizeof sum);
        add288(sum, rec.own);
        if (std::memcmp(sum, rec.incl, sizeof sum)) return std::fprintf(stderr, "record %zu: add288 disagrees\n", entries), 1;
        std::memcpy(back, sum, sizeof back);
        sub288(back, rec.own);
        if (std::memcmp(back, rec.spent, sizeof back)) return std::fprintf(stderr, "record %zu: sub288 disagrees\n", entries), 1;
        RowIn r;
        r.fork = rec.fork, r.i = rec.i, r.rank = rec.rank, r.nonce = rec.nonce, r.acc_nonce = rec.acc_nonce;
        std::memcpy(r.own, rec.own, sizeof r.own);
        std::memcpy(r.incl, sum, sizeof r.incl);
        load_be256(rec.balance, r.balance);
        if (less288(r.balance, r.incl) != ((rec.bits & 16u) != 0u) || less288(r.incl, r.incl))
            return std::fprintf(stderr, "record %zu: less288 disagrees\n", entries), 1;
        r.code_empty = rec.bits & 1u, r.code_none = rec.bits & 2u, r.code_designator = rec.bits & 4u, r.authorized = rec.bits & 8u;
        RowOut o;
        sender_rule(r, o);
        uint8_t spent_before[32];
        store_be256(spent_before, o.spent);
        if (o.flags != rec.flags || o.expected_nonce != rec.expected_nonce || std::memcmp(spent_before, rec.spent_before, 32))
            return std::fprintf(stderr, "record %zu: flags %x (expected %x), nonce %llu (expected %llu)\n", entries, o.flags, rec.flags,
                                (unsigned long long)o.expected_nonce, (unsigned long long)rec.expected_nonce), 1;
        flagged += (o.flags & PHANT_TXST_ERROR_BITS) != 0u;
        undetermined += (o.flags & PHANT_TXST_UNDETERMINED) != 0u;
        saturated += (o.flags & PHANT_TXST_SPENT_SATURATED) != 0u;
    }
    std::printf("%zu entries, %zu flagged, %zu undetermined, %zu saturated\n", entries, flagged, undetermined, saturated);
    return 0;
}
