// ranges_main.cpp -- the leaf rules and the walkers' slot and divergence decisions of phant_mpt_verify_ranges
// (phant_amd/csrc/range_verify.hip.h: range::leaf_rule, range::cmp_keys, range::SideRule, compiled here for the host alone) as a
// stand-alone program, meant to be built with -fsanitize=address,undefined and run over a corpus tests/test_ranges_native.py writes
// from the definition (tests/range_ref.py).  A record, little-endian, 128 bytes:
//   u32 kind
//   kind 0, a leaf:      u32 flags (1: there is a leaf in front of it, 2: the first leaf of a range with a proof), u64 value length,
//                        key, the key in front, the origin (32 bytes each), u32 the rule it breaks (0: none), 12 bytes unused
//   kind 1, a branch:    u32 right, u32 nibble, u32 mask of the slots the walker emits (bit s: slot s), 112 bytes unused
//   kind 2, a divergence: u32 right, u32 before (the node sorts in front of the key), u32 emitted, 112 bytes unused
// Exit status 0: every record agrees.
#include <cstdio>
#include <cstring>
#include <vector>

#define PHANT_RANGE_RULES_ONLY
#include "../../phant_amd/csrc/range_verify.hip.h"

using namespace phant::range;

struct __attribute__((packed)) Record {
    uint32_t kind, a;
    union {
        struct __attribute__((packed)) {
            uint64_t vlen;
            uint8_t key[32], prev[32], origin[32];
            uint32_t expected;
            uint8_t unused[12];
        } leaf;
        struct __attribute__((packed)) {
            uint32_t b, expected;
            uint8_t unused[112];
        } walk;
    };
};
static_assert(sizeof(Record) == 128, "the corpus is written in records of 128 bytes");

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    std::vector<uint8_t> blob;
    uint8_t buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + k);
    std::fclose(f);
    if (blob.size() % sizeof(Record)) return std::fprintf(stderr, "the corpus is no whole number of records\n"), 2;
    size_t entries = 0, counts[3] = {0, 0, 0}, broken = 0;
    for (size_t at = 0; at < blob.size(); at += sizeof(Record), ++entries) {
        Record rec;  // (a copy: the corpus has no alignment)
        std::memcpy(&rec, blob.data() + at, sizeof rec);
        if (rec.kind > 2u) return std::fprintf(stderr, "record %zu: no such kind\n", entries), 2;
        ++counts[rec.kind];
        if (rec.kind == 0u) {
            // exact copies on the heap: a read beyond a key's 32 bytes is the sanitizer's to find
            std::vector<uint8_t> key(rec.leaf.key, rec.leaf.key + 32), prev(rec.leaf.prev, rec.leaf.prev + 32), origin(rec.leaf.origin, rec.leaf.origin + 32);
            const uint32_t got = leaf_rule(key.data(), rec.leaf.vlen, (rec.a & 1u) ? prev.data() : nullptr, (rec.a & 2u) ? origin.data() : nullptr);
            if (got != rec.leaf.expected) return std::fprintf(stderr, "record %zu: leaf_rule gives %u, the definition %u\n", entries, got, rec.leaf.expected), 1;
            broken += got != 0u;
            const int c = cmp_keys(key.data(), prev.data());
            if ((c < 0) != (std::memcmp(key.data(), prev.data(), 32) < 0) || (c == 0) != (key == prev))
                return std::fprintf(stderr, "record %zu: cmp_keys disagrees with memcmp\n", entries), 1;
        } else if (rec.kind == 1u) {
            const SideRule rule{rec.a != 0u};
            uint32_t front_end = 0, back_begin = 16, back_end = 16, mask = 0;
            rule.slots(0, rec.walk.b, front_end, back_begin, back_end);
            if (front_end > 16u || back_begin > 16u || back_end > 16u) return std::fprintf(stderr, "record %zu: a slot beyond 16\n", entries), 1;
            for (uint32_t s = 0; s < front_end; ++s) mask |= 1u << s;
            for (uint32_t s = back_begin; s < back_end; ++s) mask |= 1u << s;
            if (mask != rec.walk.expected || ((mask >> rec.walk.b) & 1u))
                return std::fprintf(stderr, "record %zu: slots %04x, the definition %04x\n", entries, mask, rec.walk.expected), 1;
        } else {
            const SideRule rule{rec.a != 0u};
            const auto unused = [](const uint8_t*) { return 0; };
            if (rule.diverging(rec.walk.b != 0u, 0, unused) != (rec.walk.expected != 0u))
                return std::fprintf(stderr, "record %zu: the divergence is decided the other way\n", entries), 1;
        }
    }
    std::printf("%zu records: %zu leaves (%zu break a rule), %zu branches, %zu divergences\n", entries, counts[0], broken, counts[1], counts[2]);
    return 0;
}
