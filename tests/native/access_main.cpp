// access_main.cpp -- the lane functions of phant_block_access_lists (phant_amd/csrc/access_lists.hip.h: al::walk_tuple, walk_count, key_ok,
// load_key / same_key, slot_home, tuple_home, and txstate.hip.h's load_addr / home_slot / same_addr they build on, compiled here for the
// host alone) as a stand-alone program, meant to be built with -fsanitize=address,undefined and run over a corpus
// tests/test_access_native.py writes from the definition (tests/access_ref.py).  The program joins the way the kernels do -- tables with
// open addressing where the lowest index wins -- but one entry after the other, and every span lies in an allocation of exactly its
// size: a walk that read one byte beyond its span would be reported.  A case, little-endian u32 unless said otherwise:
//   n, n_accounts, n_slots;  addresses (20 each), slot_first (n_accounts + 1), slots (32 each);  per span: its length, its bytes;
//   expected: n_tuples, n_keys, n_missing_accounts, n_missing_slots, first_malformed;  tuple_first (n + 1), al_flags, warm_addresses,
//   warm_keys (n each);  address (20 each), key_first (n_tuples + 1), account_row, tuple_same;  key (32 each), slot_row, key_same
// Exit status 0: every case agrees, under two different keys of the mix.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#define PHANT_AL_WALK_ONLY
#include "../../phant_amd/csrc/access_lists.hip.h"

using namespace phant;
using namespace phant::al;

struct Reader {
    const std::vector<uint8_t>& b;
    size_t at = 0;
    bool ok = true;
    uint32_t u32() {
        uint32_t v = 0;
        if (at + 4 > b.size()) return ok = false, 0u;
        std::memcpy(&v, b.data() + at, 4), at += 4;
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {
        if (at + n > b.size()) return ok = false, std::vector<uint8_t>();
        std::vector<uint8_t> v(b.begin() + at, b.begin() + at + n);
        at += n;
        return v;
    }
    std::vector<uint32_t> words(size_t n) {
        std::vector<uint32_t> v(n);
        for (auto& x : v) x = u32();
        return v;
    }
};

// a table of the kernels' kind, filled one entry after the other: `same(old)` tells whether the holder of a slot equals the newcomer
struct Table {
    std::vector<uint32_t> slot;
    uint32_t mask;
    explicit Table(size_t entries) {
        size_t s = 64;
        while (s < 2 * entries) s <<= 1;
        slot.assign(s, NONE), mask = (uint32_t)s - 1u;
    }
    template <class Same>
    void claim(uint32_t home, uint32_t me, Same same) {
        for (uint32_t at = home & mask;; at = (at + 1u) & mask) {
            if (slot[at] == NONE) return void(slot[at] = me);
            if (same(slot[at])) return void(slot[at] = slot[at] < me ? slot[at] : me);
        }
    }
    template <class Same>
    uint32_t find(uint32_t home, Same same) const {
        for (uint32_t at = home & mask;; at = (at + 1u) & mask) {
            if (slot[at] == NONE || same(slot[at])) return slot[at];
        }
    }
};

struct TupleRec {
    uint32_t txi;
    const uint8_t* addr;
    uint32_t kfirst, same, row;
};
struct KeyRec {
    uint32_t tuple;
    const uint8_t* key;
};

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    std::vector<uint8_t> blob;
    uint8_t buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + k);
    std::fclose(f);
    Reader r{blob};
    size_t cases = 0, tuples_seen = 0, keys_seen = 0, malformed_seen = 0, joined = 0;
    while (r.at < blob.size()) {
        const uint32_t n = r.u32(), na = r.u32(), ns = r.u32();
        const std::vector<uint8_t> addresses = r.bytes(20 * (size_t)na);
        const std::vector<uint32_t> slot_first = r.words((size_t)na + 1);
        const std::vector<uint8_t> slots = r.bytes(32 * (size_t)ns);
        std::vector<std::unique_ptr<uint8_t[]>> span(n);
        std::vector<uint32_t> len(n);
        for (uint32_t i = 0; i < n && r.ok; ++i) {
            len[i] = r.u32();
            const std::vector<uint8_t> b = r.bytes(len[i]);
            span[i].reset(new uint8_t[len[i]]);  // (exactly the span: nothing behind it belongs to the program)
            if (len[i]) std::memcpy(span[i].get(), b.data(), len[i]);
        }
        const uint32_t e_tuples = r.u32(), e_keys = r.u32(), e_miss_a = r.u32(), e_miss_s = r.u32(), e_first = r.u32();
        const std::vector<uint32_t> e_tuple_first = r.words((size_t)n + 1), e_flags = r.words(n), e_warm_a = r.words(n), e_warm_k = r.words(n);
        const std::vector<uint8_t> e_address = r.bytes(20 * (size_t)e_tuples);
        const std::vector<uint32_t> e_key_first = r.words((size_t)e_tuples + 1), e_row = r.words(e_tuples), e_tsame = r.words(e_tuples);
        const std::vector<uint8_t> e_key = r.bytes(32 * (size_t)e_keys);
        const std::vector<uint32_t> e_srow = r.words(e_keys), e_ksame = r.words(e_keys);
        if (!r.ok) return std::fprintf(stderr, "case %zu: the corpus ends inside it\n", cases), 2;
#define FAIL(...) return std::fprintf(stderr, "case %zu: ", cases), std::fprintf(stderr, __VA_ARGS__), std::fprintf(stderr, "\n"), 1

        for (uint32_t salt = 0; salt < 2; ++salt) {
            const uint32_t s0 = salt ? 0x243f6a88u : 0u, s1 = salt ? 0x85a308d3u : 0u;
            // the witness's tables
            Table rows(na), slot_rows(ns);
            for (uint32_t j = 0; j < na; ++j) {
                uint32_t w[5];
                txst::load_addr(addresses.data() + 20 * (size_t)j, w);
                rows.claim(txst::home_slot(w, s0, s1), j, [&](uint32_t old) { return txst::same_addr(addresses.data() + 20 * (size_t)old, w); });
                for (uint32_t s = slot_first[j]; s < slot_first[j + 1]; ++s) {
                    uint32_t k[8];
                    load_key(slots.data() + 32 * (size_t)s, k);
                    slot_rows.claim(slot_home(j, k, s0, s1), s, [&](uint32_t old) {
                        return old >= slot_first[j] && old < slot_first[j + 1] && same_key(slots.data() + 32 * (size_t)old, k);
                    });
                }
            }
            // the walk: headers first, then every key by itself
            std::vector<TupleRec> tuples;
            std::vector<KeyRec> keys;
            std::vector<uint32_t> tuple_first(1, 0u), flags(n, 0u), warm_a(n, 0u), warm_k(n, 0u);
            uint32_t first_malformed = n;
            for (uint32_t i = 0; i < n; ++i) {
                const uint8_t* const p = span[i].get();
                uint32_t ct = 0, ck = 0;
                bool ok = walk_count(p, len[i], ct, ck);
                const size_t t0 = tuples.size(), k0 = keys.size();
                Tuple t;
                for (uint32_t pos = 0; ok && pos < len[i]; pos = t.next) {
                    if (!walk_tuple(p, pos, len[i], t)) FAIL("row %u: the second walk disagrees with the first", i);
                    tuples.push_back(TupleRec{i, p + t.addr, (uint32_t)keys.size(), 0u, 0u});
                    for (uint32_t j = 0; j < t.n_keys; ++j) {
                        if (!key_ok(p, t.keys, j)) ok = false;  // (every key of the tuple is looked at, as every key has its lane)
                        keys.push_back(KeyRec{(uint32_t)tuples.size() - 1u, p + key_at(t.keys, j)});
                    }
                }
                if (ok && (tuples.size() - t0 != ct || keys.size() - k0 != ck)) FAIL("row %u: the counts of the two walks differ", i);
                if (!ok) {
                    tuples.resize(t0), keys.resize(k0), flags[i] = PHANT_AL_MALFORMED;
                    if (first_malformed == n) first_malformed = i;
                }
                tuple_first.push_back((uint32_t)tuples.size());
            }
            // the joins and the first occurrences
            Table tsame(tuples.size()), ksame(keys.size());
            uint32_t miss_a = 0, miss_s = 0;
            for (uint32_t e = 0; e < tuples.size(); ++e) {
                uint32_t w[5];
                txst::load_addr(tuples[e].addr, w);
                tsame.claim(tuple_home(tuples[e].txi, w, s0, s1), e,
                            [&](uint32_t old) { return tuples[old].txi == tuples[e].txi && txst::same_addr(tuples[old].addr, w); });
            }
            for (uint32_t e = 0; e < tuples.size(); ++e) {
                TupleRec& t = tuples[e];
                uint32_t w[5];
                txst::load_addr(t.addr, w);
                t.same = tsame.find(tuple_home(t.txi, w, s0, s1), [&](uint32_t j) { return tuples[j].txi == t.txi && txst::same_addr(tuples[j].addr, w); });
                t.row = na ? rows.find(txst::home_slot(w, s0, s1), [&](uint32_t j) { return txst::same_addr(addresses.data() + 20 * (size_t)j, w); }) : (uint32_t)NONE;
                if (t.same == e) ++warm_a[t.txi], miss_a += t.row == NONE;
                else flags[t.txi] |= PHANT_AL_DUPLICATES;
                if (std::memcmp(t.addr, e_address.data() + 20 * (size_t)e, 20) || t.row != e_row[e] || t.same != e_tsame[e] || t.kfirst != e_key_first[e])
                    FAIL("tuple %u: row %u (expected %u), same %u (expected %u), first key %u (expected %u)", e, t.row, e_row[e], t.same, e_tsame[e], t.kfirst,
                         e_key_first[e]);
                joined += t.row != NONE;
            }
            for (uint32_t k = 0; k < keys.size(); ++k) {
                uint32_t w[8];
                load_key(keys[k].key, w);
                const uint32_t under = tuples[keys[k].tuple].same;
                ksame.claim(slot_home(under, w, s0, s1), k, [&](uint32_t old) { return tuples[keys[old].tuple].same == under && same_key(keys[old].key, w); });
            }
            for (uint32_t k = 0; k < keys.size(); ++k) {
                uint32_t w[8];
                load_key(keys[k].key, w);
                const TupleRec& t = tuples[keys[k].tuple];
                const uint32_t same = ksame.find(slot_home(t.same, w, s0, s1), [&](uint32_t j) { return tuples[keys[j].tuple].same == t.same && same_key(keys[j].key, w); });
                uint32_t srow = NONE;
                if (t.row != NONE)
                    srow = slot_rows.find(slot_home(t.row, w, s0, s1), [&](uint32_t s) {
                        return s >= slot_first[t.row] && s < slot_first[t.row + 1] && same_key(slots.data() + 32 * (size_t)s, w);
                    });
                if (same == k) ++warm_k[t.txi], miss_s += srow == NONE;
                else flags[t.txi] |= PHANT_AL_DUPLICATES;
                if (std::memcmp(keys[k].key, e_key.data() + 32 * (size_t)k, 32) || srow != e_srow[k] || same != e_ksame[k])
                    FAIL("key %u: slot %u (expected %u), same %u (expected %u)", k, srow, e_srow[k], same, e_ksame[k]);
                joined += srow != NONE;
            }
            if (tuples.size() != e_tuples || keys.size() != e_keys || e_key_first[e_tuples] != e_keys) FAIL("%zu tuples, %zu keys", tuples.size(), keys.size());
            if (tuple_first != e_tuple_first || flags != e_flags || warm_a != e_warm_a || warm_k != e_warm_k) FAIL("the per-row outputs differ");
            if (miss_a != e_miss_a || miss_s != e_miss_s || first_malformed != e_first)
                FAIL("missing %u / %u (expected %u / %u), first malformed %u (expected %u)", miss_a, miss_s, e_miss_a, e_miss_s, first_malformed, e_first);
            if (salt == 0) {
                tuples_seen += tuples.size(), keys_seen += keys.size();
                for (uint32_t i = 0; i < n; ++i) malformed_seen += (flags[i] & PHANT_AL_MALFORMED) != 0u;
            }
        }
        ++cases;
    }
    std::printf("%zu cases, %zu tuples, %zu keys, %zu malformed, %zu joined\n", cases, tuples_seen, keys_seen, malformed_seen, joined);
    return 0;
}
