// settle_main.cpp -- the per-row functions and the 320-bit signed arithmetic of phant_block_settle (phant_amd/csrc/settle.hip.h:
// settle::classify, tx_event / wd_event, row_rule, account_rule, add320 / sub320 / neg320 / mul_u64_u256 / clamp256 / below, compiled
// here for the host alone) as a stand-alone program, meant to be built with -fsanitize=address,undefined and run over a corpus
// tests/test_settle_native.py writes from the definition (tests/settle_ref.py).  Records, little-endian, each behind a kind byte:
//   1 (a transaction): u32 fork, type, tx_flags, state_flags, sender_row, to_row;  u64 intrinsic_gas, floor_gas, gas_limit,
//     block_gas_limit;  value, price, base_fee, upfront_cost, to_code_hash (32 bytes big-endian each), to (20);  cum[3] (u32 limbs: the
//     gas up to and including the row), balance[10] (i32 limbs, signed: the sender's before the row);  expected: u32 class, u64 gas,
//     the three events' values (10 limbs each, signed), u32 flags of row_rule, u64 cumulative_gas_used, balance_before (32 bytes)
//   2 (an account): u8 status, u8 code_empty, u64 nonce, u32 sends, total[10] (signed);  expected: u32 op, u64 nonce_after,
//     balance (32 bytes), u32 flags
//   3 (a withdrawal): u64 gwei;  expected: value[10]
// Exit status 0: every record agrees.
#include <cstdio>
#include <cstring>
#include <vector>

#define PHANT_TXST_RULE_ONLY
#define PHANT_SETTLE_RULE_ONLY
#include "../../phant_amd/csrc/settle.hip.h"

using namespace phant::settle;

struct __attribute__((packed)) TxRecord {
    uint32_t fork, type, tx_flags, state_flags, sender_row, to_row;
    uint64_t intrinsic_gas, floor_gas, gas_limit, block_gas_limit;
    uint8_t value[32], price[32], base_fee[32], upfront_cost[32], to_code_hash[32], to[20];
    uint32_t cum[3], balance[10];
    uint32_t cls;
    uint64_t gas;
    uint32_t events[3][10];
    uint32_t flags;
    uint64_t cumulative;
    uint8_t balance_before[32];
};
struct __attribute__((packed)) AccountRecord {
    uint8_t status, code_empty;
    uint64_t nonce;
    uint32_t sends, total[10];
    uint32_t op;
    uint64_t nonce_after;
    uint8_t balance[32];
    uint32_t flags;
};
struct __attribute__((packed)) WdRecord {
    uint64_t gwei;
    uint32_t value[10];
};

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s corpus.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    std::vector<uint8_t> blob;
    uint8_t buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + k);
    std::fclose(f);
    size_t entries = 0, plain = 0, flagged = 0, deleted = 0, clamped = 0;
    for (size_t at = 0; at < blob.size(); ++entries) {
        const uint8_t kind = blob[at++];
        if (kind == 1 && at + sizeof(TxRecord) <= blob.size()) {
            TxRecord rec;  // (a copy: the corpus has no alignment)
            std::memcpy(&rec, blob.data() + at, sizeof rec);
            at += sizeof rec;
            TxRow r;
            r.fork = rec.fork, r.type = rec.type, r.tx_flags = rec.tx_flags, r.state_flags = rec.state_flags, r.sender_row = rec.sender_row, r.to_row = rec.to_row;
            r.intrinsic_gas = rec.intrinsic_gas, r.floor_gas = rec.floor_gas;
            r.value = rec.value, r.price = rec.price, r.to = rec.to, r.base_fee = rec.base_fee;
            r.to_code_hash = rec.to_row == PHANT_ROW_NONE ? nullptr : rec.to_code_hash;
            uint64_t gas = 0;
            const uint32_t cls = classify(r, gas);
            if (cls != rec.cls || gas != rec.gas) return std::fprintf(stderr, "record %zu: class %x (expected %x), gas %llu\n", entries, cls, rec.cls, (unsigned long long)gas), 1;
            if (cls) continue;
            ++plain;
            uint32_t own[LIMBS] = {0};
            for (uint32_t k = 0; k < 3u; ++k) {
                uint32_t w[LIMBS];
                tx_event(k, gas, rec.value, rec.price, rec.base_fee, w);
                if (std::memcmp(w, rec.events[k], sizeof w)) return std::fprintf(stderr, "record %zu: event %u disagrees\n", entries, k), 1;
                if (k == 0) std::memcpy(own, w, sizeof own);
            }
            // the kernel's way to the balance before the row: the pre-state's plus the scan up to and including the debit, minus the debit
            uint32_t before[LIMBS], incl[LIMBS];
            std::memcpy(incl, rec.balance, sizeof incl);
            add320(incl, own);
            std::memcpy(before, incl, sizeof before);
            sub320(before, own);
            if (std::memcmp(before, rec.balance, sizeof before)) return std::fprintf(stderr, "record %zu: add320 / sub320 disagree\n", entries), 1;
            uint64_t cumulative = 0;
            uint32_t cum[3];  // (the record is packed: its words have no alignment)
            std::memcpy(cum, rec.cum, sizeof cum);
            const uint32_t flags = row_rule(gas, rec.gas_limit, rec.block_gas_limit, cum, before, rec.upfront_cost, cumulative);
            uint32_t bal[8];
            (void)clamp256(before, bal);
            uint8_t balance_before[32];
            phant::txst::store_be256(balance_before, bal);
            if (flags != rec.flags || cumulative != rec.cumulative || std::memcmp(balance_before, rec.balance_before, 32))
                return std::fprintf(stderr, "record %zu: flags %x (expected %x), cumulative %llu (expected %llu)\n", entries, flags, rec.flags,
                                    (unsigned long long)cumulative, (unsigned long long)rec.cumulative), 1;
            flagged += flags != 0u;
        } else if (kind == 2 && at + sizeof(AccountRecord) <= blob.size()) {
            AccountRecord rec;
            std::memcpy(&rec, blob.data() + at, sizeof rec);
            at += sizeof rec;
            uint64_t nonce_after = 0;
            uint32_t bal[8], flags = 0;
            uint32_t total[LIMBS];
            std::memcpy(total, rec.total, sizeof total);
            const uint32_t op = account_rule(rec.status, rec.nonce, rec.sends, total, rec.code_empty != 0, nonce_after, bal, flags);
            uint8_t balance[32];
            phant::txst::store_be256(balance, bal);
            if (op != rec.op || nonce_after != rec.nonce_after || flags != rec.flags || std::memcmp(balance, rec.balance, 32))
                return std::fprintf(stderr, "record %zu: op %u (expected %u), flags %x (expected %x)\n", entries, op, rec.op, flags, rec.flags), 1;
            deleted += op == PHANT_POST_DELETE, clamped += flags != 0u;
        } else if (kind == 3 && at + sizeof(WdRecord) <= blob.size()) {
            WdRecord rec;
            std::memcpy(&rec, blob.data() + at, sizeof rec);
            at += sizeof rec;
            uint32_t w[LIMBS];
            wd_event(rec.gwei, w);
            if (std::memcmp(w, rec.value, sizeof w)) return std::fprintf(stderr, "record %zu: the withdrawal's value disagrees\n", entries), 1;
        } else {
            return std::fprintf(stderr, "record %zu: the corpus ends inside it, or its kind is unknown\n", entries), 2;
        }
    }
    std::printf("%zu entries, %zu plain, %zu flagged, %zu deleted, %zu clamped\n", entries, plain, flagged, deleted, clamped);
    return 0;
}
