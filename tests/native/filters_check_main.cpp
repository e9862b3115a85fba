// filters_check_main.cpp -- the host-side checks of phant_block_log_filters and phant_log_filters_bloom (phant_amd/csrc/filters_check.h:
// check_match_args, check_bloom_args, check_rows_host, check_filters_host; the firsts rules of segment_checks.h) as a stand-alone program
// under AddressSanitizer + UBSan.  Every array lives in an allocation of exactly its entries, so a check that reads an entry too far is
// caught; a case is a good call with one thing wrong, and each must be refused (or accepted) as include/phant_gpu.h says.  Prints how many
// cases were refused and how many accepted; tests/test_filters_check_native.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../phant_amd/csrc/filters_check.h"

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// three blocks of 2, 0 and 3 receipts; 4 logs, 5 topics; two filters: 3 addresses and 0, topic sets of 1, 0, 2, 0 and 0, 0, 0, 1 entries
struct Call {
    std::vector<uint32_t> block_first{0, 2, 2, 5}, log_first{0, 2, 2, 3, 4, 4}, topic_first{0, 1, 1, 3, 5};
    std::vector<uint32_t> addr_first{0, 3, 3}, ftopic_first{0, 1, 1, 3, 3, 3, 3, 3, 4}, block_lo{0, 1}, block_hi{3, 2};
    std::vector<uint8_t> address = std::vector<uint8_t>(80, 0x11), topics = std::vector<uint8_t>(160, 0x22), addr = std::vector<uint8_t>(60, 0x33),
                         topic = std::vector<uint8_t>(128, 0x44), blooms = std::vector<uint8_t>(3 * 256, 0x55);
    phant_logmatch_in in;
    phant_log_filters fl;
    phant_logmatch_out out;
    std::unique_ptr<uint32_t[]> p_bf, p_lf, p_tf, p_af, p_ftf, p_lo, p_hi;
    std::unique_ptr<uint8_t[]> p_ad, p_tp, p_fa, p_ft, p_bl;
    uint64_t* may = nullptr;
    uint32_t* may_count = nullptr;

    void bind() {
        p_bf = exact(block_first), p_lf = exact(log_first), p_tf = exact(topic_first), p_af = exact(addr_first), p_ftf = exact(ftopic_first), p_lo = exact(block_lo);
        p_hi = exact(block_hi), p_ad = exact(address), p_tp = exact(topics), p_fa = exact(addr), p_ft = exact(topic), p_bl = exact(blooms);
        std::memset(&in, 0, sizeof in);
        std::memset(&fl, 0, sizeof fl);
        std::memset(&out, 0, sizeof out);
        in.struct_size = sizeof in, fl.struct_size = sizeof fl, out.struct_size = sizeof out;
        in.n_blocks = (uint32_t)block_first.size() - 1, in.n = (uint32_t)log_first.size() - 1, in.n_logs = (uint32_t)topic_first.size() - 1, in.n_topics = (uint32_t)topics.size() / 32;
        in.match_cap = 8;
        in.block_first = p_bf.get(), in.log_first = p_lf.get(), in.address = p_ad.get(), in.topic_first = p_tf.get(), in.topics = p_tp.get();
        fl.n_filters = (uint32_t)addr_first.size() - 1, fl.n_addr = (uint32_t)addr.size() / 20, fl.n_topic = (uint32_t)topic.size() / 32;
        fl.addr_first = p_af.get(), fl.addr = p_fa.get(), fl.topic_first = p_ftf.get(), fl.topic = p_ft.get(), fl.block_lo = p_lo.get(), fl.block_hi = p_hi.get();
    }
};

// PHANT_OK or the code the call answers before anything is copied: the exact call, or the bloom call over the three blooms
int32_t verdict(const Call& c, bool dev, bool bloom) {
    const char* const what = bloom ? phant::lf::check_bloom_args(c.p_bl.get(), 3, &c.fl, c.may, c.may_count, dev) : phant::lf::check_match_args(&c.in, &c.fl, &c.out, dev);
    if (*what) return PHANT_E_INVALID_ARG;
    if (c.fl.n_filters == 0 || dev) return PHANT_OK;
    std::string err;
    int32_t rc = PHANT_OK;
    if (!bloom && c.in.n_blocks) rc = phant::lf::check_rows_host("call", c.in, err);
    if (rc == PHANT_OK) rc = phant::lf::check_filters_host("call", c.fl, bloom ? 3u : c.in.n_blocks, err);
    if ((rc != PHANT_OK) != !err.empty()) return 100;  // (a refusal says why)
    if (rc == PHANT_OK && phant::lf::large_entries_host(c.fl, 2) != 3u) return 101;  // (one set above two entries: the three addresses)
    return rc;
}

}  // namespace

int main() {
    unsigned refused = 0, accepted = 0, cases = 0;
    bool bloom = false;
    auto expect = [&](const char* name, int32_t want, const std::function<void(Call&)>& before, const std::function<void(Call&)>& after, bool dev = false) {
        Call c;
        before(c);
        c.bind();
        after(c);
        const int32_t got = verdict(c, dev, bloom);
        ++cases, ++(got == PHANT_OK ? accepted : refused);
        if (got != want) std::printf("case %s (%s form, %s call): %d, expected %d\n", name, dev ? "device" : "host", bloom ? "bloom" : "exact", got, want);
        return got == want;
    };
    auto nothing = [](Call&) {};
    const int32_t BAD = PHANT_E_INVALID_ARG;
    bool ok = true;
    for (const bool b : {false, true}) {
        bloom = b;
        for (const bool dev : {false, true}) {
            ok &= expect("good", PHANT_OK, nothing, nothing, dev);
            ok &= expect("filters size", BAD, nothing, [](Call& c) { c.fl.struct_size += 8; }, dev);
            ok &= expect("filters reserved", BAD, nothing, [](Call& c) { c.fl.reserved = 1; }, dev);
            ok &= expect("null addr_first", BAD, nothing, [](Call& c) { c.fl.addr_first = nullptr; }, dev);
            ok &= expect("null topic_first of the filters", BAD, nothing, [](Call& c) { c.fl.topic_first = nullptr; }, dev);
            ok &= expect("null addr", BAD, nothing, [](Call& c) { c.fl.addr = nullptr; }, dev);
            ok &= expect("null topic", BAD, nothing, [](Call& c) { c.fl.topic = nullptr; }, dev);
            ok &= expect("entries without a filter", BAD, nothing, [](Call& c) { c.fl.n_filters = 0; }, dev);
            ok &= expect("no filter", PHANT_OK, nothing, [](Call& c) { c.fl.n_filters = c.fl.n_addr = c.fl.n_topic = 0, c.fl.addr_first = c.fl.topic_first = nullptr; }, dev);
            ok &= expect("too many filters", BAD, nothing, [](Call& c) { c.fl.n_filters = 0x40000000u; }, dev);
            ok &= expect("null ranges", PHANT_OK, nothing, [](Call& c) { c.fl.block_lo = c.fl.block_hi = nullptr; }, dev);
            ok &= expect("null block_lo", PHANT_OK, nothing, [](Call& c) { c.fl.block_lo = nullptr; }, dev);
            ok &= expect("odd addr_first", dev ? BAD : PHANT_OK, nothing,
                         [&](Call& c) { if (dev) c.fl.addr_first = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(c.fl.addr_first) + 2); }, dev);
            ok &= expect("odd block_hi", dev ? BAD : PHANT_OK, nothing,
                         [&](Call& c) { if (dev) c.fl.block_hi = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(c.fl.block_hi) + 1); }, dev);
            if (bloom) {
                ok &= expect("odd may", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.may = reinterpret_cast<uint64_t*>(uintptr_t(0x1004)); }, dev);
                ok &= expect("odd may_count", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.may_count = reinterpret_cast<uint32_t*>(uintptr_t(0x1002)); }, dev);
                ok &= expect("null blooms", BAD, nothing, [](Call& c) { c.p_bl.reset(); }, dev);
                continue;
            }
            ok &= expect("in size", BAD, nothing, [](Call& c) { c.in.struct_size += 8; }, dev);
            ok &= expect("out size", BAD, nothing, [](Call& c) { c.out.struct_size -= 8; }, dev);
            ok &= expect("reserved", BAD, nothing, [](Call& c) { c.in.reserved = 1; }, dev);
            ok &= expect("reserved2", BAD, nothing, [](Call& c) { c.in.reserved2 = 1; }, dev);
            ok &= expect("out reserved", BAD, nothing, [](Call& c) { c.out.reserved = 1; }, dev);
            ok &= expect("out reserved2", BAD, nothing, [](Call& c) { c.out.reserved2 = 1; }, dev);
            ok &= expect("null block_first", BAD, nothing, [](Call& c) { c.in.block_first = nullptr; }, dev);
            ok &= expect("null log_first", BAD, nothing, [](Call& c) { c.in.log_first = nullptr; }, dev);
            ok &= expect("null address", BAD, nothing, [](Call& c) { c.in.address = nullptr; }, dev);
            ok &= expect("null topic_first", BAD, nothing, [](Call& c) { c.in.topic_first = nullptr; }, dev);
            ok &= expect("null topics", BAD, nothing, [](Call& c) { c.in.topics = nullptr; }, dev);
            ok &= expect("no block, rows", BAD, nothing, [](Call& c) { c.in.n_blocks = 0; }, dev);
            ok &= expect("no block", dev ? PHANT_OK : BAD, nothing, [](Call& c) { c.in.n_blocks = c.in.n = c.in.n_logs = c.in.n_topics = 0, c.in.block_first = nullptr; }, dev);  // (host: block_hi above 0)
            ok &= expect("no block, no ranges", PHANT_OK, [](Call& c) { c.block_lo = {0, 0}, c.block_hi = {0, 0}; },
                         [](Call& c) { c.in.n_blocks = c.in.n = c.in.n_logs = c.in.n_topics = 0, c.in.block_first = nullptr; }, dev);
            ok &= expect("logs without a receipt", BAD, [](Call& c) { c.block_first = {0, 0, 0, 0}, c.log_first = {0}; }, [](Call& c) { c.in.n = 0; }, dev);
            ok &= expect("topics without a log", BAD, [](Call& c) { c.log_first = {0, 0, 0, 0, 0, 0}; }, [](Call& c) { c.in.n_logs = 0; }, dev);
            ok &= expect("odd block_first", dev ? BAD : PHANT_OK, nothing,
                         [&](Call& c) { if (dev) c.in.block_first = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(c.in.block_first) + 2); }, dev);
            ok &= expect("odd match_log", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.out.match_log = reinterpret_cast<uint32_t*>(uintptr_t(0x1001)); }, dev);
        }
        // the host form's firsts: each entry one up, one down
        for (int which = bloom ? 3 : 0; which < 5; ++which) {
            Call shape;
            const size_t len = (which == 0 ? shape.block_first : which == 1 ? shape.log_first : which == 2 ? shape.topic_first : which == 3 ? shape.addr_first : shape.ftopic_first).size();
            for (size_t at = 0; at < len; ++at)
                for (const int by : {-1, 1}) {
                    auto pick = [&](Call& c) -> std::vector<uint32_t>& {
                        return which == 0 ? c.block_first : which == 1 ? c.log_first : which == 2 ? c.topic_first : which == 3 ? c.addr_first : c.ftopic_first;
                    };
                    auto lie = [&](Call& c) { pick(c)[at] += (uint32_t)by; };
                    Call probe;
                    lie(probe);
                    const std::vector<uint32_t>& v = pick(probe);
                    const uint32_t total = which == 0 ? 5 : which == 1 ? 4 : which == 2 ? 5 : which == 3 ? 3 : 4;
                    bool fine = v.front() == 0 && v.back() == total;
                    for (size_t k = 0; k + 1 < v.size(); ++k) fine = fine && v[k] <= v[k + 1];
                    // (a moved first of the filters that stays legal moves an entry between sets: the sets above two entries change)
                    if (fine && which >= 3) continue;
                    ok &= expect("a first moved", fine ? PHANT_OK : BAD, lie, nothing);
                }
        }
        ok &= expect("lo above hi", BAD, [](Call& c) { c.block_lo[1] = 3; }, nothing);
        ok &= expect("hi above the blocks", BAD, [](Call& c) { c.block_hi[0] = 4; }, nothing);
        ok &= expect("lo == hi", PHANT_OK, [](Call& c) { c.block_lo[0] = 3; }, nothing);
        ok &= expect("lo above the blocks, null hi", BAD, [](Call& c) { c.block_lo[1] = 4; }, [](Call& c) { c.fl.block_hi = nullptr; });
        ok &= expect("n_addr one less", BAD, nothing, [](Call& c) { c.fl.n_addr -= 1; });
        ok &= expect("n_topic one more", BAD, nothing, [](Call& c) { c.fl.n_topic += 1; });
        if (bloom) continue;
        ok &= expect("n one less", BAD, nothing, [](Call& c) { c.in.n -= 1; });
        ok &= expect("n_logs one more", BAD, nothing, [](Call& c) { c.in.n_logs += 1; });
        ok &= expect("n_topics one less", BAD, nothing, [](Call& c) { c.in.n_topics -= 1; });
    }
    if (!phant::lf::too_many_words(1u << 25, 4096) || phant::lf::too_many_words((1u << 25) - 1u, 4096) || phant::lf::too_many_words(0x3fffffffu, 0)) ok = false, std::printf("too_many_words\n");
    std::printf("%u cases: %u refused, %u accepted\n", cases, refused, accepted);
    return ok ? 0 : 1;
}
