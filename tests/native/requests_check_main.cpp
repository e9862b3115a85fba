// requests_check_main.cpp -- the host-side checks of phant_block_requests (phant_amd/csrc/requests_check.h: check_args, check_host; the
// firsts and offsets rules of segment_checks.h) as a stand-alone program under AddressSanitizer + UBSan.  Every array lives in an
// allocation of exactly its entries, so a check that reads an entry too far is caught; a case is a good call with one thing wrong, and
// each must be refused (or accepted) as include/phant_gpu.h says.  Prints how many cases were refused and how many accepted;
// tests/test_requests_check_native.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../phant_amd/csrc/requests_check.h"

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// three blocks of 2, 0 and 3 receipts; 4 logs, 5 topics; 3 rows of the caller's
struct Call {
    std::vector<uint32_t> block_first{0, 2, 2, 5}, log_first{0, 2, 2, 3, 4, 4}, topic_first{0, 1, 1, 3, 5}, data_len{576, 3, 0, 576}, req_block_first{0, 1, 1, 3};
    std::vector<uint64_t> data_at{10, 600, 700, 800}, req_off{0, 2, 3, 7};
    std::vector<uint8_t> address = std::vector<uint8_t>(80, 0x11), topics = std::vector<uint8_t>(160, 0x22), receipts = std::vector<uint8_t>(1400, 0x33);
    std::vector<uint8_t> req_type{1, 1, 2}, req_bytes = std::vector<uint8_t>(7, 0x44);
    phant_requests_in in;
    phant_requests_out out;
    std::unique_ptr<uint32_t[]> p_bf, p_lf, p_tf, p_dl, p_rbf;
    std::unique_ptr<uint64_t[]> p_da, p_ro;
    std::unique_ptr<uint8_t[]> p_ad, p_tp, p_rc, p_rt, p_rb;

    void bind() {
        p_bf = exact(block_first), p_lf = exact(log_first), p_tf = exact(topic_first), p_dl = exact(data_len), p_rbf = exact(req_block_first);
        p_da = exact(data_at), p_ro = exact(req_off), p_ad = exact(address), p_tp = exact(topics), p_rc = exact(receipts), p_rt = exact(req_type), p_rb = exact(req_bytes);
        std::memset(&in, 0, sizeof in);
        std::memset(&out, 0, sizeof out);
        in.struct_size = sizeof in, out.struct_size = sizeof out;
        in.n_blocks = (uint32_t)block_first.size() - 1, in.n = (uint32_t)log_first.size() - 1, in.n_logs = (uint32_t)data_at.size(), in.n_topics = (uint32_t)topics.size() / 32;
        in.n_req = (uint32_t)req_type.size(), in.deposit_cap = 4, in.rc_bytes = receipts.size(), in.req_total = req_bytes.size();
        in.receipts = p_rc.get(), in.block_first = p_bf.get(), in.log_first = p_lf.get(), in.address = p_ad.get(), in.topic_first = p_tf.get(), in.topics = p_tp.get();
        in.data_at = p_da.get(), in.data_len = p_dl.get(), in.req_block_first = p_rbf.get(), in.req_type = p_rt.get(), in.req_bytes = p_rb.get(), in.req_off = p_ro.get();
    }
};

// PHANT_OK or the code the host form answers before anything is copied
int32_t verdict(const Call& c, bool dev) {
    const char* const what = phant::qreq::check_args(&c.in, &c.out, dev);
    if (*what) return PHANT_E_INVALID_ARG;
    if (c.in.n_blocks == 0 || dev) return PHANT_OK;
    std::string err;
    const int32_t rc = phant::qreq::check_host(c.in, err);
    if ((rc != PHANT_OK) != !err.empty()) return 100;  // (a refusal says why)
    return rc;
}

}  // namespace

int main() {
    unsigned refused = 0, accepted = 0, cases = 0;
    auto expect = [&](const char* name, int32_t want, const std::function<void(Call&)>& before, const std::function<void(Call&)>& after, bool dev = false) {
        Call c;
        before(c);
        c.bind();
        after(c);
        const int32_t got = verdict(c, dev);
        ++cases, ++(got == PHANT_OK ? accepted : refused);
        if (got != want) std::printf("case %s (%s form): %d, expected %d\n", name, dev ? "device" : "host", got, want);
        return got == want;
    };
    auto nothing = [](Call&) {};
    bool ok = true;
    for (const bool dev : {false, true}) {
        ok &= expect("good", PHANT_OK, nothing, nothing, dev);
        ok &= expect("in size", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.struct_size += 8; }, dev);
        ok &= expect("out size", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.out.struct_size -= 8; }, dev);
        ok &= expect("reserved", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.reserved = 1; }, dev);
        ok &= expect("out reserved", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.out.reserved = 1; }, dev);
        ok &= expect("null block_first", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.block_first = nullptr; }, dev);
        ok &= expect("null log_first", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.log_first = nullptr; }, dev);
        ok &= expect("null address", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.address = nullptr; }, dev);
        ok &= expect("null topic_first", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.topic_first = nullptr; }, dev);
        ok &= expect("null topics", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.topics = nullptr; }, dev);
        ok &= expect("null data_at", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.data_at = nullptr; }, dev);
        ok &= expect("null data_len", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.data_len = nullptr; }, dev);
        ok &= expect("null receipts", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.receipts = nullptr; }, dev);
        ok &= expect("null req_block_first", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.req_block_first = nullptr; }, dev);
        ok &= expect("null req_type", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.req_type = nullptr; }, dev);
        ok &= expect("null req_off", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.req_off = nullptr; }, dev);
        ok &= expect("null req_bytes", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.req_bytes = nullptr; }, dev);
        ok &= expect("no block, rows", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.n_blocks = 0; }, dev);
        ok &= expect("no block", PHANT_OK, nothing, [](Call& c) { c.in.n_blocks = c.in.n = c.in.n_logs = c.in.n_topics = c.in.n_req = 0, c.in.block_first = nullptr; }, dev);
        ok &= expect("no requests, null arrays", PHANT_OK, nothing, [](Call& c) { c.in.n_req = 0, c.in.req_block_first = nullptr, c.in.req_type = nullptr, c.in.req_bytes = nullptr, c.in.req_off = nullptr; }, dev);
        ok &= expect("logs without a receipt", PHANT_E_INVALID_ARG, [](Call& c) { c.block_first = {0, 0, 0, 0}, c.log_first = {0}; }, [](Call& c) { c.in.n = 0; }, dev);
        ok &= expect("topics without a log", PHANT_E_INVALID_ARG, [](Call& c) { c.log_first = {0, 0, 0, 0, 0, 0}; }, [](Call& c) { c.in.n_logs = 0; }, dev);
    }
    // the device form's alignment
    ok &= expect("odd data_at", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.data_at = reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(c.in.data_at) + 4); }, true);
    ok &= expect("odd block_first", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.block_first = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(c.in.block_first) + 2); }, true);
    ok &= expect("odd block_flags", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.out.block_flags = reinterpret_cast<uint32_t*>(uintptr_t(0x1001)); }, true);
    ok &= expect("odd deposit", PHANT_OK, nothing, [](Call& c) { c.out.deposit = reinterpret_cast<uint8_t*>(uintptr_t(0x1001)); }, true);
    // the host form's firsts and offsets: each entry one up, one down, and the totals
    for (int which = 0; which < 4; ++which) {
        const size_t len = which == 0 ? 4 : which == 1 ? 6 : which == 2 ? 5 : 4;
        for (size_t at = 0; at < len; ++at)
            for (const int by : {-1, 1}) {
                auto lie = [&](Call& c) {
                    std::vector<uint32_t>& v = which == 0 ? c.block_first : which == 1 ? c.log_first : which == 2 ? c.topic_first : c.req_block_first;
                    v[at] += (uint32_t)by;
                };
                Call probe;
                lie(probe);
                const std::vector<uint32_t>& v = which == 0 ? probe.block_first : which == 1 ? probe.log_first : which == 2 ? probe.topic_first : probe.req_block_first;
                const uint32_t total = which == 0 ? 5 : which == 1 ? 4 : which == 2 ? 5 : 3;
                bool fine = v.front() == 0 && v.back() == total;
                for (size_t k = 0; k + 1 < v.size(); ++k) fine = fine && v[k] <= v[k + 1];
                ok &= expect("a first moved", fine ? PHANT_OK : PHANT_E_INVALID_ARG, lie, nothing);
            }
    }
    ok &= expect("req_off from 1", PHANT_E_INVALID_ARG, [](Call& c) { c.req_off[0] = 1; }, nothing);
    ok &= expect("req_off backwards", PHANT_E_INVALID_ARG, [](Call& c) { c.req_off[1] = 4; }, nothing);
    ok &= expect("req_off, a shorter last row", PHANT_OK, [](Call& c) { c.req_off[3] = 6; }, nothing);
    ok &= expect("a request of 4 GiB", PHANT_E_UNSUPPORTED, [](Call& c) { c.req_off[3] += 1ull << 32; }, nothing);
    ok &= expect("n one less", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.n -= 1; });
    ok &= expect("n_logs one more", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.n_logs += 1; });
    ok &= expect("n_topics one less", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.n_topics -= 1; });
    ok &= expect("n_req one less", PHANT_E_INVALID_ARG, nothing, [](Call& c) { c.in.n_req -= 1; });
    std::printf("%u cases: %u refused, %u accepted\n", cases, refused, accepted);
    return ok ? 0 : 1;
}
