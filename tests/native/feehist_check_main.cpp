// feehist_check_main.cpp -- the host-side checks of phant_block_fee_history (phant_amd/csrc/feehist_check.h: check_args, check_percentiles,
// check_rows_host, too_many_rewards, block_max_of, reaches) and wide_uint.h's mul_small as a stand-alone program under AddressSanitizer +
// UBSan.  Every array lives in an allocation of exactly its entries, so a check that reads an entry too far is caught; a case is a good
// call with one thing wrong, and each must be refused (or accepted) as include/phant_gpu.h says.  Prints how many cases were refused and
// how many accepted; tests/test_feehist_check_native.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../phant_amd/csrc/feehist_check.h"

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// four blocks of 2, 0, 3 and 1 rows; three percentiles
struct Call {
    std::vector<uint32_t> block_first{0, 2, 2, 5, 6}, percentile{10000, 0, 5000};
    std::vector<uint64_t> gas_used{21000, 1, 0, ~0ull, 5, 6};
    std::vector<uint8_t> price = std::vector<uint8_t>(6 * 32, 0x11), base_fee = std::vector<uint8_t>(4 * 32, 0x01);
    phant_fee_history_in in;
    phant_fee_history_out out;
    std::unique_ptr<uint32_t[]> p_bf, p_pc;
    std::unique_ptr<uint64_t[]> p_gu;
    std::unique_ptr<uint8_t[]> p_pr, p_ba;
    uint32_t block_max = PHANT_FEEHIST_BLOCK_MAX;

    void bind() {
        p_bf = exact(block_first), p_pc = exact(percentile), p_gu = exact(gas_used), p_pr = exact(price), p_ba = exact(base_fee);
        std::memset(&in, 0, sizeof in);
        std::memset(&out, 0, sizeof out);
        in.struct_size = sizeof in, out.struct_size = sizeof out;
        in.n_blocks = (uint32_t)block_first.size() - 1, in.n = (uint32_t)gas_used.size(), in.n_percentiles = (uint32_t)percentile.size();
        in.block_first = p_bf.get(), in.price = p_pr.get(), in.base_fee = p_ba.get(), in.gas_used = p_gu.get(), in.percentile = p_pc.get();
    }
};

// PHANT_OK or the code the call answers before anything is copied
int32_t verdict(const Call& c, bool dev) {
    if (*phant::fh::check_args(&c.in, &c.out, dev)) return PHANT_E_INVALID_ARG;
    if (*phant::fh::check_percentiles(c.in)) return PHANT_E_INVALID_ARG;
    if (c.in.n_blocks == 0) return PHANT_OK;
    if (phant::fh::too_many_rewards(c.in.n_blocks, c.in.n_percentiles)) return PHANT_E_UNSUPPORTED;
    if (dev) return PHANT_OK;
    std::string err;
    const int32_t rc = phant::fh::check_rows_host("call", c.in, c.block_max, err);
    if ((rc != PHANT_OK) != !err.empty()) return 100;  // (a refusal says why)
    return rc;
}

typedef unsigned __int128 u128;

bool arithmetic() {
    bool ok = true;
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto next = [&] { return x ^= x << 13, x ^= x >> 7, x ^= x << 17, x; };
    const uint32_t edge[] = {0u, 1u, 2u, 9999u, 10000u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    for (int it = 0; it < 20000; ++it) {
        // mul_small<4> against the compiler's 128 bits, modulo 2^128; <3> and <1> are its low limbs
        const u128 v = it < 64 ? ((u128)edge[it & 7] << 96 | (u128)edge[it >> 3 & 7] << 32 | 0xffffffffu) : ((u128)next() << 64 | next());
        const uint32_t m = it < 64 ? edge[(it * 5) & 7] : (uint32_t)next();
        uint32_t a[4] = {(uint32_t)v, (uint32_t)(v >> 32), (uint32_t)(v >> 64), (uint32_t)(v >> 96)}, b[3] = {a[0], a[1], a[2]}, c[1] = {a[0]};
        phant::wide::mul_small<4>(a, m);
        phant::wide::mul_small<3>(b, m);
        phant::wide::mul_small<1>(c, m);
        const u128 w = v * m;
        if (a[0] != (uint32_t)w || a[1] != (uint32_t)(w >> 32) || a[2] != (uint32_t)(w >> 64) || a[3] != (uint32_t)(w >> 96) || b[0] != a[0] || b[1] != a[1] ||
            b[2] != a[2] || c[0] != a[0])
            ok = false, std::printf("mul_small %d\n", it);
    }
    // reaches(S, G, p) == (S >= floor(G p / 10000)) over 96-bit S and G: the corners, and sums at the threshold of random G
    const uint32_t ps[] = {0u, 1u, 4999u, 5000u, 9999u, 10000u};
    const u128 top = ((u128)1 << 96) - 1;
    for (const uint32_t p : ps)
        for (int it = 0; it < 6000; ++it) {
            u128 G = ((u128)next() << 64 | next()) & top, S;
            if (it < 4) G = it & 1 ? top : it >> 1;
            const u128 t = G * p / 10000u;
            switch (it % 4) {
                case 0: S = t; break;
                case 1: S = t ? t - 1 : 0; break;
                case 2: S = t < top ? t + 1 : top; break;
                default: S = ((u128)next() << 64 | next()) & top;
            }
            const uint32_t s[3] = {(uint32_t)S, (uint32_t)(S >> 32), (uint32_t)(S >> 64)}, g[3] = {(uint32_t)G, (uint32_t)(G >> 32), (uint32_t)(G >> 64)};
            if (phant::fh::reaches(s, g, p) != (S >= t)) ok = false, std::printf("reaches %u %d\n", p, it);
        }
    if (!phant::fh::too_many_rewards(1u << 16, 1u << 15) || phant::fh::too_many_rewards((1u << 16) - 1u, 1u << 15) || phant::fh::too_many_rewards(0xffffffffu, 0)) ok = false, std::printf("too_many_rewards\n");
    if (phant::fh::block_max_of(0) != PHANT_FEEHIST_BLOCK_MAX || phant::fh::block_max_of(-5) != PHANT_FEEHIST_BLOCK_MAX || phant::fh::block_max_of(257) != 257u ||
        phant::fh::block_max_of(65535) != 65535u || phant::fh::block_max_of(65536) != PHANT_FEEHIST_BLOCK_MAX || phant::fh::block_max_of(1ll << 40) != PHANT_FEEHIST_BLOCK_MAX)
        ok = false, std::printf("block_max_of\n");
    return ok;
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
    auto odd = [](auto*& p, int by) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(p) + by); };
    const int32_t BAD = PHANT_E_INVALID_ARG, UNS = PHANT_E_UNSUPPORTED;
    bool ok = true;
    for (const bool dev : {false, true}) {
        ok &= expect("good", PHANT_OK, nothing, nothing, dev);
        ok &= expect("in size up", BAD, nothing, [](Call& c) { c.in.struct_size += 8; }, dev);
        ok &= expect("in size down", BAD, nothing, [](Call& c) { c.in.struct_size -= 8; }, dev);
        ok &= expect("out size up", BAD, nothing, [](Call& c) { c.out.struct_size += 8; }, dev);
        ok &= expect("out size down", BAD, nothing, [](Call& c) { c.out.struct_size -= 8; }, dev);
        ok &= expect("in reserved", BAD, nothing, [](Call& c) { c.in.reserved = 1; }, dev);
        ok &= expect("out reserved", BAD, nothing, [](Call& c) { c.out.reserved = 1ull << 40; }, dev);
        ok &= expect("null block_first", BAD, nothing, [](Call& c) { c.in.block_first = nullptr; }, dev);
        ok &= expect("null price", BAD, nothing, [](Call& c) { c.in.price = nullptr; }, dev);
        ok &= expect("null gas_used", BAD, nothing, [](Call& c) { c.in.gas_used = nullptr; }, dev);
        ok &= expect("null percentile", BAD, nothing, [](Call& c) { c.in.percentile = nullptr; }, dev);
        ok &= expect("null base_fee", PHANT_OK, nothing, [](Call& c) { c.in.base_fee = nullptr; }, dev);
        ok &= expect("no percentile", PHANT_OK, nothing, [](Call& c) { c.in.n_percentiles = 0, c.in.percentile = nullptr; }, dev);
        ok &= expect("rows without a block", BAD, nothing, [](Call& c) { c.in.n_blocks = 0; }, dev);
        ok &= expect("no block", PHANT_OK, nothing, [](Call& c) { c.in.n_blocks = c.in.n = 0, c.in.block_first = nullptr, c.in.price = nullptr, c.in.gas_used = nullptr; }, dev);
        ok &= expect("no row", PHANT_OK, [](Call& c) { c.block_first = {0, 0, 0, 0, 0}, c.gas_used = {}, c.price = {}; }, [](Call& c) { c.in.price = nullptr, c.in.gas_used = nullptr; }, dev);
        for (size_t k = 0; k < 3; ++k) {
            ok &= expect("a percentile of 10001", BAD, [k](Call& c) { c.percentile[k] = 10001u; }, nothing, dev);
            ok &= expect("a percentile of 2^32 - 1", BAD, [k](Call& c) { c.percentile[k] = 0xffffffffu; }, nothing, dev);
            ok &= expect("a percentile of 10000", PHANT_OK, [k](Call& c) { c.percentile[k] = 10000u; }, nothing, dev);
        }
        ok &= expect("too many rewards", UNS, nothing, [](Call& c) { c.in.n_blocks = 1u << 30; }, dev);  // (refused from the counts: block_first is not read)
        ok &= expect("odd block_first", dev ? BAD : PHANT_OK, nothing, [&](Call& c) { if (dev) odd(c.in.block_first, 2); }, dev);
        ok &= expect("odd gas_used", dev ? BAD : PHANT_OK, nothing, [&](Call& c) { if (dev) odd(c.in.gas_used, 4); }, dev);
        ok &= expect("odd order", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.out.order = reinterpret_cast<uint32_t*>(uintptr_t(0x1002)); }, dev);
        ok &= expect("odd block_flags", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.out.block_flags = reinterpret_cast<uint32_t*>(uintptr_t(0x1001)); }, dev);
        ok &= expect("odd block_gas_used", dev ? BAD : PHANT_OK, nothing, [](Call& c) { c.out.block_gas_used = reinterpret_cast<uint64_t*>(uintptr_t(0x1004)); }, dev);
        ok &= expect("odd reward and tip", PHANT_OK, nothing, [](Call& c) { c.out.reward = reinterpret_cast<uint8_t*>(uintptr_t(0x1001)), c.out.tip = reinterpret_cast<uint8_t*>(uintptr_t(0x1003)); }, dev);
        ok &= expect("odd price and base_fee", PHANT_OK, [](Call& c) { c.price.push_back(0), c.base_fee.push_back(0); }, [&](Call& c) { odd(c.in.price, 1), odd(c.in.base_fee, 1); }, dev);
    }
    // the host form's block_first: each entry one up, one down
    {
        Call shape;
        for (size_t at = 0; at < shape.block_first.size(); ++at)
            for (const int by : {-1, 1}) {
                auto lie = [&](Call& c) { c.block_first[at] += (uint32_t)by; };
                Call probe;
                lie(probe);
                const std::vector<uint32_t>& v = probe.block_first;
                bool fine = v.front() == 0 && v.back() == 6;
                for (size_t k = 0; k + 1 < v.size(); ++k) fine = fine && v[k] <= v[k + 1];
                ok &= expect("a first moved", fine ? PHANT_OK : BAD, lie, nothing);
            }
    }
    ok &= expect("n one less", BAD, nothing, [](Call& c) { c.in.n -= 1; });
    ok &= expect("n one more", BAD, nothing, [](Call& c) { c.in.n += 1; });
    // the cap: a block of exactly the cap is answered, one row more is unsupported; an invalid block_first wins over the cap
    ok &= expect("cap 3", PHANT_OK, [](Call& c) { c.block_max = 3; }, nothing);
    ok &= expect("cap 2", UNS, [](Call& c) { c.block_max = 2; }, nothing);
    ok &= expect("cap 1", UNS, [](Call& c) { c.block_max = 1; }, nothing);
    ok &= expect("cap 2, backwards", BAD, [](Call& c) { c.block_max = 2, c.block_first[1] = 6; }, nothing);
    ok &= arithmetic();
    std::printf("%u cases: %u refused, %u accepted\n", cases, refused, accepted);
    return ok ? 0 : 1;
}
