// rlp_main.cpp -- TEST INFRASTRUCTURE: phant_amd/csrc/rlp.h as a stand-alone host program (tests/test_rlp_native.py builds it with
// g++ under AddressSanitizer + UBSan and runs it as a child process).  It reads records the test wrote, each with the bytes the test's
// own encoder / decoder expects, and holds rlp.h against them:
//   record = kind u8, a u64, b u64, in_len u32, exp_len u32, in bytes, exp bytes            (little-endian)
//     'h'  put_hdr(base = a, payload = b) == exp, hdr_len(b) == the count, put_hdr_to writes the same bytes
//     'u'  put_uint(a) == exp, uint_len(a) == the count, uint_bytes(a) == b
//     's'  put_str(in) == exp, str_len(in_len, in[0]) == the count
//     'm'  put_minimal(in, in_len) == exp, be_bytes(in, in_len) == a
//     'd'  rlp_decode(in) with 32-bit and with size_t offsets, at offset 0 and behind one more byte: accepted == a, and then
//          (pay, len, total, is_list) == exp (four u64)
// Every input and every output lives in a heap block of exactly its size, so a read or a write beyond it stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../phant_amd/csrc/rlp.h"

namespace {

uint64_t get(const uint8_t* p, int n) {
    uint64_t v = 0;
    for (int i = n - 1; i >= 0; --i) v = v << 8 | p[i];
    return v;
}

[[noreturn]] void fail(size_t rec, char kind, const char* what) {
    std::fprintf(stderr, "record %zu ('%c'): %s\n", rec, kind, what);
    std::exit(1);
}

// a heap block of exactly n bytes holding p[0, n)
uint8_t* exact(const uint8_t* p, size_t n) {
    uint8_t* q = (uint8_t*)std::malloc(n);
    if (n) std::memcpy(q, p, n);
    return q;
}

template <class Off>
bool decode_as(const uint8_t* in, size_t n, size_t lead, uint64_t out[4]) {
    // `lead` bytes in front of the item: the decoder starts at offset lead with n bytes left
    uint8_t* const buf = (uint8_t*)std::malloc(lead + n);
    std::memset(buf, 0xee, lead);
    if (n) std::memcpy(buf + lead, in, n);
    phant::RlpItemOf<Off> it;
    const bool ok = phant::rlp_decode(phant::MemBytes{buf}, (Off)lead, (Off)n, it);
    if (ok) out[0] = it.pay - lead, out[1] = it.len, out[2] = it.total, out[3] = it.is_list;
    std::free(buf);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
    std::fclose(f);
    size_t at = 0, rec = 0, written = 0, accepted = 0, refused = 0;
    while (at < file.size()) {
        if (file.size() - at < 25) fail(rec, '?', "short record");
        const char kind = (char)file[at];
        const uint64_t a = get(&file[at + 1], 8), b = get(&file[at + 9], 8);
        const size_t in_len = get(&file[at + 17], 4), exp_len = get(&file[at + 21], 4);
        at += 25;
        if (file.size() - at < in_len + exp_len) fail(rec, kind, "short record");
        uint8_t* const in = exact(file.data() + at, in_len);
        const uint8_t* const exp = file.data() + at + in_len;
        at += in_len + exp_len;
        if (kind == 'd') {
            uint64_t r32[4] = {0, 0, 0, 0}, r64[4] = {0, 0, 0, 0};
            for (size_t lead = 0; lead < 2; ++lead) {
                const bool ok32 = decode_as<uint32_t>(in, in_len, lead, r32), ok64 = decode_as<size_t>(in, in_len, lead, r64);
                if (ok32 != ok64) fail(rec, kind, "the two offset types disagree on the verdict");
                if (ok32 != (a != 0)) fail(rec, kind, ok32 ? "accepted, expected refused" : "refused, expected accepted");
                if (!ok32) continue;
                if (exp_len != 32) fail(rec, kind, "bad record");
                for (int k = 0; k < 4; ++k) {
                    if (r32[k] != r64[k]) fail(rec, kind, "the two offset types disagree on the item");
                    if (r32[k] != get(exp + 8 * k, 8)) fail(rec, kind, "pay / len / total / is_list differ from the expected item");
                }
            }
            ++(a ? accepted : refused);
        } else {
            uint8_t* const out = (uint8_t*)std::malloc(exp_len);
            uint64_t count = 0, len = 0;
            if (kind == 'h') {
                count = phant::put_hdr(out, (uint32_t)a, b), len = phant::hdr_len(b);
                uint8_t* const out2 = (uint8_t*)std::malloc(exp_len);
                if (phant::put_hdr_to(out2, (uint32_t)a, b) != out2 + count || std::memcmp(out2, out, count) != 0) fail(rec, kind, "put_hdr_to");
                std::free(out2);
            } else if (kind == 'u') {
                count = phant::put_uint(out, a), len = phant::uint_len(a);
                if (phant::uint_bytes(a) != b) fail(rec, kind, "uint_bytes");
            } else if (kind == 's') {
                count = phant::put_str(out, in, (uint32_t)in_len), len = phant::str_len(in_len, in_len ? in[0] : 0u);
            } else if (kind == 'm') {
                count = phant::put_minimal(out, in, (uint32_t)in_len), len = count;
                if (phant::be_bytes(in, (uint32_t)in_len) != a) fail(rec, kind, "be_bytes");
                if (phant::str_len(a, in_len ? in[in_len - 1] : 0u) != count) fail(rec, kind, "str_len of the significant bytes");
            } else {
                fail(rec, kind, "unknown kind");
            }
            if (count != exp_len) fail(rec, kind, "the writer's count differs from the expected length");
            if (len != count) fail(rec, kind, "the length function differs from the writer's count");
            if (std::memcmp(out, exp, exp_len) != 0) fail(rec, kind, "bytes differ");
            std::free(out);
            ++written;
        }
        std::free(in);
        ++rec;
    }
    std::printf("%zu written, %zu accepted, %zu refused\n", written, accepted, refused);
    return 0;
}
