// TEST INFRASTRUCTURE: phant_witness_to_json's host code (witness_json.cpp: witness_to_json) as a stand-alone program, built by
// tests/test_witness_write_native.py with -fsanitize=address,undefined.  For every document named on the command line:
// parse -> write -> parse, and the two witnesses must be the same object member by member; the text is written into heap buffers
// of exactly the needed size (a byte more written would be a heap overflow the sanitizer reports) and of one byte less (nothing
// may be written); the index form of the same document is refused.  Prints "<n> documents, <p> proofs, <b> bytes written".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>

#include "witness.h"

using phant::Witness;

static int fail(const char* file, const char* what) {
    std::fprintf(stderr, "%s: %s\n", file, what);
    return 1;
}

template <class V>
static bool same(const V& a, const V& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

static bool same_witness(const Witness& a, const Witness& b, const char*& what) {
    if (!same(a.roots, b.roots)) return what = "roots", false;
    if (!same(a.root_idx, b.root_idx)) return what = "root_idx", false;
    if (!same(a.account_of, b.account_of)) return what = "account_of", false;
    if (!same(a.preimages, b.preimages)) return what = "preimages", false;
    if (!same(a.preimage_off, b.preimage_off)) return what = "preimage_off", false;
    if (!same(a.nodes, b.nodes)) return what = "nodes", false;
    if (!same(a.node_off, b.node_off)) return what = "node_off", false;
    if (!same(a.proof_first_node, b.proof_first_node)) return what = "proof_first_node", false;
    if (a.node_set != b.node_set || a.deferred != b.deferred) return what = "form", false;
    if (a.accounts.size() != b.accounts.size() || a.slots.size() != b.slots.size()) return what = "counts", false;
    for (size_t i = 0; i < a.accounts.size(); ++i) {
        const phant::WitnessAccount &x = a.accounts[i], &y = b.accounts[i];
        if (std::memcmp(x.address, y.address, 20) || std::memcmp(x.storage_hash, y.storage_hash, 32) || x.proof != y.proof ||
            x.has_storage_hash != y.has_storage_hash || x.has_code_hash != y.has_code_hash || x.has_balance != y.has_balance ||
            x.has_nonce != y.has_nonce)
            return what = "account", false;
        if ((x.has_code_hash && std::memcmp(x.code_hash, y.code_hash, 32)) || (x.has_balance && std::memcmp(x.balance, y.balance, 32)) ||
            (x.has_nonce && x.nonce != y.nonce))
            return what = "account declaration", false;
    }
    for (size_t i = 0; i < a.slots.size(); ++i) {
        const phant::WitnessSlot &x = a.slots[i], &y = b.slots[i];
        if (x.proof != y.proof || x.account != y.account || x.has_value != y.has_value || (x.has_value && std::memcmp(x.value, y.value, 32)))
            return what = "slot", false;
    }
    return true;
}

int main(int argc, char** argv) {
    size_t proofs = 0, bytes = 0;
    for (int k = 1; k < argc; ++k) {
        std::ifstream in(argv[k], std::ios::binary);
        std::stringstream ss;
        ss << in.rdbuf();
        const std::string doc = ss.str();
        Witness first, second, index;
        std::string err;
        if (!phant::witness_parse_json(doc.data(), doc.size(), first, err)) return fail(argv[k], err.c_str());
        // the needed length, with no buffer at all
        uint64_t need = 0;
        if (!phant::witness_to_json(first, nullptr, 0, need) || need == 0) return fail(argv[k], "no length reported");
        // one byte less: the length again, nothing written
        {
            std::unique_ptr<char[]> small(new char[need - 1 ? need - 1 : 1]);
            std::memset(small.get(), 0x5a, need - 1);
            uint64_t len = 0;
            if (!phant::witness_to_json(first, small.get(), need - 1, len) || len != need) return fail(argv[k], "short buffer: wrong length");
            for (uint64_t i = 0; i + 1 < need; ++i)
                if (small[i] != 0x5a) return fail(argv[k], "short buffer: written to");
        }
        // exactly the needed size
        std::unique_ptr<char[]> text(new char[need]);
        uint64_t len = 0;
        if (!phant::witness_to_json(first, text.get(), need, len) || len != need) return fail(argv[k], "exact buffer: wrong length");
        if (!phant::witness_parse_json(text.get(), need, second, err)) return fail(argv[k], ("the written text does not parse: " + err).c_str());
        const char* what = "";
        if (!same_witness(first, second, what)) return fail(argv[k], what);
        // written a second time from the parsed copy: the same text (the writer is a function of the witness alone)
        std::string again;
        if (!phant::witness_to_json(second, again) || again.size() != need || std::memcmp(again.data(), text.get(), need) != 0)
            return fail(argv[k], "the second writing differs");
        // the threaded parser reads the written text to the same witness
        Witness mt;
        if (!phant::witness_parse_json_mt(text.get(), need, 3, mt, err) || !same_witness(first, mt, what)) return fail(argv[k], "threaded parse differs");
        // the index form holds no decoded nodes: refused, length 0
        if (!phant::witness_index_json(doc.data(), doc.size(), 1, index, err)) return fail(argv[k], err.c_str());
        uint64_t none = 77;
        if (phant::witness_to_json(index, nullptr, 0, none) || none != 0) return fail(argv[k], "the index form was not refused");
        proofs += first.root_idx.size();
        bytes += need;
    }
    std::printf("%d documents, %zu proofs, %zu bytes written\n", argc - 1, proofs, bytes);
    return 0;
}
