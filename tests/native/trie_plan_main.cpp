// trie_plan_main.cpp -- phant_amd/csrc/trie_plan.h alone: what the trie hasher's launcher chooses, held to numbers written out here
// (none is computed from the header's constants).  Every depth bin's launch -- class, grid and block of the main launch and of the
// fallback pass -- at the sizes where the rules change, under every knob that moves it; the pass; the min-tree's levels; the helper
// stream; the idle LDS; leaves ahead by size and by free memory; the one scratch bound against the three sums the driver used to carry.
// tests/test_trie_plan_native.py builds it with AddressSanitizer + UBSan.  No GPU, no kernel and no Python-loaded library is involved.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../phant_amd/csrc/trie_plan.h"

using namespace phant;

static int g_checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_where); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)
static char g_where[128] = "";

struct Knobs {
    int no_coop, no_wave;
    long long coop_max;
    int slot_blocks;
    long long fallback_grid;
};
struct BinCase {
    unsigned count;
    unsigned long long children;
    unsigned cls, grid, block, fb_grid, fb_block;  // cls: 0 a wave per node, 1 a node per half wave, 2 / 3 / 4: slots of 1 / 2 / 4 blocks
};
struct Setting {
    const char* name;
    Knobs k;
    std::vector<BinCase> cases;
};

static const Setting SETTINGS[] = {
    {"default", {0, 0, -1, 0, -1}, {
        {1, 2, 0, 1, 64, 0, 0}, {512, 1024, 0, 512, 64, 0, 0}, {513, 1026, 0, 129, 256, 0, 0}, {1024, 2048, 0, 256, 256, 0, 0},
        {1025, 2050, 0, 257, 256, 0, 0}, {2048, 4096, 0, 512, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"no_coop", {1, 0, -1, 0, -1}, {
        {1, 2, 4, 1, 64, 0, 0}, {512, 1024, 4, 8, 64, 0, 0}, {513, 1026, 4, 9, 64, 0, 0}, {1024, 2048, 4, 16, 64, 0, 0},
        {1025, 2050, 4, 17, 64, 0, 0}, {2048, 4096, 4, 32, 64, 0, 0}, {2049, 4098, 4, 33, 64, 0, 0}, {4096, 8192, 4, 64, 64, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"no_wave", {0, 1, -1, 0, -1}, {
        {1, 2, 1, 1, 64, 0, 0}, {512, 1024, 1, 256, 64, 0, 0}, {513, 1026, 1, 257, 64, 0, 0}, {1024, 2048, 1, 512, 64, 0, 0},
        {1025, 2050, 1, 129, 256, 0, 0}, {2048, 4096, 1, 256, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"coop_max0", {0, 0, 0, 0, -1}, {
        {1, 2, 4, 1, 64, 0, 0}, {512, 1024, 4, 8, 64, 0, 0}, {513, 1026, 4, 9, 64, 0, 0}, {1024, 2048, 4, 16, 64, 0, 0},
        {1025, 2050, 4, 17, 64, 0, 0}, {2048, 4096, 4, 32, 64, 0, 0}, {2049, 4098, 4, 33, 64, 0, 0}, {4096, 8192, 4, 64, 64, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    // (1 << 21 is clamped to 1 << 20: three million nodes are beyond it)
    {"coop_max_2_21", {0, 0, 2097152, 0, -1}, {
        {1, 2, 0, 1, 64, 0, 0}, {512, 1024, 0, 512, 64, 0, 0}, {513, 1026, 0, 129, 256, 0, 0}, {1024, 2048, 0, 256, 256, 0, 0},
        {1025, 2050, 0, 257, 256, 0, 0}, {2048, 4096, 0, 512, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 1, 513, 256, 0, 0}, {65535, 131070, 1, 8192, 256, 0, 0}, {65536, 196608, 1, 8192, 256, 0, 0}, {65536, 196609, 1, 8192, 256, 0, 0},
        {65536, 393216, 1, 8192, 256, 0, 0}, {65536, 393217, 1, 8192, 256, 0, 0}, {65537, 196611, 1, 8193, 256, 0, 0}, {65537, 196612, 1, 8193, 256, 0, 0},
        {65537, 393222, 1, 8193, 256, 0, 0}, {65537, 393223, 1, 8193, 256, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"blocks1", {0, 0, -1, 1, -1}, {
        {1, 2, 2, 1, 256, 1, 64}, {512, 1024, 2, 2, 256, 8, 64}, {513, 1026, 2, 3, 256, 9, 64}, {1024, 2048, 2, 4, 256, 16, 64},
        {1025, 2050, 2, 5, 256, 17, 64}, {2048, 4096, 2, 8, 256, 32, 64}, {2049, 4098, 2, 9, 256, 33, 64}, {4096, 8192, 2, 16, 256, 64, 64},
        {4097, 8194, 2, 17, 256, 65, 64}, {65535, 131070, 2, 256, 256, 1024, 64}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 2, 256, 256, 1024, 64},
        {65536, 393216, 2, 256, 256, 1024, 64}, {65536, 393217, 2, 256, 256, 1024, 64}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 2, 257, 256, 1024, 64},
        {65537, 393222, 2, 257, 256, 1024, 64}, {65537, 393223, 2, 257, 256, 1024, 64}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"blocks2", {0, 0, -1, 2, -1}, {
        {1, 2, 3, 1, 128, 1, 64}, {512, 1024, 3, 4, 128, 8, 64}, {513, 1026, 3, 5, 128, 9, 64}, {1024, 2048, 3, 8, 128, 16, 64},
        {1025, 2050, 3, 9, 128, 17, 64}, {2048, 4096, 3, 16, 128, 32, 64}, {2049, 4098, 3, 17, 128, 33, 64}, {4096, 8192, 3, 32, 128, 64, 64},
        {4097, 8194, 3, 33, 128, 65, 64}, {65535, 131070, 3, 512, 128, 1024, 64}, {65536, 196608, 3, 512, 128, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 3, 512, 128, 1024, 64}, {65537, 196611, 3, 513, 128, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 3, 513, 128, 1024, 64}, {3000000, 9000000, 3, 23438, 128, 1024, 64},
    }},
    {"blocks4", {0, 0, -1, 4, -1}, {
        {1, 2, 4, 1, 64, 0, 0}, {512, 1024, 4, 8, 64, 0, 0}, {513, 1026, 4, 9, 64, 0, 0}, {1024, 2048, 4, 16, 64, 0, 0},
        {1025, 2050, 4, 17, 64, 0, 0}, {2048, 4096, 4, 32, 64, 0, 0}, {2049, 4098, 4, 33, 64, 0, 0}, {4096, 8192, 4, 64, 64, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 4, 1024, 64, 0, 0}, {65536, 196609, 4, 1024, 64, 0, 0},
        {65536, 393216, 4, 1024, 64, 0, 0}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 4, 1025, 64, 0, 0}, {65537, 196612, 4, 1025, 64, 0, 0},
        {65537, 393222, 4, 1025, 64, 0, 0}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 4, 46875, 64, 0, 0},
    }},
    // (3 is no slot size: it only keeps the thin-bin kernels away)
    {"blocks3", {0, 0, -1, 3, -1}, {
        {1, 2, 4, 1, 64, 0, 0}, {512, 1024, 4, 8, 64, 0, 0}, {513, 1026, 4, 9, 64, 0, 0}, {1024, 2048, 4, 16, 64, 0, 0},
        {1025, 2050, 4, 17, 64, 0, 0}, {2048, 4096, 4, 32, 64, 0, 0}, {2049, 4098, 4, 33, 64, 0, 0}, {4096, 8192, 4, 64, 64, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    // (0 is no grid: the default of 1 024 workgroups)
    {"grid0", {0, 0, -1, 0, 0}, {
        {1, 2, 0, 1, 64, 0, 0}, {512, 1024, 0, 512, 64, 0, 0}, {513, 1026, 0, 129, 256, 0, 0}, {1024, 2048, 0, 256, 256, 0, 0},
        {1025, 2050, 0, 257, 256, 0, 0}, {2048, 4096, 0, 512, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1024, 64}, {65537, 196612, 3, 513, 128, 1024, 64},
        {65537, 393222, 3, 513, 128, 1024, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1024, 64},
    }},
    {"grid1", {0, 0, -1, 0, 1}, {
        {1, 2, 0, 1, 64, 0, 0}, {512, 1024, 0, 512, 64, 0, 0}, {513, 1026, 0, 129, 256, 0, 0}, {1024, 2048, 0, 256, 256, 0, 0},
        {1025, 2050, 0, 257, 256, 0, 0}, {2048, 4096, 0, 512, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1, 64}, {65536, 196609, 3, 512, 128, 1, 64},
        {65536, 393216, 3, 512, 128, 1, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1, 64}, {65537, 196612, 3, 513, 128, 1, 64},
        {65537, 393222, 3, 513, 128, 1, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 1, 64},
    }},
    // (1 << 21 is clamped to 1 << 20: a bin's own wave count is below it everywhere here)
    {"grid_2_21", {0, 0, -1, 0, 2097152}, {
        {1, 2, 0, 1, 64, 0, 0}, {512, 1024, 0, 512, 64, 0, 0}, {513, 1026, 0, 129, 256, 0, 0}, {1024, 2048, 0, 256, 256, 0, 0},
        {1025, 2050, 0, 257, 256, 0, 0}, {2048, 4096, 0, 512, 256, 0, 0}, {2049, 4098, 1, 257, 256, 0, 0}, {4096, 8192, 1, 512, 256, 0, 0},
        {4097, 8194, 4, 65, 64, 0, 0}, {65535, 131070, 4, 1024, 64, 0, 0}, {65536, 196608, 2, 256, 256, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 4, 1024, 64, 0, 0}, {65537, 196611, 2, 257, 256, 1025, 64}, {65537, 196612, 3, 513, 128, 1025, 64},
        {65537, 393222, 3, 513, 128, 1025, 64}, {65537, 393223, 4, 1025, 64, 0, 0}, {3000000, 9000000, 2, 11719, 256, 46875, 64},
    }},
    {"blocks1_grid1", {0, 0, -1, 1, 1}, {
        {1, 2, 2, 1, 256, 1, 64}, {512, 1024, 2, 2, 256, 1, 64}, {513, 1026, 2, 3, 256, 1, 64}, {1024, 2048, 2, 4, 256, 1, 64},
        {1025, 2050, 2, 5, 256, 1, 64}, {2048, 4096, 2, 8, 256, 1, 64}, {2049, 4098, 2, 9, 256, 1, 64}, {4096, 8192, 2, 16, 256, 1, 64},
        {4097, 8194, 2, 17, 256, 1, 64}, {65535, 131070, 2, 256, 256, 1, 64}, {65536, 196608, 2, 256, 256, 1, 64}, {65536, 196609, 2, 256, 256, 1, 64},
        {65536, 393216, 2, 256, 256, 1, 64}, {65536, 393217, 2, 256, 256, 1, 64}, {65537, 196611, 2, 257, 256, 1, 64}, {65537, 196612, 2, 257, 256, 1, 64},
        {65537, 393222, 2, 257, 256, 1, 64}, {65537, 393223, 2, 257, 256, 1, 64}, {3000000, 9000000, 2, 11719, 256, 1, 64},
    }},
    {"blocks2_grid_2_21", {0, 0, -1, 2, 2097152}, {
        {1, 2, 3, 1, 128, 1, 64}, {512, 1024, 3, 4, 128, 8, 64}, {513, 1026, 3, 5, 128, 9, 64}, {1024, 2048, 3, 8, 128, 16, 64},
        {1025, 2050, 3, 9, 128, 17, 64}, {2048, 4096, 3, 16, 128, 32, 64}, {2049, 4098, 3, 17, 128, 33, 64}, {4096, 8192, 3, 32, 128, 64, 64},
        {4097, 8194, 3, 33, 128, 65, 64}, {65535, 131070, 3, 512, 128, 1024, 64}, {65536, 196608, 3, 512, 128, 1024, 64}, {65536, 196609, 3, 512, 128, 1024, 64},
        {65536, 393216, 3, 512, 128, 1024, 64}, {65536, 393217, 3, 512, 128, 1024, 64}, {65537, 196611, 3, 513, 128, 1025, 64}, {65537, 196612, 3, 513, 128, 1025, 64},
        {65537, 393222, 3, 513, 128, 1025, 64}, {65537, 393223, 3, 513, 128, 1025, 64}, {3000000, 9000000, 3, 23438, 128, 46875, 64},
    }},
};

static void bins() {
    for (const Setting& s : SETTINGS) {
        TrieTune tune;
        tune.no_coop = s.k.no_coop;
        tune.no_wave = s.k.no_wave;
        tune.coop_max = s.k.coop_max;
        tune.slot_blocks = s.k.slot_blocks;
        tune.fallback_grid = s.k.fallback_grid;
        const TrieChoices ch = resolve_choices(tune);
        CHECK(s.cases.size() == 19);
        for (const BinCase& b : s.cases) {
            std::snprintf(g_where, sizeof g_where, "%s, %u nodes, %llu children", s.name, b.count, b.children);
            const BinLaunch p = plan_bin(b.count, b.children, ch);
            CHECK(p.cls == b.cls && p.grid == b.grid && p.block == b.block && p.fb_grid == b.fb_grid && p.fb_block == b.fb_block);
            CHECK(p.slot_blocks == (b.cls == 2 ? 1u : b.cls == 3 ? 2u : b.cls == 4 ? 4u : 0u));
        }
    }
}

static TrieChoices with_small_max(long long v) {
    TrieTune tune;
    tune.small_max_keys = v;
    return resolve_choices(tune);
}

static void passes() {
    struct {
        unsigned n;
        unsigned long long val_bytes;
        bool by_default, at0, at100, at5000;  // small_max_keys -1, 0, 100, 5 000
    } const cases[] = {
        {0, 0, true, true, true, true},
        {1, 1, true, false, true, true},
        {2048, 2048, true, false, false, true},
        {2049, 278663, false, false, false, true},  // 136 x 2 049 - 1
        {2049, 278664, true, false, false, true},
        {4096, 557055, false, false, false, true},  // 136 x 4 096 - 1
        {4096, 557056, true, false, false, true},
        {4097, 557191, false, false, false, false},
        {4097, 557192, false, false, false, false},  // (beyond what the first kernel's LDS holds, whatever the values)
    };
    for (const auto& c : cases) {
        std::snprintf(g_where, sizeof g_where, "pass of %u keys, %llu value bytes", c.n, c.val_bytes);
        const TreeLevels lv = tree_levels(c.n);
        CHECK(small_pass(c.n, c.val_bytes, lv, with_small_max(-1)) == c.by_default);
        CHECK(small_pass(c.n, c.val_bytes, lv, with_small_max(0)) == c.at0);
        CHECK(small_pass(c.n, c.val_bytes, lv, with_small_max(100)) == c.at100);
        CHECK(small_pass(c.n, c.val_bytes, lv, with_small_max(5000)) == c.at5000);
    }
    std::snprintf(g_where, sizeof g_where, "small_climb_grid");
    CHECK(small_climb_grid(1) == 1 && small_climb_grid(4) == 1 && small_climb_grid(5) == 2 && small_climb_grid(2048) == 512 && small_climb_grid(4096) == 512);
}

static void levels() {
    struct {
        unsigned n, n_lvl;
        unsigned size[5], off[5];
        size_t tree_ints;
    } const cases[] = {
        {1, 1, {16}, {0}, 0},
        {15, 1, {16}, {0}, 0},
        {16, 2, {32, 16}, {0, 0}, 16},
        {255, 2, {256, 16}, {0, 0}, 16},
        {256, 3, {272, 32, 16}, {0, 0, 32}, 48},
        {4096, 4, {4112, 272, 32, 16}, {0, 0, 272, 304}, 320},
        {1000000, 5, {1000016, 62512, 3920, 256, 16}, {0, 0, 62512, 66432, 66688}, 66704},
    };
    for (const auto& c : cases) {
        std::snprintf(g_where, sizeof g_where, "levels of %u keys", c.n);
        const TreeLevels lv = tree_levels(c.n);
        CHECK(lv.n_lvl == c.n_lvl && lv.tree_ints == c.tree_ints);
        for (unsigned k = 0; k < c.n_lvl; ++k) CHECK(lv.size[k] == c.size[k] && lv.off[k] == c.off[k]);
    }
    std::snprintf(g_where, sizeof g_where, "levels of 2^31 - 2 keys");
    CHECK(tree_levels(0x7ffffffeu).n_lvl == 8 && tree_levels(0x7ffffffeu).size[0] == 0x80000000u && tree_levels(0x7ffffffeu).size[7] == 16);
}

static void side_and_lds() {
    std::snprintf(g_where, sizeof g_where, "side_ok");
    TrieTune tune;
    CHECK(!side_ok(399999, resolve_choices(tune)) && side_ok(400000, resolve_choices(tune)) && side_ok(400001, resolve_choices(tune)));
    tune.no_side = true;
    CHECK(!side_ok(400001, resolve_choices(tune)));
    tune.side_min_keys = 0;
    CHECK(!side_ok(400001, resolve_choices(tune)));
    tune.no_side = false;
    CHECK(side_ok(1, resolve_choices(tune)) && side_ok(399999, resolve_choices(tune)));
    CHECK(bin_on_side(5, 5) && bin_on_side(511, 5) && !bin_on_side(4, 5) && !bin_on_side(0, -1) && !bin_on_side(511, -1));
    std::snprintf(g_where, sizeof g_where, "side_lds");
    const long long knob[] = {-1, 0, 29696, 29697}, lds[] = {20480, 0, 29696, 29696};
    for (int i = 0; i < 4; ++i) {
        TrieTune t2;
        t2.side_lds = knob[i];
        CHECK(resolve_choices(t2).side_lds == lds[i]);
    }
    std::snprintf(g_where, sizeof g_where, "the other knobs");
    TrieTune t3;
    CHECK(!resolve_choices(t3).join_in_stream && resolve_choices(t3).force_blocks == 0 && resolve_choices(t3).small_max == -1);
    t3.join_in_stream = true;
    CHECK(resolve_choices(t3).join_in_stream);
}

static void ahead() {
    std::snprintf(g_where, sizeof g_where, "leaves ahead by size");
    const unsigned long long ROOMY = 1ull << 50;  // (a t2 arena that holds anything: the size alone decides)
    TrieTune tune;
    TrieChoices ch = resolve_choices(tune);
    CHECK(leaves_ahead(1, 100, ROOMY, false, 0, ch) && leaves_ahead(8388608, 100, ROOMY, false, 0, ch) && !leaves_ahead(8388609, 100, ROOMY, false, 0, ch));
    tune.ahead_max_keys = 0;
    ch = resolve_choices(tune);
    CHECK(!leaves_ahead(1, 100, ROOMY, false, 0, ch) && !leaves_ahead(8388608, 100, ROOMY, false, 0, ch));
    CHECK(!ask_free_bytes(1, 1000000, 1000, ch));  // (never ahead: nothing to ask)
    std::snprintf(g_where, sizeof g_where, "leaves ahead by memory");
    ch = resolve_choices(TrieTune{});
    // tables of 1 000 000 bytes, an arena of 1 000: the runtime is asked, and 999 000 free bytes are exactly enough
    CHECK(ask_free_bytes(3000, 1000000, 1000, ch) && !ask_free_bytes(3000, 1000000, 1000000, ch) && !ask_free_bytes(8388609, 1000000, 1000, ch));
    CHECK(!leaves_ahead(3000, 1000000, 1000, true, 998999, ch));
    CHECK(leaves_ahead(3000, 1000000, 1000, true, 999000, ch));
    CHECK(leaves_ahead(3000, 1000000, 1000, false, 0, ch));       // (the runtime gave no answer: tried)
    CHECK(leaves_ahead(3000, 1000000, 1000000, false, 0, ch));    // (the arena as it stands holds them)
}

static void bounds() {
    struct {
        unsigned long long n, key_bytes, val_bytes, scratch, worst;
    } const cases[] = {{1, 32, 1, 4899, 1315}, {3000, 96000, 240000, 2650096, 4182000}, {1000000, 32000000, 78000000, 880004096, 1392000000}};
    for (const auto& c : cases) {
        std::snprintf(g_where, sizeof g_where, "bounds of %llu keys", c.n);
        const unsigned long long n = c.n, total_key_bytes = c.key_bytes, total_val_bytes = c.val_bytes, reps = c.n, max_key = 255;
        // the three sums as the driver carried them: the general pass's tables, the small pass's, the leaves-ahead decision's
        const unsigned long long general = total_val_bytes + total_key_bytes + n * 32 + reps * (3 + 16 * 33 + 16 + 48 + max_key / 2 + 16) + 4096;
        const unsigned long long small = total_val_bytes + total_key_bytes + n * (32 + 3 + 16 * 33 + 16 + 48 + 127 + 16) + 4096;
        const unsigned long long worst = n * (16 * 32 + 3 + 16 * 33 + 16 + 48 + 127 + 16 + 32) + total_val_bytes + total_key_bytes;
        CHECK(general == c.scratch && small == c.scratch && worst == c.worst);
        CHECK(scratch_bound(n, n, c.key_bytes, c.val_bytes) == c.scratch);
        CHECK(slot_table_bytes(n) == 512 * n);
        CHECK(ahead_need(n, c.key_bytes, c.val_bytes) == c.worst);
        CHECK(slot_table_bytes(n) + scratch_bound(n, n, c.key_bytes, c.val_bytes) == c.worst + 4096);
    }
    std::snprintf(g_where, sizeof g_where, "tables from the node count");
    CHECK(scratch_bound(1025, 3000, 96000, 240000) == 1192546 && slot_table_bytes(1025) == 524800);
}

int main() {
    bins();
    passes();
    levels();
    side_and_lds();
    ahead();
    bounds();
    std::printf("%d checks\n", g_checks);
    return 0;
}
