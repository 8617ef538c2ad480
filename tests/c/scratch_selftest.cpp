// Stand-alone check of zlib_rs_amd/csrc/zmi_scratch.h (tests/test_scratch_layout.py builds it with the address and undefined-behaviour
// sanitizers and runs it): the carver's two passes agree and its arrays are aligned, disjoint and inside the reservation; the
// launch-group planner equals the formula written out here.  ZMI_EMU arms the carver's own bound assertion.
#define ZMI_EMU 1
#include "zmi_scratch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

// One layout with every width, counts 0 / 1 / odd / even, a u64 directly behind an odd number of u32, the four-word block behind an
// odd number of u32, an "owned unless supplied" table, and a byte region with margins behind a 256-byte rounding.
struct tables {
    uint64_t *a64, *none64, *b64, *own;
    uint32_t *a32, *b32, *c32;
    int32_t* s32;
    uint16_t *a16, *b16;
    uint8_t *a8, *b8, *reg;
    zmi_words4 w4;
    size_t layout(zmi_carver k, uint64_t* supplied) {
        k.take(3, a64);
        k.take(0, none64);
        k.take(5, a32);             // odd
        k.take(1, b64);             // u64 directly behind an odd number of u32
        k.take(7, a8);
        k.take(3, a16);
        k.take(1, b8);
        k.take(2, b16);
        k.take(3, b32, s32);        // two tables of one count
        k.take(w4);                 // behind 3 + 3 u32: the block must still be 8-byte aligned
        k.take(4, c32);
        k.take_unless(supplied, 6, own);
        k.align(256u);
        k.region(reg, 37, 16u);
        return k.end();
    }
};
struct span { const uint8_t* p; size_t n; size_t al; const char* name; };

static void check_carver(bool supply) {
    uint64_t callers[6];
    uint64_t* const supplied = supply ? callers : nullptr;
    tables t;
    const size_t total = t.layout(zmi_carver(), supplied);
    CHECK(t.a64 == nullptr && t.reg == nullptr && t.w4.w == nullptr);   // the sizing pass yields no pointers
    uint8_t* base = (uint8_t*)malloc(total);                           // exactly `total`: the sanitizer sees one byte too many
    const size_t end = t.layout(zmi_carver(base, total), supplied);
    CHECK(end == total);
    const std::vector<span> v = {
        {(uint8_t*)t.a64, 3 * 8, 8, "a64"}, {(uint8_t*)t.none64, 0, 8, "none64"}, {(uint8_t*)t.a32, 5 * 4, 4, "a32"},
        {(uint8_t*)t.b64, 8, 8, "b64"}, {t.a8, 7, 1, "a8"}, {(uint8_t*)t.a16, 3 * 2, 2, "a16"}, {t.b8, 1, 1, "b8"},
        {(uint8_t*)t.b16, 2 * 2, 2, "b16"}, {(uint8_t*)t.b32, 3 * 4, 4, "b32"}, {(uint8_t*)t.s32, 3 * 4, 4, "s32"},
        {(uint8_t*)t.w4.w, 16, 8, "w4"}, {(uint8_t*)t.c32, 4 * 4, 4, "c32"}, {t.reg - 16, 37 + 32, 1, "reg and its margins"},
        {(uint8_t*)t.own, supply ? 0u : 6u * 8u, 8, "own"}};
    for (size_t i = 0; i < v.size(); ++i) {
        if (supply && i + 1 == v.size()) break;   // (the caller's table lies outside the buffer)
        CHECK(((uintptr_t)v[i].p % v[i].al) == 0);
        CHECK(v[i].p >= base && v[i].p + v[i].n <= base + total);
        for (size_t j = 0; j < i; ++j) CHECK(v[i].p + v[i].n <= v[j].p || v[j].p + v[j].n <= v[i].p);
        memset((void*)v[i].p, 0xA5, v[i].n);      // to the last element, on a block of exactly `total` bytes
    }
    CHECK(((uintptr_t)t.reg - (uintptr_t)base - 16u) % 256u == 0);
    // typed stores to every last element
    t.a64[2] = 1; t.a32[4] = 1; t.b64[0] = 1; t.a16[2] = 1; t.b16[1] = 1; t.b32[2] = 1; t.s32[2] = -1; t.c32[3] = 1; t.reg[36] = 1;
    // the four-word block: word(i) are its words, upper64() its upper half
    CHECK(t.w4.word(0) == t.w4.w && t.w4.word(3) == t.w4.w + 3);
    CHECK((uint8_t*)t.w4.upper64() == (uint8_t*)t.w4.w + 8 && ((uintptr_t)t.w4.upper64() % 8) == 0);
    *t.w4.upper64() = 0x1122334455667788ull;
    CHECK(*t.w4.word(2) == 0x55667788u && *t.w4.word(3) == 0x11223344u);
    if (supply) CHECK(t.own == callers);
    free(base);
}
// an "owned unless supplied" table takes its room when owned and none when the caller supplies it
static void check_take_unless() {
    uint64_t callers[6], *head, *own;
    zmi_carver k;
    k.take(2, head);
    k.take_unless((uint64_t*)nullptr, 6, own);
    CHECK(k.end() == 2 * 8 + 6 * 8 && own == nullptr);
    k.take_unless(callers, 6, own);
    CHECK(k.end() == 2 * 8 + 6 * 8 && own == callers);
}

// the formula, written out independently of the header
static uint64_t want_group(uint64_t limit, uint64_t ov, uint64_t np, uint64_t max_len, uint64_t stride) {
    uint64_t padded = (max_len + 63) / 64 * 64;
    if (padded == 0) padded = 64;
    const uint64_t match_per = padded * 4;
    uint64_t group = limit / (stride + match_per + match_per / 16);
    if (ov) group = ov;
    return group < np ? group : np;
}
static void check_planner() {
    const uint64_t lens[] = {0, 1, 63, 64, 65, 65280, 65536, 1ull << 20, 1ull << 30};
    const uint64_t limits[] = {64ull << 20, 8ull << 30};
    const uint64_t nps[] = {1, 2, 33, (1ull << 31) - 1};
    for (uint64_t max_len : lens)
        for (uint64_t limit : limits)
            for (uint64_t np : nps) {
                const uint64_t ovs[] = {0, 1, np + 5};
                for (uint64_t ov : ovs) {
                    const uint64_t stride = max_len + (max_len >> 3) + 160;   // (any slot size of the right order)
                    const zmi_group_plan p = zmi_plan_groups(limit, ov, np, max_len, stride);
                    const uint64_t want = want_group(limit, ov, np, max_len, stride);
                    CHECK(p.group == want);
                    if (want == 0) {
                        CHECK(p.wpg == 0 && p.n_groups == 0 && p.bm_words == 0);
                        continue;
                    }
                    CHECK(p.wpg == (want + 31) / 32);
                    CHECK(p.n_groups == (np + want - 1) / want);
                    CHECK(p.bm_words == p.n_groups * p.wpg);
                }
            }
    // one piece that does not fit: 2^30 bytes under 64 MiB, and nothing else in the result
    const zmi_group_plan none = zmi_plan_groups(64ull << 20, 0, 4, 1ull << 30, (1ull << 30) + 160);
    CHECK(none.group == 0 && none.wpg == 0 && none.n_groups == 0 && none.bm_words == 0);
    // ... unless the override says otherwise
    CHECK(zmi_plan_groups(64ull << 20, 3, 4, 1ull << 30, (1ull << 30) + 160).group == 3);
    // the bitmap geometry at the 32 / 33 boundary
    const zmi_group_plan g32 = zmi_plan_groups(8ull << 30, 32, 100, 1024, 2048), g33 = zmi_plan_groups(8ull << 30, 33, 100, 1024, 2048);
    CHECK(g32.group == 32 && g32.wpg == 1 && g32.n_groups == 4 && g32.bm_words == 4);
    CHECK(g33.group == 33 && g33.wpg == 2 && g33.n_groups == 4 && g33.bm_words == 8);
    // no pieces: no group, and no per-piece cost: one group
    CHECK(zmi_plan_groups(8ull << 30, 0, 0, 1024, 2048).group == 0);
    CHECK(zmi_plan_groups_per(8ull << 30, 0, 7, 0).group == 7 && zmi_plan_groups_per(8ull << 30, 2, 7, 0).n_groups == 4);
    CHECK(zmi_match_per(0) == 256 && zmi_match_per(1) == 256 && zmi_match_per(64) == 256 && zmi_match_per(65) == 512);
}

int main() {
    check_carver(false);
    check_carver(true);
    check_take_unless();
    check_planner();
    if (g_fail) return 1;
    printf("scratch_selftest: ok\n");
    return 0;
}
