// The split plan of bm25_topk_kernel (kektordb_amd/csrc/kdb_text_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/text_plan_test.cpp
// When a call splits and into how many parts, the bytes of the partial lists, and the boundary routine on hand-made lists.
#include "kdb_text_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static constexpr uint64_t BIG = KDB_TEXT_SPLIT_MIN_POSTINGS, END = 1ull << 32;
static constexpr uint32_t M = 1000000u; // 1M ids: 245 tiles
static_assert(kdb_text_tiles(M) == 245 && kdb_text_tiles(4095) == 1 && kdb_text_tiles(4096) == 2 && kdb_text_tiles(0) == 1, "ids 0..n_ids");
static constexpr uint32_t capped(uint32_t want, uint32_t tiles) { // the rules restated: the tile cap, the parts cap, below two = one
    uint32_t p = want < tiles / KDB_TEXT_MIN_TILES_PER_PART ? want : tiles / KDB_TEXT_MIN_TILES_PER_PART;
    p = p > KDB_TEXT_MAX_PARTS ? KDB_TEXT_MAX_PARTS : p;
    return p < 2 ? 1 : p;
}
static_assert(kdb_text_split_plan(KdbTextSplitIn{1, 10, M, 256, BIG, -1}).parts == capped(512, 245), "usable in constant expressions");

static const struct {
    KdbTextSplitIn in; // B, k, n_ids, n_cus, postings_bound, forced
    uint32_t parts;
} CASES[] = {
    {{512, 10, M, 256, BIG << 8, -1}, 1}, // B >= 2 * n_cus: one workgroup per query, whatever the lists
    {{4096, 10, M, 256, BIG << 8, -1}, 1},
    {{511, 10, M, 256, BIG, -1}, capped(2, 245)}, // fewer queries: ceil(2 * n_cus / B), capped by the tiles ...
    {{100, 10, M, 256, BIG, -1}, capped(6, 245)},
    {{64, 3, M, 256, BIG, -1}, capped(8, 245)},
    {{1, 10, M, 256, BIG, -1}, capped(512, 245)},
    {{1, 10, 40000, 256, BIG, -1}, capped(512, 10)},
    {{1, 10, 4095, 256, BIG, -1}, 1},
    {{1, 10, KDB_TEXT_MAX_ID, 1024, BIG, -1}, capped(2048, 262144)}, // ... and by KDB_TEXT_MAX_PARTS
    {{1, 10, KDB_TEXT_MAX_ID, 1024, BIG, 100000}, KDB_TEXT_MAX_PARTS},
    {{1, 10, M, 256, BIG - 1, -1}, 1}, // the postings threshold, from below
    {{1, 10, M, 256, BIG << 8, 0}, 1}, // forced: 0 never; N exactly N whatever the bound and B, clamped to a tile per part
    {{7, 1, M, 256, 0, 3}, 3},
    {{4096, 1024, M, 256, 1, 7}, 7},
    {{1, 10, M, 256, 0, 1}, 1},
    {{10, 10, 40000, 256, 0, 10}, 10},
    {{10, 10, 40000, 256, 0, 64}, 10},
    {{10, 10, 4095, 256, 0, 64}, 1},
    {{65536, 10, M, 256, 0, 4}, 1}, // the queries are the grid's second dimension
};

static void plans() {
    for (const auto &c : CASES) {
        const KdbTextSplitPlan p = kdb_text_split_plan(c.in);
        CHECK(p.parts == c.parts && p.parts <= KDB_TEXT_MAX_PARTS && p.parts <= kdb_text_tiles(c.in.n_ids));
        const uint64_t R = (uint64_t)c.in.B * p.parts, k = c.in.k;
        CHECK(p.scratch_bytes % 8 == 0 && p.scratch_bytes == (p.parts == 1 ? 0 : (R * (12 * k + 8) + 7) / 8 * 8));
        const KdbTextParts P = kdb_text_parts(c.in.B, p.parts, c.in.k); // the arrays in order, 8-byte aligned, inside the total
        CHECK(P.o_keys == 0 && P.o_counts == R * k * 8 && P.o_ids == P.o_counts + R * 8 && P.o_ids + R * k * 4 <= P.total);
        CHECK(p.merge_lds == kdb_text_sort_n(c.in.k) * 12u + 8u + 64u && p.merge_lds <= KDB_TEXT_LDS_LIMIT);
    }
}

// the bounds of every part of a query with the lists [lo[t], hi[t]) of post_doc, checked against the rules of the header
static std::vector<uint64_t> bounds_of(const std::vector<uint32_t> &post_doc, const std::vector<uint64_t> &lo, const std::vector<uint64_t> &hi, uint32_t parts) {
    const KdbTextSpan sp = kdb_text_longest(lo.data(), hi.data(), (uint32_t)lo.size());
    std::vector<uint64_t> b;
    for (uint32_t s = 0; s <= parts; s++) b.push_back(kdb_text_split_bound(post_doc.data(), sp, parts, s));
    CHECK(b.front() == 0 && b.back() > KDB_TEXT_MAX_ID && b.back() == END);
    for (uint32_t s = 0; s < parts; s++) CHECK(b[s] <= b[s + 1] && b[s] % KDB_TEXT_TILE == 0);
    for (size_t t = 0; t < lo.size(); t++) { // the parts' cursor ranges tile every list, each posting inside its part's bounds
        uint64_t at = lo[t];
        for (uint32_t s = 0; s < parts; s++) {
            const uint64_t c = kdb_text_lower_bound(post_doc.data(), lo[t], hi[t], b[s]), e = kdb_text_lower_bound(post_doc.data(), c, hi[t], b[s + 1]);
            CHECK(c == at && e >= c);
            for (uint64_t i = c; i < e; i++) CHECK(post_doc[i] >= b[s] && post_doc[i] < b[s + 1]);
            at = e;
        }
        CHECK(at == hi[t]);
    }
    return b;
}

static void boundaries() {
    std::vector<uint32_t> pd;
    std::vector<uint64_t> lo, hi;
    auto list = [&](uint32_t first, uint32_t last, uint32_t step) {
        lo.push_back(pd.size());
        for (uint32_t d = first; d <= last; d += step) pd.push_back(d);
        hi.push_back(pd.size());
    };
    list(5000, 5600, 1);   // inside tile 1
    list(1, 12297, 4);     // 3075 postings over tiles 0..3: the longest
    list(30000, 30050, 1); // behind the longest list's last tile: the last part takes it
    list(40000, 40000, 1);
    list(9, 12305, 4);     // as long as the longest, later in the query: the earlier one is taken
    const KdbTextSpan sp = kdb_text_longest(lo.data(), hi.data(), 5);
    CHECK(sp.a == lo[1] && sp.len == 3075);
    for (uint32_t parts : {2u, 10u, 512u}) CHECK(bounds_of(pd, lo, hi, parts)[parts - 1] <= 12288);
    CHECK((bounds_of(pd, lo, hi, 3) == std::vector<uint64_t>{0, 4096, 8192, END})); // postings 1025 and 2050: ids 4101 and 8201
    // the longest list inside one tile: equal inner bounds, the middle parts empty
    CHECK((bounds_of(pd, {lo[0], lo[3]}, {hi[0], hi[3]}, 4) == std::vector<uint64_t>{0, 4096, 4096, 4096, END}));
    // no list at all: nothing is read (a null array), every part is empty
    const uint64_t z[2] = {0, 0};
    CHECK(kdb_text_longest(z, z, 2).len == 0 && kdb_text_longest(z, z, 0).len == 0);
    for (uint32_t s = 0; s <= 5; s++) CHECK(kdb_text_split_bound(nullptr, KdbTextSpan{0, 0}, 5, s) == (s == 5 ? END : 0));
    CHECK((bounds_of({KDB_TEXT_MAX_ID - 1, KDB_TEXT_MAX_ID}, {0}, {2}, 2) == std::vector<uint64_t>{0, KDB_TEXT_MAX_ID & ~(KDB_TEXT_TILE - 1), END}));
}

int main() {
    plans();
    boundaries();
    printf("ok\n");
    return 0;
}
