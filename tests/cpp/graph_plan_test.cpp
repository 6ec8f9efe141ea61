// The plan of the graph-filter kernels (kektordb_amd/csrc/kdb_graph_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/graph_plan_test.cpp
#include "kdb_graph_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) ((cond) ? (void)0 : exit((printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond), 1)))

static_assert(kdb_graph_clamp_depth(-7) == 1 && kdb_graph_clamp_depth(0) == 1 && kdb_graph_clamp_depth(1) == 1 && kdb_graph_clamp_depth(5) == 5 &&
                  kdb_graph_clamp_depth(6) == 5 && kdb_graph_clamp_depth(INT32_MAX) == 5 && kdb_graph_clamp_depth(INT32_MIN) == 1, "graph.go:185-190");
static_assert(kdb_graph_wpn(63) == 1 && kdb_graph_wpn(64) == 2 && kdb_graph_wpn(KDB_GRAPH_MAX_NODES) == (1u << 25) + 1u &&
                  kdb_graph_min_words(100, 8) == 2 && kdb_graph_min_words(8, 300) == 5, "nodes 0..n_nodes; a list is also the visited set");
static_assert(kdb_graph_live_mask(0, 5) == 0x3e && kdb_graph_live_mask(0, 63) == ~1ull && kdb_graph_live_mask(1, 63) == 0 && kdb_graph_live_mask(1, 64) == 1 &&
                  kdb_graph_live_mask(0, 64) == ~1ull && kdb_graph_live_mask(1, 127) == ~0ull, "bit 0 and the bits above count");

static kdb_graph_query query(uint32_t root, int32_t depth, uint32_t dir, uint64_t mask) { return kdb_graph_query{root, depth, dir, 0, mask}; }

int main() {
    // staging: "follows nothing", the clamp, direction bits, the level count
    CHECK(kdb_graph_follows_nothing(query(0, 3, KDB_GDIR_BOTH, 1)) && kdb_graph_follows_nothing(query(4, 3, KDB_GDIR_NONE, 1)) &&
          kdb_graph_follows_nothing(query(4, 3, KDB_GDIR_OUT, 0)) && !kdb_graph_follows_nothing(query(4, -1, KDB_GDIR_IN, 1ull << 63)));
    const uint32_t dirs[4] = {1, 2, 3, 0}; // OUT, IN, BOTH, NONE as (out | in << 1)
    std::vector<KdbGraphStaged> st;
    for (uint32_t d = 0; d < 4; d++) {
        st.push_back(kdb_graph_stage_query(query(9, 99, d, 6), d));
        CHECK(st[d].root == 9 && st[d].dirs == dirs[d] && st[d].depth == (d == KDB_GDIR_NONE ? 0u : 5u) && st[d].and_idx == d && st[d].rel_mask == 6);
    }
    st.push_back(kdb_graph_stage_query(query(9, 2, KDB_GDIR_OUT, 1), KDB_NO_FILTER));
    CHECK(kdb_graph_levels(st.data(), 5) == 5 && kdb_graph_levels(st.data() + 3, 2) == 2 && kdb_graph_levels(st.data() + 3, 1) == 0 && kdb_graph_levels(st.data(), 0) == 0);
    // parts, their bounds, chunks of queries, the scratch layout
    const struct {
        uint64_t wpn;
        uint32_t Bc, n_cus;
        int32_t forced;
        uint32_t parts;
    } cases[] = {
        {156251, 1, 256, 0, 512}, {156251, 64, 256, 0, 8}, {156251, 1024, 256, 0, 1}, // 10M nodes: 2 per CU for the whole launch, at most 512
        {15626, 1, 256, 0, 61}, {94, 1, 256, 0, 1},                                  // at least KDB_GRAPH_MIN_WORDS_PER_PART words each
        {94, 12, 256, 3, 3}, {94, 12, 256, 512, 94}, {156251, 4096, 256, 100000, 512}, {1, 1, 256, 7, 1}, // forced: N, a part per word at most
    };
    for (const auto &c : cases) {
        const uint32_t parts = kdb_graph_parts(c.wpn, c.Bc, c.n_cus, c.forced);
        CHECK(parts == c.parts);
        uint64_t at = 0; // the bounds cover every word exactly once, in order
        for (uint32_t s = 0; s < parts; s++) {
            CHECK(kdb_graph_part_first(c.wpn, parts, s) == at && kdb_graph_part_first(c.wpn, parts, s + 1) >= at);
            at = kdb_graph_part_first(c.wpn, parts, s + 1);
        }
        CHECK(at == c.wpn);
    }
    CHECK(kdb_graph_chunk_queries(37, 3, 5 * 2 * 3 * 8) == 5 && kdb_graph_chunk_queries(37, 3, 5 * 2 * 3 * 8 - 1) == 4 && kdb_graph_chunk_queries(37, 3, 1) == 1);
    CHECK(kdb_graph_chunk_queries(4096, 156251, KDB_GRAPH_SCRATCH_MAX) == 107 && kdb_graph_chunk_queries(64, 15626, KDB_GRAPH_SCRATCH_MAX) == 64);
    const KdbGraphScratch L = kdb_graph_scratch(37, 5, 3); // 37 * 24 = 888 -> 1024; 5 * 3 * 8 = 120 -> 256
    CHECK(L.o_queries == 0 && L.o_f0 == 1024 && L.o_f1 == 1280 && L.total == 1536);
    // validation of views and queries
    std::vector<uint64_t> off = {0, 0, 2, 2, 3};
    std::vector<uint32_t> dst = {3, 1, 3};
    std::vector<uint8_t> rel = {0, 63, 5};
    kdb_relations_view v{3, 0, off.data(), dst.data(), rel.data()};
    uint64_t bad = 99;
    auto is = [&](int rc) { return kdb_graph_validate_view(&v, &bad) == rc; };
    CHECK(is(KDB_GRAPH_OK) && kdb_graph_validate_view(nullptr, &bad) == KDB_GRAPH_BAD_VIEW); // a self loop (3 -> 3), codes 0 and 63: legal
    CHECK((v.n_nodes = 0, is(KDB_GRAPH_BAD_VIEW)) && (v.n_nodes = 3, off[1] = 1, is(KDB_GRAPH_BAD_OFFSETS)));
    CHECK((off[1] = 0, off[3] = 1, is(KDB_GRAPH_BAD_OFFSETS)) && bad == 2);
    CHECK((off[3] = 2, dst[1] = 0, is(KDB_GRAPH_BAD_DST)) && bad == 1 && (dst[1] = 4, is(KDB_GRAPH_BAD_DST)));
    CHECK((dst[1] = 1, rel[2] = 64, is(KDB_GRAPH_BAD_REL)) && bad == 2 && (rel[2] = 5, v.dst = nullptr, is(KDB_GRAPH_BAD_VIEW)));

    std::vector<kdb_graph_query> q = {query(0, 1, KDB_GDIR_OUT, 1), query(8, 1, KDB_GDIR_NONE, 0)};
    const uint32_t and_of[2] = {KDB_NO_FILTER, 2};
    uint32_t at = 99;
    CHECK(kdb_graph_validate_queries(q.data(), 2, 8, and_of, 3, &at) == KDB_GRAPH_OK);
    CHECK(kdb_graph_validate_queries(q.data(), 2, 8, and_of, 2, &at) == KDB_GRAPH_BAD_AND && at == 1);
    CHECK(kdb_graph_validate_queries(q.data(), 2, 7, nullptr, 0, &at) == KDB_GRAPH_BAD_ROOT && at == 1);
    CHECK((q[0].direction = 4, kdb_graph_validate_queries(q.data(), 2, 8, nullptr, 0, &at)) == KDB_GRAPH_BAD_DIR && at == 0);
    CHECK(kdb_graph_validate_queries(q.data(), 0, 8, nullptr, 0, &at) == KDB_GRAPH_BAD_COUNTS && kdb_graph_validate_queries(nullptr, 1, 8, nullptr, 0, &at) == KDB_GRAPH_BAD_COUNTS &&
          kdb_graph_validate_queries(q.data(), KDB_GRAPH_MAX_QUERIES + 1, 8, nullptr, 0, &at) == KDB_GRAPH_BAD_COUNTS);
    printf("ok\n");
    return 0;
}
