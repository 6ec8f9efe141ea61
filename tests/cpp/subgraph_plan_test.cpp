// The plan of the subgraph kernels (kektordb_amd/csrc/kdb_subgraph_plan.h) on its own: no HIP, no library.
#include "kdb_subgraph_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) ((cond) ? (void)0 : exit((printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond), 1)))

static kdb_subgraph_query query(uint32_t root, int32_t depth, uint32_t flags, uint64_t mask, double thr) { return kdb_subgraph_query{root, depth, flags, 0, mask, thr}; }

int main() {
    // staging: the staged depth is 0 when nothing is followed, else the clamp; the guided bit and the threshold travel
    const KdbSubStaged st[5] = {kdb_subgraph_stage_query(query(0, 3, 0, 1, 0)), kdb_subgraph_stage_query(query(4, 3, 1, 0, 0.5)),
                                kdb_subgraph_stage_query(query(4, -1, 0, 1ull << 63, 0)), kdb_subgraph_stage_query(query(4, 99, 1, 6, 0.25)),
                                kdb_subgraph_stage_query(query(4, 2, 0, 6, 0))};
    CHECK(st[0].depth == 0 && st[1].depth == 0 && st[2].depth == 1 && st[3].depth == 5 && st[4].depth == 2 && st[3].root == 4 && st[3].guided == 1 && st[3].rel_mask == 6 && st[3].threshold == 0.25 && st[2].guided == 0);
    CHECK(kdb_subgraph_levels(st, 5) == 5 && kdb_subgraph_levels(st, 3) == 1 && kdb_subgraph_levels(st, 2) == 0 && kdb_subgraph_levels(st, 0) == 0);
    CHECK(!kdb_subgraph_any_guided(st, 3) && kdb_subgraph_any_guided(st, 4) && !kdb_subgraph_any_guided(st + 4, 1)); // (a guided query that follows nothing gates nothing)
    // chunking covers B exactly; the scratch regions are disjoint, in order and on 256-byte boundaries
    CHECK(kdb_subgraph_chunk_queries(37, 3, 5 * 5 * 3 * 8) == 5 && kdb_subgraph_chunk_queries(37, 3, 5 * 5 * 3 * 8 - 1) == 4 && kdb_subgraph_chunk_queries(37, 3, 1) == 1);
    for (const uint32_t B : {1u, 37u, 4096u}) {
        const uint32_t Bc = kdb_subgraph_chunk_queries(B, 15626, 1u << 20);
        uint32_t covered = 0;
        for (uint32_t c0 = 0; c0 < B; c0 += Bc) covered += B - c0 < Bc ? B - c0 : Bc;
        CHECK(covered == B && Bc >= 1 && Bc <= B);
    }
    const KdbSubScratch L = kdb_subgraph_scratch(37, 5, 3, 400); // 37 * 32 -> 1280; 37 * 400 -> 14848; 37 * 4 -> 256; 5 * 3 * 8 -> 256 each
    CHECK(L.o_queries == 0 && L.o_guides == 1280 && L.o_qnorm == 16128 && L.o_f0 == 16384 && L.o_f1 == 16640 && L.o_t == 16896 && L.o_p == 17152 && L.o_c == 17408 &&
          L.total == 17664 && kdb_subgraph_scratch(37, 5, 3, 0).o_f0 == 1280);
    // validation
    std::vector<kdb_subgraph_query> q = {query(0, 1, 0, 1, 0), query(8, 1, 1, 0, 0.5)};
    uint32_t at = 99;
    CHECK(kdb_subgraph_validate(q.data(), 2, 8, true, 1, &at) == KDB_SUBGRAPH_OK && kdb_subgraph_validate(q.data(), 2, 0xffffffffu, true, 0, &at) == KDB_SUBGRAPH_OK);
    CHECK(kdb_subgraph_validate(q.data(), 2, 8, false, 1, &at) == KDB_SUBGRAPH_NO_GUIDES && at == 1 && kdb_subgraph_validate(q.data(), 2, 7, true, 1, &at) == KDB_SUBGRAPH_BAD_ROOT && at == 1);
    CHECK(kdb_subgraph_validate(q.data(), 2, 64, true, 1, &at) == KDB_SUBGRAPH_BAD_WORDS && kdb_subgraph_validate(q.data(), 2, 8, true, KDB_GRAPH_MAX_WORDS + 1, &at) == KDB_SUBGRAPH_BAD_WORDS);
    CHECK((q[0].flags = 2, kdb_subgraph_validate(q.data(), 2, 8, true, 1, &at)) == KDB_SUBGRAPH_BAD_FLAGS && at == 0 &&
          (q[0].flags = 0, q[0].reserved = 1, kdb_subgraph_validate(q.data(), 2, 8, true, 1, &at)) == KDB_SUBGRAPH_BAD_FLAGS);
    CHECK(kdb_subgraph_validate(q.data(), 0, 8, true, 1, &at) == KDB_SUBGRAPH_BAD_COUNTS && kdb_subgraph_validate(nullptr, 1, 8, true, 1, &at) == KDB_SUBGRAPH_BAD_COUNTS &&
          kdb_subgraph_validate(q.data(), KDB_GRAPH_MAX_QUERIES + 1, 8, true, 1, &at) == KDB_SUBGRAPH_BAD_COUNTS);
    printf("ok\n");
    return 0;
}
