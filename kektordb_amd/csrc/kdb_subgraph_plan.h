// kdb_subgraph_plan.h -- the plan of the subgraph kernels (subgraph.hip): what a query stages, which launches a level needs, how a
// call is cut into chunks of queries, the scratch layout and the validation of a call.  The depth clamp, wpn, parts and
// kdb_graph_part_first are kdb_graph_plan.h's.  Shared by the host (kdb_api_relations.hip validates, subgraph.hip's launcher plans
// with it) and the kernels (which index with it).  Plain C++, no HIP header: tests/cpp/subgraph_plan_test.cpp builds it alone.
//
// GEOMETRY.  Engine.VExtractSubgraph (pkg/engine/graph.go:296-386) as a level-synchronous BFS on bitmaps over graph nodes.  Per
// query: V, the node set, IS the output bitmap (words_per_list words); F0, F1 (frontiers), T (far ends already tested against the
// guide), P (those that passed) and C (this level's candidates) are wpn words each in the lane's scratch.  init writes every word of
// all six and zeroes the counts.  Level L of a chunk is up to three launches on (parts, Bc) workgroups:
//   collect  guided queries: every edge in the mask out of F[L & 1] whose far end is not in T sets its bit in C
//   gate     guided queries: C swept word by word -- the word ORed into T and zeroed -- its nodes' rows against the guide, passes into P
//   expand   F[L & 1] swept and zeroed: every edge in the mask whose far end is in P (unguided: every edge in the mask) is one edge
//            record; a far end not in V enters V and, unless no level follows, F[(L + 1) & 1]
// finish masks V (bit 0 and the bits above n_nodes) and counts it.  A workgroup of level L returns at once for a query whose staged
// depth is <= L, and collect / gate for an unguided one; a chunk without a guided query launches neither.
#ifndef KDB_SUBGRAPH_PLAN_H
#define KDB_SUBGRAPH_PLAN_H
#include "kdb_graph_plan.h"

constexpr uint32_t KDB_SUBGRAPH_F_GUIDED = 1u;       // kdb_subgraph_query.flags, bit 0
constexpr double KDB_SUBGRAPH_NOT_LIVE = 999999.0;   // computeDistance for a node GetNodeData does not find (ops.go:1774-1781)
constexpr uint32_t KDB_SUBGRAPH_BITMAPS = 5u;        // F0, F1, T, P, C
// UNMEASURED: where the design started; scripts/subgraph_probe.py measures it.
constexpr uint32_t KDB_SUBGRAPH_GATE_BATCH = 1024u;  // node ids of one gate batch in LDS: 4 KB, 64 trips of 16 rows
constexpr uint64_t KDB_SUBGRAPH_GUIDE_MAX = 48u << 10; // bytes of a prepared guide the gate holds in LDS beside its batch: 12288 float32 columns
static_assert(KDB_SUBGRAPH_GATE_BATCH >= KDB_GRAPH_WAVE, "after a drain the nodes of any one candidate word fit the batch");
static_assert(sizeof(kdb_subgraph_query) == 32u, "kdb_subgraph_query is 32 bytes");
static_assert(sizeof(kdb_subgraph_edge) == 12u, "kdb_subgraph_edge is 12 bytes");

// the third word of an edge record: relation code | direction << 8 (0 out, 1 in) | the level that found it << 16
KDB_GRAPH_HD constexpr uint32_t kdb_subgraph_edge_info(uint32_t rel, uint32_t dir, uint32_t level) { return rel | (dir << 8) | (level << 16); }

// what the kernels read per query (32 bytes, staged in front of the guides)
struct KdbSubStaged {
    uint32_t root;   // 0: the result is empty
    uint32_t depth;  // levels that expand: 0 = follows nothing (root 0, empty mask), else the clamped max_depth
    uint32_t guided; // 1: far ends are gated by `threshold`
    uint32_t pad;
    uint64_t rel_mask;
    double threshold;
};
static_assert(sizeof(KdbSubStaged) == 32u, "KdbSubStaged is 32 bytes");
KDB_GRAPH_HD constexpr KdbSubStaged kdb_subgraph_stage_query(const kdb_subgraph_query &q) {
    return KdbSubStaged{q.root, q.root == 0u || q.rel_mask == 0u ? 0u : kdb_graph_clamp_depth(q.max_depth), q.flags & KDB_SUBGRAPH_F_GUIDED, 0u, q.rel_mask,
                        q.threshold};
}
// per chunk: the level launches (the largest staged depth) and whether collect and gate are launched at all
inline uint32_t kdb_subgraph_levels(const KdbSubStaged *q, uint32_t n) {
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; i++) most = q[i].depth > most ? q[i].depth : most;
    return most;
}
inline bool kdb_subgraph_any_guided(const KdbSubStaged *q, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (q[i].guided && q[i].depth) return true;
    return false;
}

// the next run of consecutive guided queries at or behind `from`: [*b0, *b1), false when there is none.  Only these rows of `guides`
// are ever read -- copied, prepared --, one run at a time
inline bool kdb_subgraph_guided_run(const kdb_subgraph_query *q, uint32_t B, uint32_t from, uint32_t *b0, uint32_t *b1) {
    while (from < B && !(q[from].flags & KDB_SUBGRAPH_F_GUIDED)) from++;
    *b0 = *b1 = from;
    while (*b1 < B && (q[*b1].flags & KDB_SUBGRAPH_F_GUIDED)) ++*b1;
    return *b0 < B;
}

// queries per chunk: as many as keep the five bitmaps of the chunk within scratch_max bytes, at least one, at most B
KDB_GRAPH_HD constexpr uint32_t kdb_subgraph_chunk_queries(uint32_t B, uint64_t wpn, uint64_t scratch_max) {
    const uint64_t per_query = (uint64_t)KDB_SUBGRAPH_BITMAPS * wpn * 8u, fit = scratch_max / per_query;
    return fit < 1u ? 1u : fit > B ? B : (uint32_t)fit;
}
// the lane's scratch: staged queries of the call | prepared guides of the call (guide_row bytes each; none: 0) | their norms |
// F0 | F1 | T | P | C of a chunk; every region on a 256-byte boundary
struct KdbSubScratch {
    uint64_t o_queries, o_guides, o_qnorm, o_f0, o_f1, o_t, o_p, o_c, total;
};
KDB_GRAPH_HD constexpr KdbSubScratch kdb_subgraph_scratch(uint32_t B, uint32_t Bc, uint64_t wpn, uint64_t guide_row) {
    KdbSubScratch L{};
    const uint64_t bm = kdb_graph_align((uint64_t)Bc * wpn * 8u);
    L.o_queries = 0;
    L.o_guides = kdb_graph_align((uint64_t)B * sizeof(KdbSubStaged));
    L.o_qnorm = L.o_guides + kdb_graph_align((uint64_t)B * guide_row);
    L.o_f0 = L.o_qnorm + kdb_graph_align(guide_row ? (uint64_t)B * 4u : 0u);
    L.o_f1 = L.o_f0 + bm;
    L.o_t = L.o_f1 + bm;
    L.o_p = L.o_t + bm;
    L.o_c = L.o_p + bm;
    L.total = L.o_c + bm;
    return L;
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
enum {
    KDB_SUBGRAPH_OK = 0,
    KDB_SUBGRAPH_BAD_COUNTS = 1, // null queries, B outside 1..KDB_GRAPH_MAX_QUERIES
    KDB_SUBGRAPH_BAD_ROOT = 2,   // a root above n_nodes
    KDB_SUBGRAPH_BAD_FLAGS = 3,  // a flag bit other than bit 0, or a reserved word that is not 0
    KDB_SUBGRAPH_NO_GUIDES = 4,  // a guided query and no guides
    KDB_SUBGRAPH_BAD_WORDS = 5   // words_per_list below (n_nodes >> 6) + 1 or above 2^30
};
// n_nodes: of the snapshot the call runs on (0xffffffff before the index is looked at: everything but the roots and the words is
// judged; words_per_list is then only held to its upper bound).  *bad: the query at which the check failed.
inline int kdb_subgraph_validate(const kdb_subgraph_query *q, uint32_t B, uint32_t n_nodes, bool have_guides, uint64_t words_per_list, uint32_t *bad) {
    if (bad) *bad = 0;
    if (!q || B == 0u || B > KDB_GRAPH_MAX_QUERIES) return KDB_SUBGRAPH_BAD_COUNTS;
    if (words_per_list > KDB_GRAPH_MAX_WORDS || (n_nodes != 0xffffffffu && words_per_list < kdb_graph_wpn(n_nodes))) return KDB_SUBGRAPH_BAD_WORDS;
    for (uint32_t b = 0; b < B; b++) {
        if (bad) *bad = b;
        if ((q[b].flags & ~KDB_SUBGRAPH_F_GUIDED) || q[b].reserved) return KDB_SUBGRAPH_BAD_FLAGS;
        if ((q[b].flags & KDB_SUBGRAPH_F_GUIDED) && !have_guides) return KDB_SUBGRAPH_NO_GUIDES;
        if (q[b].root > n_nodes) return KDB_SUBGRAPH_BAD_ROOT;
    }
    return KDB_SUBGRAPH_OK;
}
inline const char *kdb_subgraph_strerror(int rc) {
    switch (rc) {
    case KDB_SUBGRAPH_OK: return "ok";
    case KDB_SUBGRAPH_BAD_COUNTS: return "null queries, or B outside 1..4096";
    case KDB_SUBGRAPH_BAD_ROOT: return "a root above n_nodes";
    case KDB_SUBGRAPH_BAD_FLAGS: return "flags other than bit 0 (guided), or a reserved word that is not 0";
    case KDB_SUBGRAPH_NO_GUIDES: return "a guided query and null guides";
    case KDB_SUBGRAPH_BAD_WORDS: return "words_per_list outside (n_nodes>>6)+1 .. 2^30";
    }
    return "?";
}

#endif
