// kdb_graph_plan.h -- the plan of the graph-filter kernels (graph_filter.hip): the depth clamp, which queries follow nothing, the
// words of a frontier and of a list, how a level's sweep is cut into parts, how a call is cut into chunks of queries, the scratch
// layout, and the validation of an uploaded snapshot and of a call's queries.  Shared by the host (kdb_api_relations.hip validates,
// graph_filter.hip's launcher plans with it) and the kernels (which index with it).  Plain C++, no HIP header:
// tests/cpp/graph_plan_test.cpp builds it alone.
//
// GEOMETRY.  A level-synchronous BFS on bitmaps.  The visited set of query b IS its output list V[b] (words_per_list words, indexed by
// graph node); two frontier bitmaps F0[b], F1[b] of wpn = (n_nodes >> 6) + 1 words sit in the lane's scratch.  graph_init_kernel
// writes every word of all three; level L (one launch, grid (parts, Bc), 256 lanes) sweeps F[L & 1], writes zero over every
// non-zero word it consumes -- so the bitmap is clean again when level L + 1 fills it for level L + 2 -- and sets the bits of newly
// seen nodes in V and F[(L + 1) & 1]; graph_finish_kernel masks, ANDs and counts.  A workgroup of level L returns at once for a
// query whose staged depth is <= L: the staged depth is the clamped max_depth, or 0 for a query that follows nothing.
#ifndef KDB_GRAPH_PLAN_H
#define KDB_GRAPH_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/kektor_hip.h"

#if defined(__HIPCC__)
#define KDB_GRAPH_HD __host__ __device__
#else
#define KDB_GRAPH_HD
#endif

constexpr uint32_t KDB_GRAPH_BLOCK = 256u;              // lanes of a workgroup: four waves
constexpr uint32_t KDB_GRAPH_WAVE = 64u;                // a wave loads 64 consecutive frontier words, one per lane
constexpr uint32_t KDB_GRAPH_MAX_DEPTH = 5u;            // graph.go:185-190
constexpr uint32_t KDB_GRAPH_MAX_NODES = 0x80000000u;   // 2^31
constexpr uint32_t KDB_GRAPH_MAX_PARTS = 512u;
constexpr uint32_t KDB_GRAPH_WG_PER_CU = 2u;            // about two workgroups per CU for the whole launch
// UNMEASURED: the three values below are where the design started; scripts/graph_filter_probe.py measures them.
constexpr uint32_t KDB_GRAPH_MIN_WORDS_PER_PART = 256u; // one trip of the four waves: 2 KB of frontier
constexpr uint32_t KDB_GRAPH_LIGHT_DEG = 16u;           // edges a lane expands by itself; a heavier node goes to the hub queue
constexpr uint32_t KDB_GRAPH_HUB_CAP = 256u;            // (begin, end) records of the hub queue in LDS
constexpr uint64_t KDB_GRAPH_SCRATCH_MAX = 256ull << 20; // frontier bytes of one chunk of queries
constexpr uint64_t KDB_GRAPH_MAX_WORDS = (uint64_t)1 << 30; // the largest words_per_list, as for kdb_filter_eval
static_assert(KDB_GRAPH_HUB_CAP >= 2u * KDB_GRAPH_WAVE, "after a drain a wave's heavy nodes of one word, both directions, always fit");
static_assert(KDB_GRAPH_MAX_RELATIONS == 64u, "a query's relation set is one 64-bit mask");
static_assert(sizeof(kdb_graph_query) == 24u, "kdb_graph_query is 24 bytes");

// graph.go:185-190
KDB_GRAPH_HD constexpr uint32_t kdb_graph_clamp_depth(int32_t max_depth) {
    return max_depth <= 0 ? 1u : max_depth > (int32_t)KDB_GRAPH_MAX_DEPTH ? KDB_GRAPH_MAX_DEPTH : (uint32_t)max_depth;
}
KDB_GRAPH_HD constexpr bool kdb_graph_follows_out(uint32_t direction) { return direction == KDB_GDIR_OUT || direction == KDB_GDIR_BOTH; }
KDB_GRAPH_HD constexpr bool kdb_graph_follows_in(uint32_t direction) { return direction == KDB_GDIR_IN || direction == KDB_GDIR_BOTH; }
// no edge can be followed: the allowed set is the root alone (an unknown direction string, an empty relation set) or nothing (root 0)
KDB_GRAPH_HD constexpr bool kdb_graph_follows_nothing(const kdb_graph_query &q) {
    return q.root == 0u || q.rel_mask == 0u || !(kdb_graph_follows_out(q.direction) || kdb_graph_follows_in(q.direction));
}
// what the kernels read per query (24 bytes, staged in front of the frontiers)
struct KdbGraphStaged {
    uint32_t root;    // 0: the list is empty
    uint32_t depth;   // levels that expand: 0 = follows nothing, else the clamped max_depth
    uint32_t dirs;    // bit 0: out-edges, bit 1: in-edges
    uint32_t and_idx; // KDB_NO_FILTER: none
    uint64_t rel_mask;
};
static_assert(sizeof(KdbGraphStaged) == 24u, "KdbGraphStaged is 24 bytes");
KDB_GRAPH_HD constexpr KdbGraphStaged kdb_graph_stage_query(const kdb_graph_query &q, uint32_t and_idx) {
    return KdbGraphStaged{q.root, kdb_graph_follows_nothing(q) ? 0u : kdb_graph_clamp_depth(q.max_depth),
                          (kdb_graph_follows_out(q.direction) ? 1u : 0u) | (kdb_graph_follows_in(q.direction) ? 2u : 0u), and_idx, q.rel_mask};
}

// words of a frontier bitmap over nodes 0..n_nodes; the fewest words of a list over ids 0..count that can also be the visited set
KDB_GRAPH_HD constexpr uint64_t kdb_graph_wpn(uint32_t n_nodes) { return ((uint64_t)n_nodes >> 6) + 1u; }
KDB_GRAPH_HD constexpr uint64_t kdb_graph_min_words(uint32_t count, uint32_t n_nodes) { return kdb_graph_wpn(count > n_nodes ? count : n_nodes); }
// word w of a finished list: bit 0 and the bits above count cleared
KDB_GRAPH_HD constexpr uint64_t kdb_graph_live_mask(uint64_t w, uint32_t count) {
    const uint64_t last = (uint64_t)count >> 6;
    const uint64_t m = w > last ? 0ull : w < last ? ~0ull : (2ull << (count & 63u)) - 1ull; // (2 << 63 wraps to 0: all ones)
    return w == 0u ? m & ~1ull : m;
}

// an environment override read per call (tests toggle it inside one process); unset or not a positive number: `unset`
inline long long kdb_graph_env(const char *name, long long unset) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? v : unset;
}

// ---- parts: the workgroups that share one query's sweep ---------------------------------------------------------------------------
// forced: KDB_GRAPH_PARTS, < 1 = unset.  Unforced: about KDB_GRAPH_WG_PER_CU workgroups per CU for the whole launch of Bc queries, at
// least KDB_GRAPH_MIN_WORDS_PER_PART words each.  Always 1 <= parts <= min(KDB_GRAPH_MAX_PARTS, wpn).
KDB_GRAPH_HD constexpr uint32_t kdb_graph_parts(uint64_t wpn, uint32_t Bc, uint32_t n_cus, int32_t forced) {
    uint64_t parts = 1;
    if (forced >= 1) {
        parts = (uint64_t)forced;
    } else if (Bc) {
        parts = ((uint64_t)KDB_GRAPH_WG_PER_CU * n_cus + Bc - 1u) / Bc;
        if (parts > wpn / KDB_GRAPH_MIN_WORDS_PER_PART) parts = wpn / KDB_GRAPH_MIN_WORDS_PER_PART;
    }
    if (parts > KDB_GRAPH_MAX_PARTS) parts = KDB_GRAPH_MAX_PARTS;
    if (parts > wpn) parts = wpn;
    return parts < 1u ? 1u : (uint32_t)parts;
}
// part s of `parts` sweeps words [first(s), first(s + 1)): equal slices, the last ones shorter or empty
KDB_GRAPH_HD constexpr uint64_t kdb_graph_part_first(uint64_t wpn, uint32_t parts, uint32_t s) {
    const uint64_t per = (wpn + parts - 1u) / parts, a = per * s;
    return a < wpn ? a : wpn;
}

// ---- chunks of queries, levels, scratch -------------------------------------------------------------------------------------------
// queries per chunk: as many as keep both frontiers of the chunk within scratch_max bytes, at least one, at most B
KDB_GRAPH_HD constexpr uint32_t kdb_graph_chunk_queries(uint32_t B, uint64_t wpn, uint64_t scratch_max) {
    const uint64_t per_query = 2u * wpn * 8u, fit = scratch_max / per_query;
    return fit < 1u ? 1u : fit > B ? B : (uint32_t)fit;
}
// level launches of a chunk: the largest staged depth among its queries
inline uint32_t kdb_graph_levels(const KdbGraphStaged *q, uint32_t n) {
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; i++) most = q[i].depth > most ? q[i].depth : most;
    return most;
}
// the lane's scratch: the staged queries of the whole call | F0 of a chunk | F1 of a chunk; every region on a 256-byte boundary
struct KdbGraphScratch {
    uint64_t o_queries, o_f0, o_f1, total;
};
KDB_GRAPH_HD constexpr uint64_t kdb_graph_align(uint64_t b) { return (b + 255u) & ~(uint64_t)255u; }
KDB_GRAPH_HD constexpr KdbGraphScratch kdb_graph_scratch(uint32_t B, uint32_t Bc, uint64_t wpn) {
    KdbGraphScratch L{};
    L.o_queries = 0;
    L.o_f0 = kdb_graph_align((uint64_t)B * sizeof(KdbGraphStaged));
    L.o_f1 = L.o_f0 + kdb_graph_align((uint64_t)Bc * wpn * 8u);
    L.total = L.o_f1 + kdb_graph_align((uint64_t)Bc * wpn * 8u);
    return L;
}

// ---- validation -------------------------------------------------------------------------------------------------------------------
enum {
    KDB_GRAPH_OK = 0,
    KDB_GRAPH_BAD_VIEW = 1,    // a null view or array, n_nodes of 0 or above 2^31
    KDB_GRAPH_BAD_OFFSETS = 2, // offsets that do not start at 0 (node 0 has no edges) or decrease
    KDB_GRAPH_BAD_DST = 3,     // an edge to node 0 or above n_nodes
    KDB_GRAPH_BAD_REL = 4,     // a relation code >= KDB_GRAPH_MAX_RELATIONS
    KDB_GRAPH_BAD_COUNTS = 5,  // null queries, B outside 1..KDB_GRAPH_MAX_QUERIES
    KDB_GRAPH_BAD_ROOT = 6,    // a root above n_nodes
    KDB_GRAPH_BAD_DIR = 7,     // a direction above KDB_GDIR_NONE
    KDB_GRAPH_BAD_AND = 8      // and_of_query[b] names no list
};
// *bad: the node (offsets) or the edge (dst, rel) at which the check failed
inline int kdb_graph_validate_view(const kdb_relations_view *v, uint64_t *bad) {
    if (bad) *bad = 0;
    if (!v || !v->off || v->n_nodes == 0u || v->n_nodes > KDB_GRAPH_MAX_NODES) return KDB_GRAPH_BAD_VIEW;
    if (v->off[0] != 0u || v->off[1] != 0u) return KDB_GRAPH_BAD_OFFSETS;
    for (uint64_t g = 1; g <= v->n_nodes; g++)
        if (v->off[g + 1] < v->off[g]) {
            if (bad) *bad = g;
            return KDB_GRAPH_BAD_OFFSETS;
        }
    const uint64_t E = v->off[(uint64_t)v->n_nodes + 1u];
    if (E && (!v->dst || !v->rel)) return KDB_GRAPH_BAD_VIEW;
    for (uint64_t e = 0; e < E; e++) {
        if (bad) *bad = e;
        if (v->dst[e] == 0u || v->dst[e] > v->n_nodes) return KDB_GRAPH_BAD_DST;
        if (v->rel[e] >= KDB_GRAPH_MAX_RELATIONS) return KDB_GRAPH_BAD_REL;
    }
    return KDB_GRAPH_OK;
}
// n_nodes: of the snapshot the call runs on (0xffffffff before the index is looked at: everything but the roots is judged);
// and_of_query: NULL or B entries, each KDB_NO_FILTER or below n_and_lists.  *bad: the query at which the check failed.
inline int kdb_graph_validate_queries(const kdb_graph_query *q, uint32_t B, uint32_t n_nodes, const uint32_t *and_of_query, uint32_t n_and_lists,
                                      uint32_t *bad) {
    if (bad) *bad = 0;
    if (!q || B == 0u || B > KDB_GRAPH_MAX_QUERIES) return KDB_GRAPH_BAD_COUNTS;
    for (uint32_t b = 0; b < B; b++) {
        if (bad) *bad = b;
        if (q[b].direction > KDB_GDIR_NONE) return KDB_GRAPH_BAD_DIR;
        if (q[b].root > n_nodes) return KDB_GRAPH_BAD_ROOT;
        if (and_of_query && and_of_query[b] != KDB_NO_FILTER && and_of_query[b] >= n_and_lists) return KDB_GRAPH_BAD_AND;
    }
    return KDB_GRAPH_OK;
}
inline const char *kdb_graph_strerror(int rc) {
    switch (rc) {
    case KDB_GRAPH_OK: return "ok";
    case KDB_GRAPH_BAD_VIEW: return "null view or array, or n_nodes outside 1..2^31";
    case KDB_GRAPH_BAD_OFFSETS: return "offsets must start at 0 (node 0 has no edges) and never decrease";
    case KDB_GRAPH_BAD_DST: return "an edge leads to node 0 or above n_nodes";
    case KDB_GRAPH_BAD_REL: return "a relation code is 64 or more";
    case KDB_GRAPH_BAD_COUNTS: return "null queries, or B outside 1..4096";
    case KDB_GRAPH_BAD_ROOT: return "a root above n_nodes";
    case KDB_GRAPH_BAD_DIR: return "a direction above KDB_GDIR_NONE";
    case KDB_GRAPH_BAD_AND: return "and_of_query names no list (KDB_NO_FILTER or an index below n_and_lists)";
    }
    return "?";
}

#endif
