// graph_filter.hip -- graph filters on the device: the allow list that resolveGraphFilter (pkg/engine/graph.go:173-246) builds on the
// host with a FIFO queue, Go maps and string ids, written by a level-synchronous BFS on bitmaps over the relation CSR in HBM, in the
// dense layout every filtered entry point takes.
//
//   graph_init_kernel    every word of the lists and of both frontiers: zero, or the root's bit (lists and F0)
//   graph_level_kernel   (part, query) per workgroup: one BFS level -- sweep the frontier, expand, mark the newly seen
//   graph_finish_kernel  one lane per list word: bit 0 and the bits above count cleared, the and-list, the cardinality
//
// Semantics, geometry, chunking, validation and the scratch layout are kdb_graph_plan.h's; the sweep of a frontier -- words coalesced,
// light nodes by their lanes, heavier ones through the hub queue in LDS, the rounds and their barriers -- is kdb_graph_sweep.cuh's,
// shared with subgraph.hip.  This file holds the filter's own: what a visited edge does, and the launcher.
// The result is a SET: V only ever gains bits, a node enters the next frontier exactly once (the lane whose atomicOr on V saw the
// bit clear), so nothing depends on the order in which the atomics land.
#include "kdb_graph_sweep.cuh"
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_init_kernel(const KdbGraphStaged *__restrict__ queries, unsigned long long *__restrict__ lists, uint64_t wpl, unsigned long long *__restrict__ f0,
                  unsigned long long *__restrict__ f1, uint64_t wpn, uint32_t *__restrict__ card) {
    const uint32_t b = blockIdx.y;
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    const unsigned long long seed = kdb_graph_seed_word(queries[b].root, w);
    if (w < wpl) lists[(uint64_t)b * wpl + w] = seed;
    if (w < wpn) {
        f0[(uint64_t)b * wpn + w] = seed;
        f1[(uint64_t)b * wpn + w] = 0ull;
    }
    if (card && w == 0u) card[b] = 0u;
}

// One edge: the relation test, a plain load of the visited word (most edges of a dense level end here), else the bit into V and --
// for the lane that set it, unless no level follows -- into the next frontier.  v is a dst of the snapshot: 1 <= v <= n_nodes, checked
// at upload, so its word lies inside both bitmaps; r < 64 likewise.
__device__ __forceinline__ void graph_visit(uint32_t v, uint32_t r, uint64_t rel_mask, unsigned long long *V, unsigned long long *Fn, bool last) {
    if (!((rel_mask >> r) & 1ull)) return;
    const unsigned long long bit = 1ull << (v & 63u);
    unsigned long long *const vw = V + (v >> 6);
    if (*vw & bit) return;
    if (!(atomicOr(vw, bit) & bit) && !last) atomicOr(Fn + (v >> 6), bit);
}
// the sweep's visitor: a set needs no company of the wave's other lanes, so each lane visits its own entries
struct GraphVisitor {
    static constexpr bool converged = false;
    uint64_t rel_mask;
    unsigned long long *V, *Fn;
    bool last;
    __device__ __forceinline__ void operator()(bool act, uint32_t, uint32_t far, uint32_t r, uint32_t) const {
        if (act) graph_visit(far, r, rel_mask, V, Fn, last);
    }
};

// Workgroup (s, b): level `level` of query b over words [first(s), first(s + 1)) of its current frontier, which is zeroed as it is
// read: kdb_csr_sweep (kdb_graph_sweep.cuh) in the directions the query follows, every CSR entry to graph_visit.
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_level_kernel(const KdbRelDev g, const KdbGraphStaged *__restrict__ queries, uint32_t level, uint32_t parts, unsigned long long *lists, uint64_t wpl,
                   unsigned long long *f_cur, unsigned long long *f_next, uint64_t wpn) {
    __shared__ KdbHubQueue s_hubs;
    const uint32_t b = blockIdx.y, depth = queries[b].depth;
    if (level >= depth) return; // (the whole workgroup)
    const GraphVisitor visit{queries[b].rel_mask, lists + (uint64_t)b * wpl, f_next + (uint64_t)b * wpn, level + 1u >= depth};
    kdb_csr_sweep<true>(g, f_cur + (uint64_t)b * wpn, wpn, parts, queries[b].dirs, s_hubs, visit);
}

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_finish_kernel(const KdbGraphStaged *__restrict__ queries, unsigned long long *__restrict__ lists, uint64_t wpl, uint32_t count,
                    const unsigned long long *__restrict__ and_lists, uint32_t *__restrict__ card) {
    const uint32_t b = blockIdx.y, a = queries[b].and_idx;
    kdb_graph_finish_word(lists + (uint64_t)b * wpl, wpl, count, and_lists && a != KDB_NO_FILTER ? and_lists + (uint64_t)a * wpl : nullptr,
                          card ? card + b : nullptr);
}

} // namespace

int kdb_launch_graph_filter(kdb_index *idx, const kdb_graph_query *queries, uint32_t B, uint64_t *d_lists, uint64_t words_per_list, uint32_t *d_card,
                            const uint64_t *d_and_lists, const uint32_t *and_of_query, hipStream_t s) {
    const KdbRelDev &g = idx->relations.dev;
    const uint64_t wpn = kdb_graph_wpn(g.n_nodes), wpl = words_per_list;
    std::vector<KdbGraphStaged> staged(B);
    for (uint32_t b = 0; b < B; b++) staged[b] = kdb_graph_stage_query(queries[b], d_and_lists && and_of_query ? and_of_query[b] : KDB_NO_FILTER);
    const uint32_t Bc = kdb_graph_chunk_queries(B, wpn, (uint64_t)kdb_graph_env("KDB_GRAPH_SCRATCH_MAX", (long long)KDB_GRAPH_SCRATCH_MAX));
    const int32_t forced = (int32_t)std::min<long long>(kdb_graph_env("KDB_GRAPH_PARTS", 0), KDB_GRAPH_MAX_PARTS);
    const KdbGraphScratch L = kdb_graph_scratch(B, Bc, wpn);
    const int rc = kdb_ensure_scratch(idx, (size_t)L.total);
    if (rc) return rc;
    unsigned char *const d = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch);
    const KdbGraphStaged *const d_q = reinterpret_cast<const KdbGraphStaged *>(d + L.o_queries);
    unsigned long long *const f0 = reinterpret_cast<unsigned long long *>(d + L.o_f0), *const f1 = reinterpret_cast<unsigned long long *>(d + L.o_f1);
    // (pageable memory: consumed before hipMemcpyAsync returns, like the programs of kdb_launch_filter_eval)
    KDB_HIP(hipMemcpyAsync(d + L.o_queries, staged.data(), (size_t)B * sizeof(KdbGraphStaged), hipMemcpyHostToDevice, s));
    const unsigned word_blocks = (unsigned)((wpl + KDB_GRAPH_BLOCK - 1u) / KDB_GRAPH_BLOCK);
    for (uint32_t c0 = 0; c0 < B; c0 += Bc) { // chunks of queries, one behind the other on the stream: they share the frontiers
        const uint32_t n = std::min(Bc, B - c0);
        unsigned long long *const lists = reinterpret_cast<unsigned long long *>(d_lists) + (uint64_t)c0 * wpl;
        uint32_t *const card = d_card ? d_card + c0 : nullptr;
        hipLaunchKernelGGL(graph_init_kernel, dim3(word_blocks, n), dim3(KDB_GRAPH_BLOCK), 0, s, d_q + c0, lists, wpl, f0, f1, wpn, card);
        const uint32_t levels = kdb_graph_levels(staged.data() + c0, n), parts = kdb_graph_parts(wpn, n, (uint32_t)idx->n_cu, forced);
        for (uint32_t level = 0; level < levels; level++)
            hipLaunchKernelGGL(graph_level_kernel, dim3(parts, n), dim3(KDB_GRAPH_BLOCK), 0, s, g, d_q + c0, level, parts, lists, wpl, level & 1u ? f1 : f0,
                               level & 1u ? f0 : f1, wpn);
        hipLaunchKernelGGL(graph_finish_kernel, dim3(word_blocks, n), dim3(KDB_GRAPH_BLOCK), 0, s, d_q + c0, lists, wpl, idx->count,
                           reinterpret_cast<const unsigned long long *>(d_and_lists), card);
    }
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}
