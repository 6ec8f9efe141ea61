// subgraph.hip -- subgraph extraction on the device: Engine.VExtractSubgraph (pkg/engine/graph.go:296-386), the guided BFS whose
// shouldTraverse calls hnsw.Index.ComputeDistanceToVector once per EDGE (ops.go:1763-1789, hnsw_index.go:3381-3468), as a
// level-synchronous BFS on bitmaps over the relation CSR in HBM that reads a far end's row once per QUERY.
//
//   subgraph_init_kernel    every word of V, F0, F1, T, P and C: zero, or the root's bit (V and F0); the counts zero
//   subgraph_level_kernel   (part, query) per workgroup, one sweep of the frontier in two modes:
//       COLLECT  (guided)   every edge in the mask whose far end is not in T sets its bit in C; the frontier is left as it is
//       EXPAND              the frontier is zeroed as it is read; every edge in the mask whose far end is in P (unguided: every edge
//                           in the mask) is one edge record, and its far end enters V and the next frontier if it is new
//   subgraph_gate_kernel    (part, query) per workgroup, guided: C word by word into batches of node ids in LDS, the four waves
//                           take the batch 4 * R rows at a time against the guide in LDS, passes go into P
//   subgraph_finish_kernel  one lane per word of V: bit 0 and the bits above n_nodes cleared, the node count
//
// Semantics, chunking, validation and the scratch layout are kdb_subgraph_plan.h's.  The sweep of a bitmap -- the rounds, the queue
// in LDS, the barriers -- and the expansion of a frontier over the CSR are kdb_graph_sweep.cuh's, shared with graph_filter.hip.
// Extraction's own: both directions always; sub_visit, which uses that the sweep's visits are wave-converged (EXPAND reserves edge
// slots with ONE atomic per wave and trip) and the source the hub queue keeps (an edge record names it); the gate's policy.  The
// result is a node SET and an edge MULTISET: V and P only ever gain bits, a node enters the next frontier exactly once, an edge
// record is written by the one lane that visits its CSR entry, so nothing depends on the order in which the atomics land.
#include "kdb_search_core.cuh" // kdb_trip_rows: the rows-per-trip table of compute_dists; kdb_device.cuh: the accumulate steps
#include "kdb_decode.cuh"      // kdb_row_found
#include "kdb_graph_sweep.cuh"
#include "kdb_subgraph_plan.h"
#include <algorithm>
#include <vector>

namespace {

enum { SUB_COLLECT = 0, SUB_EXPAND = 1 };

// what a workgroup knows about its query
struct SubCtx {
    uint64_t rel_mask;
    unsigned long long *V, *Fn, *T, *P, *C;
    uint32_t *n_edges;
    kdb_subgraph_edge *edges; // null: counts only
    uint32_t edge_cap, level;
    bool guided, last;
};

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_init_kernel(const KdbSubStaged *__restrict__ queries, unsigned long long *__restrict__ nodes, uint64_t wpl, unsigned long long *__restrict__ f0,
                     unsigned long long *__restrict__ f1, unsigned long long *__restrict__ bt, unsigned long long *__restrict__ bp,
                     unsigned long long *__restrict__ bc, uint64_t wpn, uint32_t *__restrict__ n_nodes, uint32_t *__restrict__ n_edges) {
    const uint32_t b = blockIdx.y;
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    const unsigned long long seed = kdb_graph_seed_word(queries[b].root, w);
    if (w < wpl) nodes[(uint64_t)b * wpl + w] = seed;
    if (w < wpn) {
        const uint64_t at = (uint64_t)b * wpn + w;
        f0[at] = seed;
        f1[at] = bt[at] = bp[at] = bc[at] = 0ull;
    }
    if (w == 0u) n_nodes[b] = n_edges[b] = 0u;
}

// One CSR entry of the expanded node `node`: far end `far`, relation r, direction dir (0: node -> far, 1: far -> node).  Called by
// ALL 64 lanes of a wave together, `act` says whose entry is real: the edge slots of a trip are reserved by lane 0 alone.
// far is a dst of the snapshot: 1 <= far <= n_nodes, checked at upload, so its word lies inside every bitmap; r < 64 likewise.
template <int MODE>
__device__ __forceinline__ void sub_visit(const SubCtx &c, bool act, uint32_t node, uint32_t far, uint32_t r, uint32_t dir) {
    act = act && ((c.rel_mask >> r) & 1ull);
    const unsigned long long bit = 1ull << (far & 63u);
    const uint32_t fw = far >> 6;
    if (MODE == SUB_COLLECT) { // plain loads first: most edges of a dense level end here
        if (act && !(c.T[fw] & bit) && !(c.C[fw] & bit)) atomicOr(c.C + fw, bit);
        return;
    }
    if (act && c.guided) act = (c.P[fw] & bit) != 0ull;
    const unsigned long long m = __ballot(act);
    if (!m) return;
    uint32_t base = 0;
    if (kdb_lane() == 0) base = atomicAdd(c.n_edges, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (!act) return;
    const uint32_t slot = base + kdb_mbcnt(m);
    if (c.edges && slot < c.edge_cap) {
        kdb_subgraph_edge rec;
        rec.src = dir ? far : node;
        rec.dst = dir ? node : far;
        rec.info = kdb_subgraph_edge_info(r, dir, c.level);
        c.edges[slot] = rec;
    }
    unsigned long long *const vw = c.V + fw; // graph_visit's idiom: the lane whose atomicOr saw the bit clear owns the node
    if (*vw & bit) return;
    if (!(atomicOr(vw, bit) & bit) && !c.last) atomicOr(c.Fn + fw, bit);
}
template <int MODE>
struct SubVisitor { // the sweep's visitor
    static constexpr bool converged = true;
    const SubCtx &c;
    __device__ __forceinline__ void operator()(bool act, uint32_t node, uint32_t far, uint32_t r, uint32_t dir) const { sub_visit<MODE>(c, act, node, far, r, dir); }
};

// Workgroup (s, b): words [first(s), first(s + 1)) of the current frontier of query b, zeroed as they are read in EXPAND only:
// kdb_csr_sweep (kdb_graph_sweep.cuh) in both directions, every CSR entry to sub_visit.
template <int MODE>
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_level_kernel(const KdbRelDev g, const KdbSubStaged *__restrict__ queries, uint32_t level, uint32_t parts, unsigned long long *nodes, uint64_t wpl,
                      unsigned long long *f_cur, unsigned long long *f_next, unsigned long long *bt, unsigned long long *bp, unsigned long long *bc,
                      uint64_t wpn, uint32_t *n_edges, kdb_subgraph_edge *edges, uint32_t edge_cap) {
    __shared__ KdbHubQueue s_hubs;
    const uint32_t b = blockIdx.y, depth = queries[b].depth;
    if (level >= depth || (MODE == SUB_COLLECT && !queries[b].guided)) return; // (the whole workgroup)
    SubCtx c;
    c.rel_mask = queries[b].rel_mask;
    c.V = nodes + (uint64_t)b * wpl, c.Fn = f_next + (uint64_t)b * wpn;
    c.T = bt + (uint64_t)b * wpn, c.P = bp + (uint64_t)b * wpn, c.C = bc + (uint64_t)b * wpn;
    c.n_edges = n_edges + b;
    c.edges = edges && edge_cap ? edges + (uint64_t)b * edge_cap : nullptr;
    c.edge_cap = edge_cap, c.level = level;
    c.guided = queries[b].guided != 0u, c.last = level + 1u >= depth;
    kdb_csr_sweep<MODE == SUB_EXPAND>(g, f_cur + (uint64_t)b * wpn, wpn, parts, 3u, s_hubs, SubVisitor<MODE>{c});
}

// ---- the gate ---------------------------------------------------------------------------------------------------------------------
// One trip of one wave: rows base + 4 r + g (r < R, g = the lane's 16-lane group) of the batch against the guide in LDS.  R is
// compute_dists' rows per trip for (precision, NCH); the loaders and the accumulate step are kdb_device.cuh's, so dot and sum are the
// walk's bits: every 16-byte load of the trip is issued before the first FMA, lane t of a group reads pieces t, t + 16, ...  A node
// that is not live (above count, deleted) reads row 0 (all zero, one cached row) and takes the constant instead of what comes out.
// The lane with t == 0 compares in float64 and sets the bit in P.
template <int PREC, int METRIC, int NCH>
__device__ __forceinline__ void gate_trip(const KdbView &v, const float *q, float qnorm, double threshold, const uint32_t *s_batch, uint32_t base,
                                          uint32_t nb, unsigned long long *P) {
    constexpr int R = kdbcore::kdb_trip_rows<PREC, NCH, 0>();
    const int lane = kdb_lane(), g = lane >> 4, t = lane & 15;
    uint32_t id[R];
    bool in[R], live[R];
    double d[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t rr = base + 4u * (uint32_t)r + (uint32_t)g;
        in[r] = rr < nb;
        id[r] = in[r] ? s_batch[rr] : 0u;
        live[r] = kdb_row_found(v, id[r]); // (the range check and the deleted bit before a row address is formed)
    }
    if constexpr (PREC == KDB_PREC_F32) {
        const float *rows[R];
        float p[R];
#pragma unroll
        for (int r = 0; r < R; r++) rows[r] = reinterpret_cast<const float *>(v.rows) + (size_t)(live[r] ? id[r] : 0u) * v.ld;
        if constexpr (NCH > 0) kdb_row_partialR_f32<METRIC, NCH, R>(rows, q, t, p, v.ld >> 2);
        else kdb_row_partialR_f32_dyn<METRIC, R, 8>(rows, q, v.ld >> 2, t, p);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float raw = kdb_reduce16(p[r]);
            d[r] = METRIC == KDB_METRIC_COSINE ? 1.0 - (double)raw : (double)raw; // distance_go.go:127 / :67
        }
    } else if constexpr (PREC == KDB_PREC_F16) {
        const uint16_t *rows[R];
        float p[R];
#pragma unroll
        for (int r = 0; r < R; r++) rows[r] = reinterpret_cast<const uint16_t *>(v.rows) + (size_t)(live[r] ? id[r] : 0u) * v.ld;
        kdb_row_partialR_f16_dyn<R, 4>(rows, q, v.ld >> 3, t, p);
#pragma unroll
        for (int r = 0; r < R; r++) d[r] = (double)kdb_reduce16(p[r]);
    } else {
        const int8_t *rows[R];
        int p[R];
#pragma unroll
        for (int r = 0; r < R; r++) rows[r] = reinterpret_cast<const int8_t *>(v.rows) + (size_t)(live[r] ? id[r] : 0u) * v.ld;
        kdb_row_partialR_i8_dyn<R, 4>(rows, reinterpret_cast<const int8_t *>(q), v.ld >> 4, t, p);
#pragma unroll
        for (int r = 0; r < R; r++) { // hnsw_index.go:3452-3464 (qnorm: float32, 0 -> 1, made by the preparation)
            const int dot = kdb_reduce16_i(p[r]);
            const float snorm = live[r] ? v.norms[id[r]] : 0.f;
            double sim = (double)dot / ((double)qnorm * (double)snorm);
            if (sim > 1.0) sim = 1.0;
            if (sim < -1.0) sim = -1.0;
            d[r] = snorm == 0.f ? 1.0 : 1.0 - sim;
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        double dd = qnorm > 0.f ? d[r] : (double)NAN; // a guide the preparation marked (a component that is not finite): nothing passes
        if (!live[r]) dd = KDB_SUBGRAPH_NOT_LIVE;
        if (t == 0 && in[r] && dd <= threshold) atomicOr(P + (id[r] >> 6), 1ull << (id[r] & 63u));
    }
}

// The gate's policy for kdb_sweep_rounds (kdb_graph_sweep.cuh): the queue is a batch of node ids in LDS.
//   load    the lane that reads a non-zero word of C ORs it into T and writes zero over it (only this workgroup touches these words
//           of T and C in this launch)
//   take    the wave reserves popcount(word) places of the batch and lane i writes node 64 j + i behind the set bits below it
//   drain   wave w takes trips w, w + 4, ... of the batch, 4 * R rows each (gate_trip): with R rows of every 16-lane group in
//           flight, a CU holds 16 * R row gathers per resident workgroup
template <int PREC, int METRIC, int NCH>
struct GateSweep {
    const KdbView &v;
    const float *guide; // in LDS
    float qnorm;
    double threshold;
    unsigned long long *T, *P, *C;
    uint32_t *s_batch, *s_n;

    __device__ __forceinline__ unsigned long long load(uint64_t w) const {
        const unsigned long long word = C[w];
        if (word) {
            T[w] |= word;
            C[w] = 0ull;
        }
        return word;
    }
    __device__ __forceinline__ bool take(uint64_t j, unsigned long long cw) const {
        const uint32_t slot = kdb_sweep_reserve(*s_n, (uint32_t)__popcll(cw), KDB_SUBGRAPH_GATE_BATCH);
        if (slot == KDB_SUBGRAPH_GATE_BATCH) return false;
        if ((cw >> kdb_lane()) & 1ull) s_batch[slot + kdb_mbcnt(cw)] = (uint32_t)(j * KDB_GRAPH_WAVE + (uint32_t)kdb_lane());
        return true;
    }
    __device__ __forceinline__ void drain(uint32_t nb) const {
        constexpr uint32_t TRIP = 4u * (uint32_t)kdbcore::kdb_trip_rows<PREC, NCH, 0>();
        for (uint32_t base = threadIdx.x / KDB_GRAPH_WAVE * TRIP; base < nb; base += 4u * TRIP)
            gate_trip<PREC, METRIC, NCH>(v, guide, qnorm, threshold, s_batch, base, nb, P);
    }
};

// Workgroup (s, b): words [first(s), first(s + 1)) of the candidate bitmap C of query b, level `level`: the prepared guide of the
// query, once per workgroup, into LDS (ld floats, or ld packed int8 values), then the sweep with GateSweep.
// A gather bound by HBM latency: no matrix instruction fits, every query has its own single guide.
template <int PREC, int METRIC, int NCH>
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_gate_kernel(const KdbView v, const KdbSubStaged *__restrict__ queries, const unsigned char *__restrict__ guides, const float *__restrict__ qnorms,
                     uint32_t guide_row, uint32_t level, uint32_t parts, unsigned long long *bt, unsigned long long *bp, unsigned long long *bc, uint64_t wpn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_guide[];
    __shared__ uint32_t s_batch[KDB_SUBGRAPH_GATE_BATCH];
    __shared__ uint32_t s_n;
    const uint32_t b = blockIdx.y;
    if (level >= queries[b].depth || !queries[b].guided) return; // (the whole workgroup)
    {
        const uint4 *const src = reinterpret_cast<const uint4 *>(guides + (size_t)b * guide_row); // (rows of 16-byte pieces on 256-byte regions)
        for (uint32_t i = threadIdx.x; i < (guide_row >> 4); i += KDB_GRAPH_BLOCK) reinterpret_cast<uint4 *>(s_guide)[i] = src[i];
    } // (visible behind the barrier the rounds open with)
    GateSweep<PREC, METRIC, NCH> p{v, reinterpret_cast<const float *>(s_guide), qnorms[b], queries[b].threshold, bt + (uint64_t)b * wpn,
                                   bp + (uint64_t)b * wpn, bc + (uint64_t)b * wpn, s_batch, &s_n};
    kdb_sweep_rounds(kdb_graph_part_first(wpn, parts, blockIdx.x), kdb_graph_part_first(wpn, parts, blockIdx.x + 1u), &s_n, p);
}

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_finish_kernel(unsigned long long *__restrict__ nodes, uint64_t wpl, uint32_t n_graph_nodes, uint32_t *__restrict__ n_nodes) {
    kdb_graph_finish_word(nodes + (uint64_t)blockIdx.y * wpl, wpl, n_graph_nodes, nullptr, n_nodes + blockIdx.y);
}

struct GateArgs {
    KdbView v;
    const KdbSubStaged *q;
    const unsigned char *guides;
    const float *qnorms;
    uint32_t guide_row, level, parts, n;
    unsigned long long *t, *p, *c;
    uint64_t wpn;
    hipStream_t s;
};
template <int PREC, int METRIC, int NCH>
void launch_gate(const GateArgs &a) {
    hipLaunchKernelGGL((subgraph_gate_kernel<PREC, METRIC, NCH>), dim3(a.parts, a.n), dim3(KDB_GRAPH_BLOCK), a.guide_row, a.s, a.v, a.q, a.guides, a.qnorms,
                       a.guide_row, a.level, a.parts, a.t, a.p, a.c, a.wpn);
}
// float32 rows take compute_dists' trip shape for their width where the gate has one (65 .. 128 columns: four rows per group; 768:
// three), every other width and the 16- and 8-bit rows the any-width loaders (two rows per group)
template <int METRIC>
void launch_gate_f32(const GateArgs &a) {
    if (a.v.ld > 64u && a.v.ld <= 128u) launch_gate<KDB_PREC_F32, METRIC, 2>(a);
    else if (a.v.ld == 768u) launch_gate<KDB_PREC_F32, METRIC, 12>(a);
    else launch_gate<KDB_PREC_F32, METRIC, 0>(a);
}

} // namespace

int kdb_launch_subgraph(kdb_index *idx, const kdb_subgraph_query *queries, uint32_t B, const float *d_guides, uint64_t *d_nodes, uint64_t words_per_list,
                        uint32_t *d_n_nodes, uint32_t *d_n_edges, kdb_subgraph_edge *d_edges, uint32_t edge_cap, hipStream_t s) {
    const KdbRelDev &g = idx->relations.dev;
    const KdbView v = kdb_make_view(idx);
    const uint64_t wpn = kdb_graph_wpn(g.n_nodes), wpl = words_per_list;
    std::vector<KdbSubStaged> staged(B);
    for (uint32_t b = 0; b < B; b++) staged[b] = kdb_subgraph_stage_query(queries[b]);
    const bool gated = d_guides && kdb_subgraph_any_guided(staged.data(), B);
    const uint64_t guide_row = !gated ? 0u : v.precision == KDB_PREC_I8 ? (uint64_t)v.ld : (uint64_t)v.ld * 4u;
    // (kdb_index_create admits float16 with L2 and int8 with cosine only, hnsw_index.go:203-229: every index has a gate instantiation)
    if (guide_row > KDB_SUBGRAPH_GUIDE_MAX) { // (before anything is queued: the gate could not be launched)
        kdb_set_error("subgraph_extract: a prepared guide of %llu bytes does not fit the gate's LDS (at most %llu)", (unsigned long long)guide_row,
                      (unsigned long long)KDB_SUBGRAPH_GUIDE_MAX);
        return KDB_ERR_UNSUPPORTED;
    }
    const uint32_t Bc = kdb_subgraph_chunk_queries(B, wpn, (uint64_t)kdb_graph_env("KDB_GRAPH_SCRATCH_MAX", (long long)KDB_GRAPH_SCRATCH_MAX));
    const int32_t forced = (int32_t)std::min<long long>(kdb_graph_env("KDB_GRAPH_PARTS", 0), KDB_GRAPH_MAX_PARTS);
    const KdbSubScratch L = kdb_subgraph_scratch(B, Bc, wpn, guide_row);
    int rc = kdb_ensure_scratch(idx, (size_t)L.total);
    if (rc) return rc;
    unsigned char *const d = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch);
    const KdbSubStaged *const d_q = reinterpret_cast<const KdbSubStaged *>(d + L.o_queries);
    float *const d_qnorm = reinterpret_cast<float *>(d + L.o_qnorm);
    auto bitmap = [&](uint64_t o) { return reinterpret_cast<unsigned long long *>(d + o); };
    unsigned long long *const f0 = bitmap(L.o_f0), *const f1 = bitmap(L.o_f1), *const bt = bitmap(L.o_t), *const bp = bitmap(L.o_p), *const bc = bitmap(L.o_c);
    // (pageable memory: consumed before hipMemcpyAsync returns, like the queries of kdb_launch_graph_filter)
    KDB_HIP(hipMemcpyAsync(d + L.o_queries, staged.data(), (size_t)B * sizeof(KdbSubStaged), hipMemcpyHostToDevice, s));
    // the guides as ComputeDistanceToVector prepares them (hnsw_index.go:3397-3423): the walk's preparation, told to normalise for
    // float32 rows only -- an int8 guide is quantised as it comes
    // -- run by run of guided queries: rows of unguided ones are not read
    for (uint32_t b0 = 0, b1 = 0; gated && kdb_subgraph_guided_run(queries, B, b1, &b0, &b1);)
        if ((rc = kdb_launch_prep_queries(v, d_guides + (size_t)b0 * v.dim, b1 - b0, d + L.o_guides + (size_t)b0 * guide_row, d_qnorm + b0,
                                          v.precision == KDB_PREC_F32 ? 1 : 0, s)) != KDB_OK)
            return rc;
    const unsigned word_blocks = (unsigned)((wpl + KDB_GRAPH_BLOCK - 1u) / KDB_GRAPH_BLOCK);
    for (uint32_t c0 = 0; c0 < B; c0 += Bc) { // chunks of queries, one behind the other on the stream: they share the bitmaps
        const uint32_t n = std::min(Bc, B - c0);
        unsigned long long *const nodes = reinterpret_cast<unsigned long long *>(d_nodes) + (uint64_t)c0 * wpl;
        kdb_subgraph_edge *const edges = d_edges && edge_cap ? d_edges + (uint64_t)c0 * edge_cap : nullptr;
        hipLaunchKernelGGL(subgraph_init_kernel, dim3(word_blocks, n), dim3(KDB_GRAPH_BLOCK), 0, s, d_q + c0, nodes, wpl, f0, f1, bt, bp, bc, wpn, d_n_nodes + c0,
                           d_n_edges + c0);
        const uint32_t levels = kdb_subgraph_levels(staged.data() + c0, n), parts = kdb_graph_parts(wpn, n, (uint32_t)idx->n_cu, forced);
        const bool chunk_gated = gated && kdb_subgraph_any_guided(staged.data() + c0, n);
        for (uint32_t level = 0; level < levels; level++) {
            unsigned long long *const fc = level & 1u ? f1 : f0, *const fn = level & 1u ? f0 : f1;
            if (chunk_gated) {
                hipLaunchKernelGGL(subgraph_level_kernel<SUB_COLLECT>, dim3(parts, n), dim3(KDB_GRAPH_BLOCK), 0, s, g, d_q + c0, level, parts, nodes, wpl, fc, fn,
                                   bt, bp, bc, wpn, d_n_edges + c0, edges, edge_cap);
                const GateArgs a{v, d_q + c0, d + L.o_guides + (size_t)c0 * guide_row, d_qnorm + c0, (uint32_t)guide_row, level, parts, n, bt, bp, bc, wpn, s};
                if (v.precision == KDB_PREC_F16) launch_gate<KDB_PREC_F16, KDB_METRIC_L2, 0>(a);
                else if (v.precision == KDB_PREC_I8) launch_gate<KDB_PREC_I8, KDB_METRIC_COSINE, 0>(a);
                else if (v.metric == KDB_METRIC_L2) launch_gate_f32<KDB_METRIC_L2>(a);
                else launch_gate_f32<KDB_METRIC_COSINE>(a);
            }
            hipLaunchKernelGGL(subgraph_level_kernel<SUB_EXPAND>, dim3(parts, n), dim3(KDB_GRAPH_BLOCK), 0, s, g, d_q + c0, level, parts, nodes, wpl, fc, fn, bt,
                               bp, bc, wpn, d_n_edges + c0, edges, edge_cap);
        }
        hipLaunchKernelGGL(subgraph_finish_kernel, dim3(word_blocks, n), dim3(KDB_GRAPH_BLOCK), 0, s, nodes, wpl, g.n_nodes, d_n_nodes + c0);
    }
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}
