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
// Semantics, chunking, validation and the scratch layout are kdb_subgraph_plan.h's.  The sweep is graph_filter.hip's -- words
// coalesced, light nodes lane-privately, heavier ones through the hub queue in LDS -- restated here with what extraction adds:
// both directions always, the source of a hub (an edge record names it), and wave-converged visits, because EXPAND reserves edge
// slots with ONE atomic per wave and trip.  The result is a node SET and an edge MULTISET: V and P only ever gain bits, a node
// enters the next frontier exactly once, an edge record is written by the one lane that visits its CSR entry, so nothing depends
// on the order in which the atomics land.
#include "kdb_search_core.cuh" // kdb_trip_rows: the rows-per-trip table of compute_dists; kdb_device.cuh: the accumulate steps
#include "kdb_decode.cuh"      // kdb_row_found
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
    const uint32_t root = queries[b].root; // (<= n_nodes: its word is below wpn <= wpl)
    const unsigned long long seed = root && w == (uint64_t)(root >> 6) ? 1ull << (root & 63u) : 0ull;
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

// Workgroup (s, b): words [first(s), first(s + 1)) of the current frontier of query b.  graph_level_kernel's sweep (graph_filter.hip):
// the four waves take the slice in groups of 64 consecutive words, one word per lane; the ballot of the non-zero words is walked
// word by word, lane i owns node 64 j + i; a node of degree <= KDB_GRAPH_LIGHT_DEG (per direction) is expanded by its lane, in a loop
// that runs as long as ANY lane has an entry left so that the wave stays converged; heavier ones go to the hub queue in LDS as
// (begin | direction << 63, end, source) with one compare-and-swap reservation per wave and word.  A wave whose reservation does not
// fit stops where it is -- (group, pending words, direction) are wave-uniform registers -- and every wave meets at the drain, where
// all 256 lanes go through the queued ranges in whole trips of 256 entries.  Everything that decides a barrier is wave-uniform and
// the loop's exit is __syncthreads_or's common verdict.
template <int MODE>
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_level_kernel(const KdbRelDev g, const KdbSubStaged *__restrict__ queries, uint32_t level, uint32_t parts, unsigned long long *nodes, uint64_t wpl,
                      unsigned long long *f_cur, unsigned long long *f_next, unsigned long long *bt, unsigned long long *bp, unsigned long long *bc,
                      uint64_t wpn, uint32_t *n_edges, kdb_subgraph_edge *edges, uint32_t edge_cap) {
    __shared__ unsigned long long s_begin[KDB_GRAPH_HUB_CAP], s_end[KDB_GRAPH_HUB_CAP];
    __shared__ uint32_t s_src[KDB_GRAPH_HUB_CAP];
    __shared__ uint32_t s_n;
    const uint32_t b = blockIdx.y, tid = threadIdx.x, lane = tid & (KDB_GRAPH_WAVE - 1u), wave = tid / KDB_GRAPH_WAVE;
    const uint32_t depth = queries[b].depth;
    if (level >= depth || (MODE == SUB_COLLECT && !queries[b].guided)) return; // (the whole workgroup)
    SubCtx c;
    c.rel_mask = queries[b].rel_mask;
    c.V = nodes + (uint64_t)b * wpl, c.Fn = f_next + (uint64_t)b * wpn;
    c.T = bt + (uint64_t)b * wpn, c.P = bp + (uint64_t)b * wpn, c.C = bc + (uint64_t)b * wpn;
    c.n_edges = n_edges + b;
    c.edges = edges && edge_cap ? edges + (uint64_t)b * edge_cap : nullptr;
    c.edge_cap = edge_cap, c.level = level;
    c.guided = queries[b].guided != 0u, c.last = level + 1u >= depth;
    unsigned long long *const Fc = f_cur + (uint64_t)b * wpn;
    const uint64_t hi = kdb_graph_part_first(wpn, parts, blockIdx.x + 1u);
    uint64_t next = kdb_graph_part_first(wpn, parts, blockIdx.x) + (uint64_t)wave * KDB_GRAPH_WAVE; // the wave's next group
    uint64_t group = 0;                // first word of the group in hand
    unsigned long long word = 0ull;    // the lane's word of it
    unsigned long long pending = 0ull; // its non-zero words not yet expanded (wave-uniform)
    uint32_t dir = 0;                  // the direction the first pending word goes on with (wave-uniform)
    bool done = false;                 // (wave-uniform)
    if (tid == 0u) s_n = 0u;
    __syncthreads();
    for (;;) {
        while (!done) {
            if (!pending) {
                if (next >= hi) {
                    done = true;
                    break;
                }
                group = next;
                next += (uint64_t)KDB_GRAPH_BLOCK;
                const uint64_t w = group + lane;
                word = w < hi ? Fc[w] : 0ull;
                if (MODE == SUB_EXPAND && word) Fc[w] = 0ull;
                pending = __ballot(word != 0ull);
                dir = 0;
                continue;
            }
            const uint32_t j = (uint32_t)__ffsll((long long)pending) - 1u;
            const unsigned long long fw = __shfl(word, (int)j, (int)KDB_GRAPH_WAVE);
            const uint64_t node = (group + j) * KDB_GRAPH_WAVE + lane;
            const bool mine = ((fw >> lane) & 1ull) && node >= 1u && node <= (uint64_t)g.n_nodes;
            bool full = false;
            for (; dir < 2u; dir++) {
                const uint64_t *const off = dir ? g.off[1] : g.off[0];
                const uint32_t *const dst = dir ? g.dst[1] : g.dst[0];
                const uint8_t *const rel = dir ? g.rel[1] : g.rel[0];
                const uint64_t e0 = mine ? off[node] : 0ull, e1 = mine ? off[node + 1u] : 0ull;
                const bool heavy = e1 - e0 > (uint64_t)KDB_GRAPH_LIGHT_DEG;
                const unsigned long long hb = __ballot(heavy);
                if (hb) {
                    const uint32_t n = (uint32_t)__popcll(hb);
                    uint32_t slot = KDB_GRAPH_HUB_CAP;
                    if (lane == 0u) {
                        uint32_t seen = *(volatile uint32_t *)&s_n;
                        while (seen + n <= KDB_GRAPH_HUB_CAP) {
                            const uint32_t was = atomicCAS(&s_n, seen, seen + n);
                            if (was == seen) {
                                slot = seen;
                                break;
                            }
                            seen = was;
                        }
                    }
                    slot = (uint32_t)__shfl((int)slot, 0, (int)KDB_GRAPH_WAVE);
                    if (slot == KDB_GRAPH_HUB_CAP) { // no room: the drain first, then this word and direction again
                        full = true;
                        break;
                    }
                    if (heavy) {
                        const uint32_t at = slot + (uint32_t)__popcll(hb & ((1ull << lane) - 1ull));
                        s_begin[at] = e0 | ((unsigned long long)dir << 63);
                        s_end[at] = e1;
                        s_src[at] = (uint32_t)node;
                    }
                }
                for (uint64_t e = e0; __ballot(!heavy && e < e1) != 0ull; e++) { // (every lane goes round while any lane has an entry)
                    const bool a = !heavy && e < e1;
                    sub_visit<MODE>(c, a, (uint32_t)node, a ? dst[e] : 0u, a ? (uint32_t)rel[e] : 0u, dir);
                }
            }
            if (full) break;
            pending &= pending - 1ull;
            dir = 0;
        }
        __syncthreads(); // the queue's records are visible
        const uint32_t n_hubs = s_n;
        for (uint32_t i = 0; i < n_hubs; i++) {
            const unsigned long long rec = s_begin[i], e1 = s_end[i];
            const uint32_t src = s_src[i], in = (uint32_t)(rec >> 63);
            const uint32_t *const dst = in ? g.dst[1] : g.dst[0];
            const uint8_t *const rel = in ? g.rel[1] : g.rel[0];
            for (uint64_t t0 = rec & ~(1ull << 63); t0 < e1; t0 += KDB_GRAPH_BLOCK) { // whole trips: the waves stay converged
                const uint64_t e = t0 + tid;
                const bool a = e < e1;
                sub_visit<MODE>(c, a, src, a ? dst[e] : 0u, a ? (uint32_t)rel[e] : 0u, in);
            }
        }
        if (!__syncthreads_or(!done)) break; // (also: every lane has read the queue)
        if (tid == 0u) s_n = 0u;
        __syncthreads();
    }
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

// Workgroup (s, b): words [first(s), first(s + 1)) of the candidate bitmap C of query b, level `level`.
//   guide   the prepared guide of the query, once per workgroup, in LDS (ld floats, or ld packed int8 values)
//   sweep   as the level kernel sweeps a frontier: one word per lane; the lane that reads a non-zero word ORs it into T and writes
//           zero over it (only this workgroup touches these words of T and C in this launch).  The non-zero words are walked one by
//           one: the wave reserves popcount(word) places of the batch with one compare-and-swap and lane i writes node 64 j + i
//           behind the set bits below it.  A wave whose word does not fit stops where it is and every wave meets at the drain
//   drain   wave w takes trips w, w + 4, ... of the batch, 4 * R rows each (gate_trip): with R rows of every 16-lane group in
//           flight, a CU holds 16 * R row gathers per resident workgroup.  The batch is empty after a drain and takes any one word
// A gather bound by HBM latency: no matrix instruction fits, every query has its own single guide.
template <int PREC, int METRIC, int NCH>
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_gate_kernel(const KdbView v, const KdbSubStaged *__restrict__ queries, const unsigned char *__restrict__ guides, const float *__restrict__ qnorms,
                     uint32_t guide_row, uint32_t level, uint32_t parts, unsigned long long *bt, unsigned long long *bp, unsigned long long *bc, uint64_t wpn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_guide[];
    __shared__ uint32_t s_batch[KDB_SUBGRAPH_GATE_BATCH];
    __shared__ uint32_t s_n;
    const uint32_t b = blockIdx.y, tid = threadIdx.x, lane = tid & (KDB_GRAPH_WAVE - 1u), wave = tid / KDB_GRAPH_WAVE;
    if (level >= queries[b].depth || !queries[b].guided) return; // (the whole workgroup)
    constexpr uint32_t TRIP = 4u * (uint32_t)kdbcore::kdb_trip_rows<PREC, NCH, 0>();
    const double threshold = queries[b].threshold;
    const float qnorm = qnorms[b];
    unsigned long long *const T = bt + (uint64_t)b * wpn, *const P = bp + (uint64_t)b * wpn, *const Cb = bc + (uint64_t)b * wpn;
    {
        const uint4 *const src = reinterpret_cast<const uint4 *>(guides + (size_t)b * guide_row); // (rows of 16-byte pieces on 256-byte regions)
        for (uint32_t i = tid; i < (guide_row >> 4); i += KDB_GRAPH_BLOCK) reinterpret_cast<uint4 *>(s_guide)[i] = src[i];
    }
    const uint64_t hi = kdb_graph_part_first(wpn, parts, blockIdx.x + 1u);
    uint64_t next = kdb_graph_part_first(wpn, parts, blockIdx.x) + (uint64_t)wave * KDB_GRAPH_WAVE;
    uint64_t group = 0;
    unsigned long long word = 0ull, pending = 0ull; // (pending: wave-uniform)
    bool done = false;                              // (wave-uniform)
    if (tid == 0u) s_n = 0u;
    __syncthreads();
    for (;;) {
        while (!done) {
            if (!pending) {
                if (next >= hi) {
                    done = true;
                    break;
                }
                group = next;
                next += (uint64_t)KDB_GRAPH_BLOCK;
                const uint64_t w = group + lane;
                word = w < hi ? Cb[w] : 0ull;
                if (word) {
                    T[w] |= word;
                    Cb[w] = 0ull;
                }
                pending = __ballot(word != 0ull);
                continue;
            }
            const uint32_t j = (uint32_t)__ffsll((long long)pending) - 1u;
            const unsigned long long cw = __shfl(word, (int)j, (int)KDB_GRAPH_WAVE);
            const uint32_t n = (uint32_t)__popcll(cw);
            uint32_t slot = KDB_SUBGRAPH_GATE_BATCH;
            if (lane == 0u) {
                uint32_t seen = *(volatile uint32_t *)&s_n;
                while (seen + n <= KDB_SUBGRAPH_GATE_BATCH) {
                    const uint32_t was = atomicCAS(&s_n, seen, seen + n);
                    if (was == seen) {
                        slot = seen;
                        break;
                    }
                    seen = was;
                }
            }
            slot = (uint32_t)__shfl((int)slot, 0, (int)KDB_GRAPH_WAVE);
            if (slot == KDB_SUBGRAPH_GATE_BATCH) break; // no room: the drain first, then this word again
            if ((cw >> lane) & 1ull) s_batch[slot + (uint32_t)__popcll(cw & ((1ull << lane) - 1ull))] = (uint32_t)((group + j) * KDB_GRAPH_WAVE + lane);
            pending &= pending - 1ull;
        }
        __syncthreads(); // the batch is visible
        const uint32_t nb = s_n;
        for (uint32_t base = wave * TRIP; base < nb; base += 4u * TRIP)
            gate_trip<PREC, METRIC, NCH>(v, reinterpret_cast<const float *>(s_guide), qnorm, threshold, s_batch, base, nb, P);
        if (!__syncthreads_or(!done)) break; // (also: every wave has read the batch)
        if (tid == 0u) s_n = 0u;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
subgraph_finish_kernel(unsigned long long *__restrict__ nodes, uint64_t wpl, uint32_t n_graph_nodes, uint32_t *__restrict__ n_nodes) {
    const uint32_t b = blockIdx.y;
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    unsigned long long v = 0ull;
    if (w < wpl) {
        v = nodes[(uint64_t)b * wpl + w] & kdb_graph_live_mask(w, n_graph_nodes);
        nodes[(uint64_t)b * wpl + w] = v;
    }
    uint32_t n = (uint32_t)__popcll(v);
#pragma unroll
    for (int o = (int)KDB_GRAPH_WAVE / 2; o >= 1; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, (int)KDB_GRAPH_WAVE);
    if ((threadIdx.x & (KDB_GRAPH_WAVE - 1u)) == 0u && n) atomicAdd(n_nodes + b, n);
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
