// graph_filter.hip -- graph filters on the device: the allow list that resolveGraphFilter (pkg/engine/graph.go:173-246) builds on the
// host with a FIFO queue, Go maps and string ids, written by a level-synchronous BFS on bitmaps over the relation CSR in HBM, in the
// dense layout every filtered entry point takes.
//
//   graph_init_kernel    every word of the lists and of both frontiers: zero, or the root's bit (lists and F0)
//   graph_level_kernel   (part, query) per workgroup: one BFS level -- sweep the frontier, expand, mark the newly seen
//   graph_finish_kernel  one lane per list word: bit 0 and the bits above count cleared, the and-list, the cardinality
//
// Semantics, geometry, chunking, validation and the scratch layout are kdb_graph_plan.h's; this file holds what needs the device.
// The result is a SET: V only ever gains bits, a node enters the next frontier exactly once (the lane whose atomicOr on V saw the
// bit clear), so nothing depends on the order in which the atomics land.
#include "kdb_internal.h"
#include "kdb_graph_plan.h"
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_init_kernel(const KdbGraphStaged *__restrict__ queries, unsigned long long *__restrict__ lists, uint64_t wpl, unsigned long long *__restrict__ f0,
                  unsigned long long *__restrict__ f1, uint64_t wpn, uint32_t *__restrict__ card) {
    const uint32_t b = blockIdx.y;
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    const uint32_t root = queries[b].root; // (<= n_nodes: its word is below wpn <= wpl)
    const unsigned long long seed = root && w == (uint64_t)(root >> 6) ? 1ull << (root & 63u) : 0ull;
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

// Workgroup (s, b): level `level` of query b over words [first(s), first(s + 1)) of its current frontier.
//   sweep   the four waves take the slice in groups of 64 consecutive words, wave w the groups w, w + 4, ...: one word per lane,
//           coalesced; a non-zero word is written back as zero by the lane that read it.  The ballot of the non-zero words is walked
//           bit by bit: for word j lane i owns node 64 j + i and reads its two CSR offsets per direction the query follows.
//   light   a node of degree <= KDB_GRAPH_LIGHT_DEG is expanded by its lane.
//   hubs    the heavier nodes of the word are appended to the workgroup's hub queue in LDS as (begin | direction << 63, end) with ONE
//           reservation per wave and word (compare-and-swap: it either takes the slots or leaves the count alone).  A wave whose
//           reservation does not fit stops where it is -- (group, pending words, direction) are wave-uniform registers -- and every
//           wave meets at the drain: all 256 lanes go through the queued edge ranges with coalesced reads of dst and rel, so a hub's
//           million edges are spread over the workgroup.  The queue is empty after a drain and takes any one word (static_assert in
//           the plan), so every round makes progress; the rounds end when every wave has finished its groups.
// Everything that decides a barrier is wave-uniform and the loop's exit is __syncthreads_or's common verdict.
// Registers: the CSR arrays are picked by selects, not by indexing the by-value argument: no scratch.
__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_level_kernel(const KdbRelDev g, const KdbGraphStaged *__restrict__ queries, uint32_t level, uint32_t parts, unsigned long long *lists, uint64_t wpl,
                   unsigned long long *f_cur, unsigned long long *f_next, uint64_t wpn) {
    __shared__ unsigned long long s_begin[KDB_GRAPH_HUB_CAP], s_end[KDB_GRAPH_HUB_CAP];
    __shared__ uint32_t s_n;
    const uint32_t b = blockIdx.y, tid = threadIdx.x, lane = tid & (KDB_GRAPH_WAVE - 1u), wave = tid / KDB_GRAPH_WAVE;
    const uint32_t depth = queries[b].depth, dirs = queries[b].dirs;
    if (level >= depth) return; // (the whole workgroup)
    const uint64_t rel_mask = queries[b].rel_mask;
    const bool last = level + 1u >= depth;
    unsigned long long *const V = lists + (uint64_t)b * wpl, *const Fc = f_cur + (uint64_t)b * wpn, *const Fn = f_next + (uint64_t)b * wpn;
    const uint64_t hi = kdb_graph_part_first(wpn, parts, blockIdx.x + 1u);
    uint64_t next = kdb_graph_part_first(wpn, parts, blockIdx.x) + (uint64_t)wave * KDB_GRAPH_WAVE; // the wave's next group
    uint64_t group = 0;               // first word of the group in hand
    unsigned long long word = 0ull;   // the lane's word of it
    unsigned long long pending = 0ull; // its non-zero words not yet expanded (wave-uniform)
    uint32_t dir = 0;                 // the direction the first pending word goes on with (wave-uniform)
    bool done = false;                // (wave-uniform)
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
                if (word) Fc[w] = 0ull;
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
                if (!((dirs >> dir) & 1u)) continue;
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
                    }
                }
                if (!heavy)
                    for (uint64_t e = e0; e < e1; e++) graph_visit(dst[e], rel[e], rel_mask, V, Fn, last);
            }
            if (full) break;
            pending &= pending - 1ull;
            dir = 0;
        }
        __syncthreads(); // the queue's records are visible
        const uint32_t n_hubs = s_n;
        for (uint32_t i = 0; i < n_hubs; i++) {
            const unsigned long long rec = s_begin[i], e1 = s_end[i];
            const bool in = (rec >> 63) != 0ull;
            const uint32_t *const dst = in ? g.dst[1] : g.dst[0];
            const uint8_t *const rel = in ? g.rel[1] : g.rel[0];
            for (uint64_t e = (rec & ~(1ull << 63)) + tid; e < e1; e += KDB_GRAPH_BLOCK) graph_visit(dst[e], rel[e], rel_mask, V, Fn, last);
        }
        if (!__syncthreads_or(!done)) break; // (also: every lane has read the queue)
        if (tid == 0u) s_n = 0u;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(KDB_GRAPH_BLOCK)
graph_finish_kernel(const KdbGraphStaged *__restrict__ queries, unsigned long long *__restrict__ lists, uint64_t wpl, uint32_t count,
                    const unsigned long long *__restrict__ and_lists, uint32_t *__restrict__ card) {
    const uint32_t b = blockIdx.y;
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    unsigned long long v = 0ull;
    if (w < wpl) {
        v = lists[(uint64_t)b * wpl + w] & kdb_graph_live_mask(w, count);
        const uint32_t a = queries[b].and_idx;
        if (and_lists && a != KDB_NO_FILTER) v &= and_lists[(uint64_t)a * wpl + w];
        lists[(uint64_t)b * wpl + w] = v;
    }
    uint32_t n = (uint32_t)__popcll(v);
#pragma unroll
    for (int o = (int)KDB_GRAPH_WAVE / 2; o >= 1; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, (int)KDB_GRAPH_WAVE);
    if (card && (threadIdx.x & (KDB_GRAPH_WAVE - 1u)) == 0u && n) atomicAdd(card + b, n);
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
