// kdb_graph_sweep.cuh -- the one bitmap sweep behind the relation-BFS kernels: graph_filter.hip's level kernel and subgraph.hip's
// level and gate kernels.  A workgroup of four waves reads a slice of a bitmap (a frontier, the gate's candidates) one word per lane,
// hands the nodes of its non-zero words to a queue in LDS and meets between rounds to work the queue off with all 256 lanes.
#pragma once
#include "kdb_device.cuh" // kdb_lane, kdb_mbcnt
#include "kdb_graph_plan.h"

// Word w of a bitmap that starts as the root alone (root 0: nothing; root <= n_nodes, so its word is below wpn <= wpl).
__device__ __forceinline__ unsigned long long kdb_graph_seed_word(uint32_t root, uint64_t w) {
    return root && w == (uint64_t)(root >> 6) ? 1ull << (root & 63u) : 0ull;
}

// One lane per word of a finished list: bit 0 and the bits above `count` cleared, the and-list (null: none), the cardinality
// (null: not wanted) by one atomicAdd per wave.
__device__ __forceinline__ void kdb_graph_finish_word(unsigned long long *__restrict__ list, uint64_t wpl, uint32_t count,
                                                      const unsigned long long *__restrict__ and_list, uint32_t *__restrict__ card) {
    const uint64_t w = (uint64_t)blockIdx.x * KDB_GRAPH_BLOCK + threadIdx.x;
    unsigned long long v = 0ull;
    if (w < wpl) {
        v = list[w] & kdb_graph_live_mask(w, count);
        if (and_list) v &= and_list[w];
        list[w] = v;
    }
    uint32_t n = (uint32_t)__popcll(v);
#pragma unroll
    for (int o = (int)KDB_GRAPH_WAVE / 2; o >= 1; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, (int)KDB_GRAPH_WAVE);
    if (card && kdb_lane() == 0 && n) atomicAdd(card, n);
}

// n places of a queue of `cap` for the calling wave (n wave-uniform): the first of them, or `cap` when they do not fit -- the
// compare-and-swap either takes the places or leaves the count alone, so a wave that finds no room has changed nothing.
__device__ __forceinline__ uint32_t kdb_sweep_reserve(uint32_t &s_n, uint32_t n, uint32_t cap) {
    uint32_t slot = cap;
    if (kdb_lane() == 0) {
        uint32_t seen = *(volatile uint32_t *)&s_n;
        while (seen + n <= cap) {
            const uint32_t was = atomicCAS(&s_n, seen, seen + n);
            if (was == seen) {
                slot = seen;
                break;
            }
            seen = was;
        }
    }
    return (uint32_t)__shfl((int)slot, 0, (int)KDB_GRAPH_WAVE);
}

// Words [lo, hi) of a bitmap, by the whole workgroup (KDB_GRAPH_BLOCK lanes; s_n: the queue's count in LDS).
//   sweep   the four waves take the slice in groups of 64 consecutive words, wave w the groups w, w + 4, ...: one word per lane,
//           coalesced, through p.load(w), which also does what reading a word entails (write zero over it, OR it elsewhere).  The
//           ballot of the non-zero words is walked bit by bit: p.take(64-bit word index, its bits) turns the nodes of one word
//           into visits and queue records, with ONE kdb_sweep_reserve per wave and step, and returns false when that found no
//           room.  The wave then stops where it is: group, word and pending are wave-uniform registers here, and whatever part
//           of the word take has behind it (KdbCsrSweep: the direction) is a wave-uniform member of the policy, so that the same
//           take goes on where it stopped.
//   drain   every wave meets between the two barriers and p.drain(count), called by all 256 lanes, works the queue off.
// PROGRESS.  The queue is empty after a drain, and an empty queue takes any one word: the heavy nodes of a word in both directions
// (static_assert KDB_GRAPH_HUB_CAP >= 2 * KDB_GRAPH_WAVE, kdb_graph_plan.h), the nodes of a candidate word (static_assert
// KDB_SUBGRAPH_GATE_BATCH >= KDB_GRAPH_WAVE, kdb_subgraph_plan.h).  A reservation fails only against a queue that holds records, so
// a round in which a wave stops is a round in which some reservation was served, and a served step is not taken again: take goes
// on behind it.  The steps of a slice are finite, so the rounds end, when every wave has finished its groups.
// BARRIERS.  Every lane of the workgroup runs every barrier of every round: what leaves the inner loop (done, take's verdict) is
// wave-uniform, nothing between the barriers returns, and the only exit is the verdict of the barrier that ORs !done over the
// workgroup, which is common to all 256 lanes.  That barrier also says that every lane has read the queue, so lane 0 may empty it for the next round.
template <class Policy>
__device__ __forceinline__ void kdb_sweep_rounds(uint64_t lo, uint64_t hi, uint32_t *s_n, Policy &p) {
    const uint32_t tid = threadIdx.x, lane = tid & (KDB_GRAPH_WAVE - 1u), wave = tid / KDB_GRAPH_WAVE;
    uint64_t next = lo + (uint64_t)wave * KDB_GRAPH_WAVE; // the wave's next group
    uint64_t group = 0;                                   // first word of the group in hand
    unsigned long long word = 0ull;                       // the lane's word of it
    unsigned long long pending = 0ull;                    // its non-zero words not yet taken (wave-uniform)
    bool done = false;                                    // (wave-uniform)
    if (tid == 0u) *s_n = 0u;
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
                word = w < hi ? p.load(w) : 0ull;
                pending = __ballot(word != 0ull);
                continue;
            }
            const uint32_t j = (uint32_t)__ffsll((long long)pending) - 1u;
            if (!p.take(group + j, __shfl(word, (int)j, (int)KDB_GRAPH_WAVE))) break; // no room: the drain first, then this word again
            pending &= pending - 1ull;
        }
        __syncthreads(); // the queue's records are visible
        p.drain(*s_n);
        if (!__syncthreads_or(!done)) break;
        if (tid == 0u) *s_n = 0u;
        __syncthreads();
    }
}

// The hub queue of a level kernel in LDS: edge ranges as (begin | direction << 63, end) and the node they belong to.
struct KdbHubQueue {
    unsigned long long begin[KDB_GRAPH_HUB_CAP], end[KDB_GRAPH_HUB_CAP];
    uint32_t src[KDB_GRAPH_HUB_CAP];
    uint32_t n;
};

// The policy of a level kernel: frontier F (ZERO: a non-zero word is written back as zero by the lane that read it) over the CSR g,
// the directions of `dirs` (bit 0: out-edges, bit 1: in-edges).  For word j lane i owns node 64 j + i and reads its two CSR offsets
// per direction.
//   light   a node of degree <= KDB_GRAPH_LIGHT_DEG is expanded by its lane
//   hubs    the heavier nodes of the word go to the hub queue; at the drain all 256 lanes go through the queued ranges with coalesced
//           reads of dst and rel, so a hub's million edges are spread over the workgroup
// Every CSR entry is one call visit(act, node, far, rel, dir).  dir: 0, node -> far; 1, far -> node.  far is a dst of the snapshot:
// 1 <= far <= n_nodes, checked at upload, so its word lies inside every bitmap; rel < 64 likewise.
// Visitor::converged (static constexpr bool) picks the form of the two loops.  true: ALL 64 lanes of the wave call visit together,
// act says whose entry is real -- the light loop runs as long as ANY lane has an entry, the drain in whole trips of 256 -- so the
// visitor may use wave-wide operations.  false: only the lanes that have an entry call it (act is true), each in a loop of its own;
// for a visitor that needs no company this measured 0.4 .. 0.8 % faster (profiles/graph_sweep_refactor.txt).
// Registers: the CSR arrays are picked by selects, not by indexing the by-value kernel argument: no scratch.
template <bool ZERO, class Visitor>
struct KdbCsrSweep {
    const KdbRelDev &g;
    unsigned long long *F;
    uint32_t dirs;
    KdbHubQueue &q;
    const Visitor &visit;
    uint32_t dir; // the direction the word in hand goes on with (wave-uniform); 0 between words

    __device__ __forceinline__ unsigned long long load(uint64_t w) const {
        const unsigned long long word = F[w];
        if (ZERO && word) F[w] = 0ull;
        return word;
    }
    __device__ __forceinline__ bool take(uint64_t j, unsigned long long fw) {
        const uint32_t lane = (uint32_t)kdb_lane();
        const uint64_t node = j * KDB_GRAPH_WAVE + lane;
        const bool mine = ((fw >> lane) & 1ull) && node >= 1u && node <= (uint64_t)g.n_nodes;
        for (; dir < 2u; dir++) {
            if (!((dirs >> dir) & 1u)) continue;
            const uint64_t *const off = dir ? g.off[1] : g.off[0];
            const uint32_t *const dst = dir ? g.dst[1] : g.dst[0];
            const uint8_t *const rel = dir ? g.rel[1] : g.rel[0];
            const uint64_t e0 = mine ? off[node] : 0ull, e1 = mine ? off[node + 1u] : 0ull;
            const bool heavy = e1 - e0 > (uint64_t)KDB_GRAPH_LIGHT_DEG;
            const unsigned long long hb = __ballot(heavy);
            if (hb) {
                const uint32_t slot = kdb_sweep_reserve(q.n, (uint32_t)__popcll(hb), KDB_GRAPH_HUB_CAP);
                if (slot == KDB_GRAPH_HUB_CAP) return false; // (dir stays: the directions before it are not visited twice)
                if (heavy) {
                    const uint32_t at = slot + kdb_mbcnt(hb);
                    q.begin[at] = e0 | ((unsigned long long)dir << 63);
                    q.end[at] = e1;
                    q.src[at] = (uint32_t)node;
                }
            }
            if constexpr (Visitor::converged) {
                for (uint64_t e = e0; __ballot(!heavy && e < e1) != 0ull; e++) {
                    const bool a = !heavy && e < e1;
                    visit(a, (uint32_t)node, a ? dst[e] : 0u, a ? (uint32_t)rel[e] : 0u, dir);
                }
            } else if (!heavy) {
                for (uint64_t e = e0; e < e1; e++) visit(true, (uint32_t)node, dst[e], (uint32_t)rel[e], dir);
            }
        }
        dir = 0;
        return true;
    }
    __device__ __forceinline__ void drain(uint32_t n_hubs) const {
        for (uint32_t i = 0; i < n_hubs; i++) {
            const unsigned long long rec = q.begin[i], e1 = q.end[i];
            const uint32_t src = q.src[i], in = (uint32_t)(rec >> 63);
            const uint32_t *const dst = in ? g.dst[1] : g.dst[0];
            const uint8_t *const rel = in ? g.rel[1] : g.rel[0];
            if constexpr (Visitor::converged) {
                for (uint64_t t0 = rec & ~(1ull << 63); t0 < e1; t0 += KDB_GRAPH_BLOCK) {
                    const uint64_t e = t0 + threadIdx.x;
                    const bool a = e < e1;
                    visit(a, src, a ? dst[e] : 0u, a ? (uint32_t)rel[e] : 0u, in);
                }
            } else {
                for (uint64_t e = (rec & ~(1ull << 63)) + threadIdx.x; e < e1; e += KDB_GRAPH_BLOCK) visit(true, src, dst[e], (uint32_t)rel[e], in);
            }
        }
    }
};

// One level of a BFS over g by workgroup blockIdx.x of `parts`: its slice of the frontier F (wpn words), every CSR entry to `visit`.
template <bool ZERO, class Visitor>
__device__ __forceinline__ void kdb_csr_sweep(const KdbRelDev &g, unsigned long long *F, uint64_t wpn, uint32_t parts, uint32_t dirs, KdbHubQueue &q,
                                              const Visitor &visit) {
    KdbCsrSweep<ZERO, Visitor> p{g, F, dirs, q, visit, 0u};
    kdb_sweep_rounds(kdb_graph_part_first(wpn, parts, blockIdx.x), kdb_graph_part_first(wpn, parts, blockIdx.x + 1u), &q.n, p);
}
