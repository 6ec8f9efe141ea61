// kdb_graph_build.cuh -- what the graph-construction family shares: build.hip (the fast builder, reference linking), refine.hip
// (Refine, Vacuum) and add.hip (the sequential Add).  Device side: the start of a walking wave, a stored row as a query, scoring
// ids against it, the (key, id) sort, selectNeighbors on a workgroup.  Host side: workspace, upper pool, dispatch, walk launch.
#pragma once
#include "kdb_search_core.cuh"
#include "kdb_stage.h"
#include "kdb_walk_lds.h"
#include <type_traits>

using namespace kdbcore;

namespace {

static_assert(KDB_WALK_MARKS == KDB_UP_MARK_CAP, "the walk plan sizes the un-mark list the layer search fills");
constexpr bool walk_bs_agrees(uint32_t efc) { return kdb_walk_bs(efc) == (kdb_beam_slots(efc) == 1 ? 2u : (uint32_t)kdb_beam_slots(efc)); }
static_assert(walk_bs_agrees(1) && walk_bs_agrees(64) && walk_bs_agrees(65) && walk_bs_agrees(128) && walk_bs_agrees(129) && walk_bs_agrees(256) &&
                  walk_bs_agrees(257) && walk_bs_agrees(512),
              "the walk plan's beam storage is kdb_beam_slots' (one slot promoted to two)");

constexpr int PR_KC = 128;            // K-chunk (floats) staged per step
constexpr int PR_STRIDE = PR_KC + 4;  // LDS row stride: 33 sixteen-byte slots -> conflict-free b128 reads
constexpr int PR_BLK = 32;            // candidates resolved per step
constexpr int PR_U = 10;              // pair slots per thread: 32*63 + 496 pairs <= 10*256
constexpr int PR_MAXSEL = 64;         // maxM <= 64
constexpr int PR_MAXC = 576;          // max candidates per prune task (efC <= 512, 64 existing + requests)
constexpr uint32_t KDB_MAX_EFC = 512;  // BENCHMARKS.md:84 publishes M=32, efConstruction=400

template <int PREC> struct BKey { using T = float; };
template <> struct BKey<KDB_PREC_I8> { using T = double; }; // the reference's float64 cosine distance

// ---- small idioms ---------------------------------------------------------------------------------
__device__ __forceinline__ bool is_deleted(const KdbView &v, uint32_t id) { return (v.deleted[id >> 5] >> (id & 31u)) & 1u; }

// stored length of a list: packed from the front, the first zero word ends it
__device__ __forceinline__ uint32_t list_len(const uint32_t *adj, uint32_t maxm) {
    uint32_t ne = 0;
    while (ne < maxm && adj[ne] != 0u) ne++;
    return ne;
}

// the list of (node, level) in a level-0 array / upper pool pair: the adjacency itself, or the keys stored beside it
template <typename T>
__device__ __forceinline__ T *adj_of(T *a0, T *a_up, const KdbView &v, uint32_t node, uint32_t level) {
    return level == 0 ? a0 + (size_t)node * v.deg0 : a_up + ((size_t)v.up_idx[node] + (level - 1u)) * v.deg_up;
}

// a node's stored row becomes a query in LDS, loaded by T threads (a wave: 64, a workgroup: 256); returns the norm the int8
// distance takes with it, as distFn takes it (:2411-2418: 0 -> 1 -- a zero norm on either side is distance 1 either way: the dot
// with a zero row is 0, and 1 - 0 / (1 * n) = 1)
template <int PREC, uint32_t T>
__device__ __forceinline__ float load_row_as_query(const KdbView &v, float *q, uint32_t node, uint32_t t) {
    float qnorm = 1.f;
    if constexpr (PREC == KDB_PREC_I8) { // the packed row itself (ld is a multiple of 16)
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const int8_t *>(v.rows) + (size_t)node * v.ld);
        for (uint32_t i = t; i < (v.ld >> 4); i += T) reinterpret_cast<uint4 *>(q)[i] = src[i];
        qnorm = v.norms[node];
        if (qnorm == 0.f) qnorm = 1.f;
    } else if constexpr (PREC == KDB_PREC_F16) { // widened (exactly) to the f32 query the search keeps in LDS
        const uint16_t *src = reinterpret_cast<const uint16_t *>(v.rows) + (size_t)node * v.ld;
        for (uint32_t i = t; i < v.ld; i += T) q[i] = (float)__builtin_bit_cast(_Float16, src[i]);
    } else {
        const float4 *src = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(v.rows) + (size_t)node * v.ld);
        for (uint32_t i = t; i < (v.ld >> 2); i += T) reinterpret_cast<float4 *>(q)[i] = src[i];
    }
    return qnorm;
}

// ---- a walking wave (build_search_kernel, refine_search_kernel, add_link_kernel) --------------------
template <int BS, bool I8>
using WalkBeam = typename std::conditional<BS == 0, LdsBeamT<I8>, RegBeam<(BS == 0 ? 1 : BS), I8>>::type;

// once per wave: its LDS cut as the plan says (kdb_walk_lds.h; the host sized the launch from the same plan and passes its two
// capacities), its visited bitset.  Soft-deleted nodes are traversed, never returned (:2583-2590): they wait in the side list
// nr_*, exactly as in the query path
template <int BS, bool I8>
__device__ __forceinline__ void walk_carve(unsigned char *smem, const KdbView &v, uint32_t beam_cap, uint32_t nr_cap, uint32_t *vis_bits, WaveLds &s,
                                           VisBitset &vis) {
    const KdbWalkLds wl = kdb_walk_lds_cut(I8, v.ld, BS, beam_cap, nr_cap);
    s.q = reinterpret_cast<float *>(smem + wl.q);
    s.beam_d = BS == 0 ? reinterpret_cast<float *>(smem + wl.beam_d) : nullptr;
    s.beam_id = BS == 0 ? reinterpret_cast<uint32_t *>(smem + wl.beam_id) : nullptr;
    s.beam_lo = BS == 0 && I8 ? reinterpret_cast<uint32_t *>(smem + wl.beam_lo) : nullptr;
    s.beam_cap = BS == 0 ? wl.beam_cap : 0;
    s.nr_d = reinterpret_cast<float *>(smem + wl.nr_d);
    s.nr_id = reinterpret_cast<uint32_t *>(smem + wl.nr_id);
    s.nr_lo = I8 ? reinterpret_cast<uint32_t *>(smem + wl.nr_lo) : nullptr;
    s.nr_cap = wl.nr_cap;
    s.ctl = nullptr;
    s.nb_id = reinterpret_cast<uint32_t *>(smem + wl.nb_id);
    s.nb_d = reinterpret_cast<float *>(smem + wl.nb_d);
    s.nb_lo = I8 ? reinterpret_cast<uint32_t *>(smem + wl.nb_lo) : nullptr;
    s.ins_d = s.nb_d;
    s.ins_id = s.nb_id;
    s.marks = reinterpret_cast<uint32_t *>(smem + wl.marks);
    vis.bits = vis_bits;
    vis.words = v.vis_words;
    vis.marks = s.marks;
}

// once per node: a clean visited set (fresh), the node's own row as the query, an empty beam; returns the query's norm
template <int PREC, typename Beam>
__device__ __forceinline__ float walk_start(const KdbView &v, const WaveLds &s, VisBitset &vis, Beam &b, uint32_t node, int lane, bool fresh = true) {
    if (fresh) vis.begin_query();
    const float qnorm = load_row_as_query<PREC, 64>(v, s.q, node, (uint32_t)lane);
    __threadfence_block();
    wave_lds_fence();
    b.bind(s);
    b.tied = 0u;
    return qnorm;
}

// the next level's entry point is this level's nearest candidate (:786-788 / :1849): its distance is known
template <typename Beam>
__device__ __forceinline__ void walk_nearest(Beam &b, uint32_t &ep, EpKnown &epk) {
    if (b.count > 0) {
        float d0;
        uint32_t l0, f0;
        b.get(0, d0, l0, f0);
        ep = f0 & KDB_ID_MASK;
        epk.known = true;
        epk.key = d0;
        epk.lo = l0;
    } else {
        epk.known = false; // (the entry point stays: its distance at this level was computed, but keep it simple)
    }
}

// ---- a workgroup scores ids against a stored row ----------------------------------------------------
// where the scratch of that lives (kdb_score_tail: behind the prune tiles of most kernels)
struct ScoreLds {
    float *w_d;     // [4][64] distances of a wave's chunk
    uint32_t *w_lo; // [4][64] int8: their low words
    float *tq;      // the row as the query
};
template <bool I8>
__device__ __forceinline__ ScoreLds score_carve(unsigned char *at, const KdbView &v) {
    const KdbScoreTail t = kdb_score_tail(I8, v.ld);
    return ScoreLds{reinterpret_cast<float *>(at + t.w_d), reinterpret_cast<uint32_t *>(at + t.w_lo), reinterpret_cast<float *>(at + t.tq)};
}

// distanceBetweenNodes(row in sl.tq, ids[i]) (:297-340) -> keys[i], i < n: 16 lanes per row, a wave per chunk of 64.  Whole
// workgroup (256 threads); the row is in place (load_row_as_query + __syncthreads), the caller synchronises behind it
template <int METRIC, int PREC>
__device__ __forceinline__ void score_ids_wg(const KdbView &v, const ScoreLds &sl, float qnorm, uint32_t *ids, uint32_t n, typename BKey<PREC>::T *keys) {
    constexpr bool I8 = PREC == KDB_PREC_I8;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    WaveLds s{};
    s.q = sl.tq;
    s.nb_d = sl.w_d + wave * 64u;
    s.nb_lo = I8 ? sl.w_lo + wave * 64u : nullptr;
    for (uint32_t c0 = wave * 64u; c0 < n; c0 += 256u) {
        const uint32_t cn = n - c0 < 64u ? n - c0 : 64u;
        s.nb_id = ids + c0;
        compute_dists<PREC, METRIC, 0>(v, s, cn, qnorm);
        if (lane < cn) {
            if constexpr (I8) keys[c0 + lane] = kdb_i8_key_double(s.nb_d[lane], s.nb_lo[lane]);
            else keys[c0 + lane] = s.nb_d[lane];
        }
        wave_lds_fence();
    }
}

// key/id[0..n) ascending by (key, id), padded to a power of two P >= 64 the arrays must hold: bitonic, whole workgroup
template <typename KT>
__device__ __forceinline__ void sort_by_key_id_wg(KT *key, uint32_t *id, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    uint32_t P = 64;
    while (P < n) P <<= 1;
    for (uint32_t i = n + tid; i < P; i += 256) {
        key[i] = (KT)INFINITY;
        id[i] = 0xffffffffu;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += 256) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0u;
                    const KT kx = key[i], ky = key[l];
                    const uint32_t ix = id[i], iy = id[l];
                    const bool gt = kx > ky || (kx == ky && ix > iy);
                    if (gt == up) {
                        key[i] = ky;
                        key[l] = kx;
                        id[i] = iy;
                        id[l] = ix;
                    }
                }
            }
            __syncthreads();
        }
}

// ---- selectNeighbors on a workgroup ---------------------------------------------------------------
template <typename KT>
struct PruneLdsT {
    uint32_t *c_id;    // [PR_MAXC] candidates IN THE ORDER selectNeighbors takes them: ascending by (key,id) from a walk or a sort,
                       // the stored order of a list (+ the new node last) from the reverse prune of Add (add_reverse_kernel)
    KT *c_key;         // [PR_MAXC]
    uint32_t *s_id;    // [PR_MAXSEL]
    KT *s_key;         // [PR_MAXSEL]
    uint16_t *disc;    // [PR_MAXC] discarded candidate indices, in order
    float *rows;       // [(PR_BLK + PR_MAXSEL) * PR_STRIDE] 4-byte words: f32 values, or four packed int8
    KT *m1;            // [PR_BLK][PR_MAXSEL]
    KT *m2;            // [PR_BLK][PR_BLK]
    uint32_t *misc;    // [8]: 0 n_sel, 1 n_disc
};

template <typename KT>
__host__ __device__ constexpr size_t prune_lds_bytes() {
    return (size_t)(PR_BLK + PR_MAXSEL) * PR_STRIDE * 4 + (size_t)PR_BLK * PR_MAXSEL * sizeof(KT) + (size_t)PR_BLK * PR_BLK * sizeof(KT) +
           (size_t)PR_MAXC * sizeof(KT) + PR_MAXSEL * sizeof(KT) + (size_t)PR_MAXC * 4 + PR_MAXSEL * 4 + 32 + (size_t)PR_MAXC * 2 + 32;
}

template <typename KT>
__device__ __forceinline__ void prune_carve(unsigned char *smem, PruneLdsT<KT> &p) {
    size_t off = 0;
    p.rows = reinterpret_cast<float *>(smem + off);
    off += (size_t)(PR_BLK + PR_MAXSEL) * PR_STRIDE * 4;
    p.m1 = reinterpret_cast<KT *>(smem + off); // (8-byte keys first: the tile is a multiple of 16 bytes)
    off += (size_t)PR_BLK * PR_MAXSEL * sizeof(KT);
    p.m2 = reinterpret_cast<KT *>(smem + off);
    off += (size_t)PR_BLK * PR_BLK * sizeof(KT);
    p.c_key = reinterpret_cast<KT *>(smem + off);
    off += (size_t)PR_MAXC * sizeof(KT);
    p.s_key = reinterpret_cast<KT *>(smem + off);
    off += PR_MAXSEL * sizeof(KT);
    p.c_id = reinterpret_cast<uint32_t *>(smem + off);
    off += (size_t)PR_MAXC * 4;
    p.s_id = reinterpret_cast<uint32_t *>(smem + off);
    off += PR_MAXSEL * 4;
    p.misc = reinterpret_cast<uint32_t *>(smem + off);
    off += 32;
    p.disc = reinterpret_cast<uint16_t *>(smem + off);
}

// int8 cosine distance between two stored rows (distanceBetweenNodes, hnsw_index.go:317-336): float64
__device__ __forceinline__ double i8_pair_distance(int dot, float n1, float n2) {
    if (n1 == 0.f || n2 == 0.f) return 1.0;
    double sim = (double)dot / ((double)n1 * (double)n2);
    if (sim > 1.0) sim = 1.0;
    if (sim < -1.0) sim = -1.0;
    return 1.0 - sim;
}

// candidates c_id/c_key[0..n) "in the order given" (:2629) -> s_id/s_key[0..n_sel). Whole workgroup (256 threads).
// ORDER-PRESERVING: every caller but one hands over a list ascending by (key,id), yet nothing below relies on that -- a candidate
// is tested against the kept ones before it (m1: kept in earlier blocks, m2 + selmask: kept earlier in its own block), the loop
// stops at maxm kept, the discarded are recorded and back-filled in the order they were met; no early-out compares keys of two
// candidates.  The reverse prune of Add (add_reverse_kernel) hands over a list's STORED order with the new node last.
template <int METRIC, int PREC>
__device__ void select_neighbors_wg(const KdbView &v, const PruneLdsT<typename BKey<PREC>::T> &p, uint32_t n, uint32_t maxm) {
    using KT = typename BKey<PREC>::T;
    constexpr bool I8 = PREC == KDB_PREC_I8;
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        p.misc[0] = 0;
        p.misc[1] = 0;
    }
    __syncthreads();
    if (n <= maxm) { // "len(candidates) <= m: return candidates" (:2634-2636)
        for (uint32_t i = (uint32_t)tid; i < n; i += 256) {
            p.s_id[i] = p.c_id[i];
            p.s_key[i] = p.c_key[i];
        }
        if (tid == 0) p.misc[0] = n;
        __syncthreads();
        return;
    }
    const float *rows = reinterpret_cast<const float *>(v.rows);
    const uint16_t *rows16 = reinterpret_cast<const uint16_t *>(v.rows); // PREC == F16: widened (exactly) into the f32 LDS tile
    const uint32_t *rows8w = reinterpret_cast<const uint32_t *>(v.rows); // PREC == I8: four packed int8 per tile word
    const uint32_t W = I8 ? v.ld >> 2 : v.ld;                            // row length in tile words
    for (uint32_t b0 = 0; b0 < n; b0 += PR_BLK) {
        const uint32_t nb = n - b0 < PR_BLK ? n - b0 : PR_BLK;
        const uint32_t ns = p.misc[0];
        const uint32_t p1 = nb * ns, p2 = nb * (nb - 1) / 2, np = p1 + p2;
        float acc[PR_U];
        int iacc[PR_U]; // int8: exact i32 dots
        uint32_t ra[PR_U], rb[PR_U];
#pragma unroll
        for (int u = 0; u < PR_U; u++) {
            const uint32_t q = (uint32_t)tid + 256u * (uint32_t)u;
            acc[u] = 0.f;
            iacc[u] = 0;
            ra[u] = 0;
            rb[u] = 0;
            if (q < p1) {
                ra[u] = q / ns;              // block candidate
                rb[u] = PR_BLK + q % ns;     // selected row
            } else if (q < np) {
                const uint32_t t = q - p1;   // triangular: i > i'
                uint32_t i = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
                while (i * (i - 1) / 2 > t) i--;
                while ((i + 1) * i / 2 <= t) i++;
                ra[u] = i;
                rb[u] = t - i * (i - 1) / 2;
            }
        }
        for (uint32_t kc = 0; kc < W; kc += PR_KC) {
            __syncthreads();
            const uint32_t nrow = nb + ns; // staged rows: block candidates then selected
            for (uint32_t e = (uint32_t)tid; e < nrow * (PR_KC / 4); e += 256) {
                const uint32_t r = e / (PR_KC / 4), c4 = e % (PR_KC / 4);
                const uint32_t id = r < nb ? p.c_id[b0 + r] : p.s_id[r - nb];
                const uint32_t lr = r < nb ? r : PR_BLK + (r - nb);
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kc + c4 * 4 < W) {
                    if (I8) {
                        x = *reinterpret_cast<const float4 *>(rows8w + (size_t)id * W + kc + c4 * 4); // 16 int8, bits untouched
                    } else if (PREC == KDB_PREC_F16) {
                        const uint2 h = *reinterpret_cast<const uint2 *>(rows16 + (size_t)id * v.ld + kc + c4 * 4);
                        x = make_float4((float)__builtin_bit_cast(_Float16, (unsigned short)(h.x & 0xffffu)),
                                        (float)__builtin_bit_cast(_Float16, (unsigned short)(h.x >> 16)),
                                        (float)__builtin_bit_cast(_Float16, (unsigned short)(h.y & 0xffffu)),
                                        (float)__builtin_bit_cast(_Float16, (unsigned short)(h.y >> 16)));
                    } else {
                        x = *reinterpret_cast<const float4 *>(rows + (size_t)id * v.ld + kc + c4 * 4);
                    }
                }
                *reinterpret_cast<float4 *>(p.rows + (size_t)lr * PR_STRIDE + c4 * 4) = x;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PR_U; u++) {
                if ((uint32_t)tid + 256u * (uint32_t)u >= np) continue;
                const float4 *a4 = reinterpret_cast<const float4 *>(p.rows + (size_t)ra[u] * PR_STRIDE);
                const float4 *b4 = reinterpret_cast<const float4 *>(p.rows + (size_t)rb[u] * PR_STRIDE);
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                if constexpr (I8) {
                    int d = iacc[u];
#pragma unroll 8
                    for (int c = 0; c < PR_KC / 4; c++) {
                        const int4 x = reinterpret_cast<const int4 *>(a4)[c], y = reinterpret_cast<const int4 *>(b4)[c];
                        d = __builtin_amdgcn_sdot4(x.x, y.x, d, false);
                        d = __builtin_amdgcn_sdot4(x.y, y.y, d, false);
                        d = __builtin_amdgcn_sdot4(x.z, y.z, d, false);
                        d = __builtin_amdgcn_sdot4(x.w, y.w, d, false);
                    }
                    iacc[u] = d;
                    continue;
                }
#pragma unroll 8
                for (int c = 0; c < PR_KC / 4; c++) {
                    const float4 x = a4[c], y = b4[c];
                    if (METRIC == KDB_METRIC_L2) {
                        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
                        a0 = __builtin_fmaf(d0, d0, a0);
                        a1 = __builtin_fmaf(d1, d1, a1);
                        a2 = __builtin_fmaf(d2, d2, a2);
                        a3 = __builtin_fmaf(d3, d3, a3);
                    } else {
                        a0 = __builtin_fmaf(x.x, y.x, a0);
                        a1 = __builtin_fmaf(x.y, y.y, a1);
                        a2 = __builtin_fmaf(x.z, y.z, a2);
                        a3 = __builtin_fmaf(x.w, y.w, a3);
                    }
                }
                acc[u] += (a0 + a1) + (a2 + a3);
            }
        }
#pragma unroll
        for (int u = 0; u < PR_U; u++) {
            const uint32_t q = (uint32_t)tid + 256u * (uint32_t)u;
            if (q >= np) continue;
            KT key;
            if constexpr (I8) {
                const uint32_t ida = p.c_id[b0 + ra[u]], idb = q < p1 ? p.s_id[rb[u] - PR_BLK] : p.c_id[b0 + rb[u]];
                key = i8_pair_distance(iacc[u], v.norms[ida], v.norms[idb]);
            } else {
                key = METRIC == KDB_METRIC_COSINE ? -acc[u] : acc[u];
            }
            if (q < p1) p.m1[ra[u] * PR_MAXSEL + (rb[u] - PR_BLK)] = key;
            else p.m2[ra[u] * PR_BLK + rb[u]] = key;
        }
        __syncthreads();
        if (tid < 64) { // one wave resolves the block in order
            uint32_t nsel = ns, ndisc = p.misc[1];
            unsigned selmask = 0; // block candidates kept so far
            for (uint32_t i = 0; i < nb && nsel < maxm; i++) {
                const KT ek = p.c_key[b0 + i];
                bool rej = false;
                if ((uint32_t)tid < ns) rej = p.m1[i * PR_MAXSEL + (uint32_t)tid] < ek;
                if ((uint32_t)tid < i && ((selmask >> tid) & 1u)) rej = rej || (p.m2[i * PR_BLK + (uint32_t)tid] < ek);
                const bool any = __ballot(rej) != 0ull;
                if (!any) {
                    if (tid == 0) {
                        p.s_id[nsel] = p.c_id[b0 + i];
                        p.s_key[nsel] = ek;
                    }
                    nsel++;
                    selmask |= 1u << i;
                } else {
                    if (tid == 0 && ndisc < (uint32_t)PR_MAXSEL) p.disc[ndisc] = (uint16_t)(b0 + i); // (the back-fill never needs more than maxm of them)
                    ndisc++;
                }
            }
            if (tid == 0) {
                p.misc[0] = nsel;
                p.misc[1] = ndisc;
            }
        }
        __syncthreads();
        if (p.misc[0] >= maxm) break;
    }
    if (tid == 0) { // back-fill from the discarded, in order (:2688-2698)
        uint32_t nsel = p.misc[0];
        const uint32_t ndisc = p.misc[1] < (uint32_t)PR_MAXSEL ? p.misc[1] : (uint32_t)PR_MAXSEL;
        for (uint32_t i = 0; i < ndisc && nsel < maxm; i++) {
            p.s_id[nsel] = p.c_id[p.disc[i]];
            p.s_key[nsel] = p.c_key[p.disc[i]];
            nsel++;
        }
        p.misc[0] = nsel;
    }
    __syncthreads();
}

template <typename KT>
__device__ __forceinline__ bool key_before(KT k1, uint32_t i1, KT k2, uint32_t i2) {
    return (k1 < k2) || (k1 == k2 && i1 < i2);
}

constexpr uint32_t RF_TQ_OFF = 2048; // words of the row tile kept for the unsorted union; the node's own row follows
static_assert((size_t)PR_MAXC * (sizeof(double) + 4) <= (size_t)RF_TQ_OFF * 4, "the union must fit in front of the row");
constexpr uint32_t RF_MAX_ROW_BYTES = (uint32_t)((PR_BLK + PR_MAXSEL) * PR_STRIDE - RF_TQ_OFF) * 4u;

// what Refine, Vacuum's repair and Add share: the limits of the three refine kernels
int refine_limits(const kdb_index *idx, uint32_t efc, const char *who) {
    if (efc < 1 || efc > KDB_MAX_EFC || idx->deg0 > PR_MAXSEL || (size_t)idx->ld * (idx->desc.precision == KDB_PREC_I8 ? 1 : 4) > RF_MAX_ROW_BYTES) {
        kdb_set_error("%s: ef_construction in 1..%u, mMax0 <= %d, rows of at most %u bytes", who, KDB_MAX_EFC, PR_MAXSEL, RF_MAX_ROW_BYTES);
        return KDB_ERR_UNSUPPORTED;
    }
    return KDB_OK;
}

// ---- host pieces ------------------------------------------------------------------------------------
// f(metric, precision) as integral constants, for the index's pair: float16 is euclidean only, int8 cosine only
template <typename F>
int for_metric_prec(const kdb_index *idx, F &&f) {
    using std::integral_constant;
    if (idx->desc.precision == KDB_PREC_F16) return f(integral_constant<int, KDB_METRIC_L2>{}, integral_constant<int, KDB_PREC_F16>{});
    if (idx->desc.precision == KDB_PREC_I8) return f(integral_constant<int, KDB_METRIC_COSINE>{}, integral_constant<int, KDB_PREC_I8>{});
    return idx->desc.metric == KDB_METRIC_COSINE ? f(integral_constant<int, KDB_METRIC_COSINE>{}, integral_constant<int, KDB_PREC_F32>{})
                                                 : f(integral_constant<int, KDB_METRIC_L2>{}, integral_constant<int, KDB_PREC_F32>{});
}

// the construction workspace d_build holds at least `bytes`
int ensure_build_ws(kdb_index *idx, size_t bytes) {
    if (idx->build_bytes >= bytes) return KDB_OK;
    if (idx->d_build) KDB_HIP(hipFree(idx->d_build));
    idx->d_build = nullptr;
    idx->build_bytes = 0;
    KDB_HIP(hipMalloc(&idx->d_build, bytes));
    idx->build_bytes = bytes;
    return KDB_OK;
}

// The upper pool holds `slots` slots, the ones behind the lists in use zeroed.  keep_old: the first up_slots slots are in use
// (else none: rows without a graph).  A pool that is too small is replaced by a larger one filled with what the old one holds:
// the same lists, so no other field of the handle changes its meaning and a caller that fails later has nothing to put back.
int grow_upper_pool(kdb_index *idx, size_t slots, bool keep_old, hipStream_t s) {
    const size_t have = keep_old ? idx->up_slots : 0;
    if (slots > idx->up_slots_cap || !idx->d_adj_up) {
        const size_t grown_cap = slots + slots / 2 + 1024;
        uint32_t *grown = nullptr;
        KDB_HIP(hipMalloc(&grown, (grown_cap * idx->deg_up + 4) * 4));
        hipError_t e = hipMemsetAsync(grown, 0, (grown_cap * idx->deg_up + 4) * 4, s);
        if (e == hipSuccess && idx->d_adj_up && have) e = hipMemcpyAsync(grown, idx->d_adj_up, have * idx->deg_up * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(grown);
            KDB_HIP(e);
        }
        if (idx->d_adj_up) (void)hipFree(idx->d_adj_up);
        idx->d_adj_up = grown;
        idx->up_slots_cap = grown_cap;
    } else if (slots > have) {
        KDB_HIP(hipMemsetAsync(idx->d_adj_up + have * idx->deg_up, 0, (slots - have) * idx->deg_up * 4, s));
    }
    return KDB_OK;
}

// the walk kernel K<METRIC, BS, PREC> of a plan's beam storage (wl.bs: 0, 2 or 4)
#define KDB_WALK_KERNEL(K, wl) ((wl).bs == 0 ? K<METRIC, 0, PREC> : (wl).bs == 2 ? K<METRIC, 2, PREC> : K<METRIC, 4, PREC>)

// a walker with one wave per workgroup and a visited bitset per resident workgroup: its LDS allowed, the pool sized
template <typename K>
int walk_pool_prepare(kdb_index *idx, K kern, const KdbWalkLds &wl, hipStream_t s, uint32_t *slots_vis) {
    if (wl.bytes > 64 * 1024) KDB_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl.bytes));
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 64, wl.bytes) != hipSuccess || nb < 1) nb = 1;
    *slots_vis = (uint32_t)idx->n_cu * (uint32_t)nb;
    return kdb_ensure_visited(idx, *slots_vis, s);
}

} // namespace
