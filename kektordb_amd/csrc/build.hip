// build.hip -- GPU batched HNSW construction for gfx950.
//
// Follows the phases of the reference's batch insert, addBatchInternal
// (pkg/core/hnsw/hnsw_index.go:1479-2088):
//   phase 1  every new node of a batch searches the frozen graph in parallel (:1766-1855):
//            greedy zoom-in with ef=1 above its level, then searchLayer(ef=efConstruction) per level
//            -- here one wavefront per new node, the same search_layer() as the query path;
//   phase 2  neighbour selection + link requests (:1864-1890): the new node keeps
//            selectNeighbors(candidates, maxM) (:2629-2701) and sends one reverse request to each
//            neighbour it kept -- the link rule of the sequential Add (:711-783); the reference's
//            batch path instead requests all efConstruction candidates, which costs ~6x more
//            prunes for the same graph degree (documented divergence);
//   phase 3  per-target commit (:1902-2060): existing links + requesters; if they fit in maxM they
//            are appended, otherwise the union is sorted by distance to the target and pruned with
//            selectNeighbors -- one workgroup per touched (target, level);
//   phase 4  entry point / maxLevel update (:2066-2080), on the host.
// Levels are drawn on the host as randomLevel() does (:2616-2625): floor(-ln U / ln m), capped at
// currentMax+1, from a seeded splitmix64 stream (the reference uses the auto-seeded global RNG).
//
// Distances: float32 / float16 rows order their candidates by float keys (squared L2, minus the dot product); int8 rows
// (cosine only) by the reference's float64 distance 1 - dot / (|a| |b|) (hnsw_index.go:317-336 node<->node, :2406-2454
// query<->node): the i32 dot is exact in any order, so every int8 distance -- and with it every link decision -- is the
// oracle's bit for bit.  The key type KT (float / double) is a template parameter of everything below.
//
// selectNeighbors on the GPU: candidates are visited in blocks of 32; the block's rows and the rows
// selected so far are staged through LDS in K-chunks, every (candidate, selected) and
// (candidate, earlier candidate) distance of the block is accumulated by the 256 threads, then one
// wave resolves the block sequentially from those matrices -- exactly the reference's rule: keep e
// unless some kept r has d(e,r) < d(e,centre); stop at m; back-fill from the discarded in order.
//
// This file: the fast builder (build_impl), reference linking (rl_*, add_batch_ref_impl) and the selectNeighbors test hook.
// Refine and Vacuum are refine.hip, the sequential Add is add.hip; what the three share is kdb_graph_build.cuh.
#include "kdb_graph_build.cuh"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr uint32_t RCAP = 16;         // reverse requests kept per (target, level) per batch
constexpr uint32_t UP_FLAG = 0x80000000u;

template <typename KT>
struct BuildViewT {
    uint32_t *adj0;      // writable graph
    uint32_t *adj_up;
    KT *adj0_key;        // distance (key) of every stored link to its owner
    KT *adj_up_key;
    uint32_t *rev0_cnt;  // [(cap+1)]
    uint32_t *revup_cnt; // [up slots]
    uint32_t *rev0_id;   // [(cap+1) * RCAP]
    KT *rev0_key;
    uint32_t *revup_id;  // [up slots * RCAP]
    KT *revup_key;
    uint32_t *touched;   // touched (target, level) codes
    uint32_t *n_touched;
    uint32_t *cand_id;   // [tasks * efc]
    KT *cand_key;
    uint32_t *cand_cnt;  // [tasks]
    uint32_t *up_task;   // [batch] first upper task of a batch node
    // reverse requests beyond the RCAP slots of their target (hubs): appended here, so that the commit can keep the RCAP NEAREST
    // requesters whatever order they arrived in (two builds of the same rows then give the same graph)
    uint32_t *ov_code;   // [ov_cap] target code (level-0 id, or UP_FLAG | upper slot)
    uint32_t *ov_id;     // [ov_cap] requester
    KT *ov_key;          // [ov_cap] its distance to the target
    uint32_t *ov_cnt;    // entries appended this batch
    uint32_t ov_cap;
    uint32_t efc;
    uint32_t first;      // first id of the batch
    uint32_t nb;         // batch size
    uint32_t n_tasks;
};

// ---- phase 1 ------------------------------------------------------------------------------------
template <int METRIC, int BS, int PREC>
__global__ void __launch_bounds__(64)
build_search_kernel(KdbView v, BuildViewT<typename BKey<PREC>::T> bv, uint32_t beam_cap, uint32_t nr_cap, uint32_t *visited_pool, uint32_t *work) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool I8 = PREC == KDB_PREC_I8;
    WaveLds s;
    VisBitset vis;
    walk_carve<BS, I8>(smem, v, beam_cap, nr_cap, visited_pool + (size_t)blockIdx.x * v.vis_words, s, vis);
    const int lane = kdb_lane();
    for (;;) {
        uint32_t bi = 0;
        if (lane == 0) bi = atomicAdd(work, 1u);
        bi = __shfl(bi, 0, 64);
        if (bi >= bv.nb) break;
        const uint32_t node = bv.first + bi;
        const int L = (int)v.levels[node];
        WalkBeam<BS, I8> b;
        const float qnorm = walk_start<PREC>(v, s, vis, b, node, lane);
        QCtr ctr{};
        uint32_t ep = v.entry;
        EpKnown epk;
        for (int l = v.max_level; l >= 0; l--) {
            const bool insert = l <= L;
            search_layer<PREC, METRIC, 0>(v, s, b, vis, nullptr, ep, l, insert ? bv.efc : 1u, qnorm, ctr, epk);
            if (insert) {
                const uint32_t task = l == 0 ? bi : bv.nb + bv.up_task[bi] + (uint32_t)(l - 1);
                uint32_t nc;
                if constexpr (I8)
                    nc = b.write_results(bv.efc, bv.cand_id + (size_t)task * bv.efc, nullptr, false, bv.cand_key + (size_t)task * bv.efc);
                else
                    nc = b.write_results(bv.efc, bv.cand_id + (size_t)task * bv.efc, bv.cand_key + (size_t)task * bv.efc, false);
                if (lane == 0) bv.cand_cnt[task] = nc;
            }
            walk_nearest(b, ep, epk);
        }
    }
}

// task -> (node, level): tasks [0, nb) are the level-0 searches of the batch, the upper ones follow in node order
template <typename KT>
__device__ __forceinline__ void task_owner(const BuildViewT<KT> &bv, uint32_t task, uint32_t &node, uint32_t &level) {
    if (task < bv.nb) {
        node = bv.first + task;
        level = 0;
        return;
    }
    // upper task: find owner by binary search over up_task (non-decreasing)
    const uint32_t ut = task - bv.nb;
    uint32_t lo = 0, hi = bv.nb - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (bv.up_task[mid] <= ut) lo = mid; else hi = mid - 1;
    }
    // several batch nodes without upper levels share the same up_task value: take the one that owns it
    while (lo + 1 < bv.nb && bv.up_task[lo + 1] <= ut) lo++;
    node = bv.first + lo;
    level = ut - bv.up_task[lo] + 1;
}

// ---- phase 2: new node keeps selectNeighbors(cands); emits reverse requests ---------------------------
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
build_select_kernel(KdbView v, BuildViewT<typename BKey<PREC>::T> bv) {
    using KT = typename BKey<PREC>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const int tid = (int)threadIdx.x;
    const uint32_t task = blockIdx.x;
    uint32_t node, level;
    task_owner(bv, task, node, level);
    const uint32_t n = bv.cand_cnt[task];
    const uint32_t maxm = level == 0 ? v.deg0 : v.deg_up;
    for (uint32_t i = (uint32_t)tid; i < n; i += 256) {
        p.c_id[i] = bv.cand_id[(size_t)task * bv.efc + i];
        p.c_key[i] = bv.cand_key[(size_t)task * bv.efc + i];
    }
    __syncthreads();
    select_neighbors_wg<METRIC, PREC>(v, p, n, maxm);
    const uint32_t nsel = p.misc[0];
    uint32_t *adj = adj_of(bv.adj0, bv.adj_up, v, node, level);
    KT *akey = adj_of(bv.adj0_key, bv.adj_up_key, v, node, level);
    if ((uint32_t)tid < maxm) {
        adj[tid] = (uint32_t)tid < nsel ? p.s_id[tid] : 0u;
        akey[tid] = (uint32_t)tid < nsel ? p.s_key[tid] : (KT)0;
    }
    if ((uint32_t)tid < nsel) { // reverse link requests (:1883-1889)
        const uint32_t t = p.s_id[tid];
        uint32_t *cnt;
        uint32_t *rid;
        KT *rkey;
        uint32_t code;
        if (level == 0) {
            cnt = bv.rev0_cnt + t;
            rid = bv.rev0_id + (size_t)t * RCAP;
            rkey = bv.rev0_key + (size_t)t * RCAP;
            code = t;
        } else {
            const uint32_t ts = v.up_idx[t] + (level - 1);
            cnt = bv.revup_cnt + ts;
            rid = bv.revup_id + (size_t)ts * RCAP;
            rkey = bv.revup_key + (size_t)ts * RCAP;
            code = UP_FLAG | ts;
        }
        const uint32_t slot = atomicAdd(cnt, 1u);
        if (slot < RCAP) {
            rid[slot] = node;
            rkey[slot] = p.s_key[tid];
        } else { // a hub: parked; the commit picks the RCAP nearest of ALL its requesters
            const uint32_t o = atomicAdd(bv.ov_cnt, 1u);
            if (o < bv.ov_cap) {
                bv.ov_code[o] = code;
                bv.ov_id[o] = node;
                bv.ov_key[o] = p.s_key[tid];
            }
        }
        if (slot == 0) bv.touched[atomicAdd(bv.n_touched, 1u)] = code;
    }
}

// ---- phase 3: per-target commit -----------------------------------------------------------------------
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
build_reverse_kernel(KdbView v, BuildViewT<typename BKey<PREC>::T> bv, uint32_t n_touched) {
    using KT = typename BKey<PREC>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const int tid = (int)threadIdx.x;
    if (blockIdx.x >= n_touched) return;
    const uint32_t code = bv.touched[blockIdx.x];
    uint32_t *adj, *cnt, *rid;
    KT *akey, *rkey;
    uint32_t maxm;
    if (code & UP_FLAG) {
        const uint32_t ts = code & ~UP_FLAG;
        adj = bv.adj_up + (size_t)ts * v.deg_up;
        akey = bv.adj_up_key + (size_t)ts * v.deg_up;
        cnt = bv.revup_cnt + ts;
        rid = bv.revup_id + (size_t)ts * RCAP;
        rkey = bv.revup_key + (size_t)ts * RCAP;
        maxm = v.deg_up;
    } else {
        adj = bv.adj0 + (size_t)code * v.deg0;
        akey = bv.adj0_key + (size_t)code * v.deg0;
        cnt = bv.rev0_cnt + code;
        rid = bv.rev0_id + (size_t)code * RCAP;
        rkey = bv.rev0_key + (size_t)code * RCAP;
        maxm = v.deg0;
    }
    uint32_t &sh_ne = p.misc[2], &sh_nr = p.misc[3], &sh_all = p.misc[4], &sh_g = p.misc[5];
    if (tid == 0) {
        const uint32_t all = *cnt;
        sh_ne = list_len(adj, maxm);
        sh_nr = all > RCAP ? RCAP : all;
        sh_all = all;
        sh_g = 0u;
        *cnt = 0; // ready for the next batch
    }
    __syncthreads();
    if (sh_all > RCAP) {
        // A hub: more requesters than slots.  Which RCAP of them reached the slots first is an accident of scheduling; the ones
        // that stay are the RCAP NEAREST by (distance, id): the slot entries and the target's parked requests are gathered into
        // LDS (the row tile is idle here), sorted, and the first RCAP written back to the slots.
        constexpr uint32_t GCAP = 4096u; // a power of two (the sort pads to one); 48 KB of the 50 KB row tile with 8-byte keys
        static_assert((size_t)GCAP * (sizeof(KT) + 4) <= (size_t)(PR_BLK + PR_MAXSEL) * PR_STRIDE * 4, "hub scratch must fit the row tile");
        KT *g_key = reinterpret_cast<KT *>(p.rows);
        uint32_t *g_id = reinterpret_cast<uint32_t *>(g_key + GCAP);
        if ((uint32_t)tid < RCAP) {
            g_key[tid] = rkey[tid];
            g_id[tid] = rid[tid];
        }
        if (tid == 0) sh_g = RCAP;
        __syncthreads();
        const uint32_t n_ov = *bv.ov_cnt < bv.ov_cap ? *bv.ov_cnt : bv.ov_cap;
        for (uint32_t i = (uint32_t)tid; i < n_ov; i += 256)
            if (bv.ov_code[i] == code) {
                const uint32_t at = atomicAdd(&sh_g, 1u);
                if (at < GCAP) { // (a target with more than GCAP = 4096 requesters in ONE batch keeps the first GCAP found)
                    g_key[at] = bv.ov_key[i];
                    g_id[at] = bv.ov_id[i];
                }
            }
        __syncthreads();
        sort_by_key_id_wg(g_key, g_id, sh_g < GCAP ? sh_g : GCAP);
        if ((uint32_t)tid < RCAP) {
            rid[tid] = g_id[tid];
            rkey[tid] = g_key[tid];
        }
        __threadfence_block();
        __syncthreads();
    }
    const uint32_t ne = sh_ne, nr = sh_nr;
    const uint32_t n = ne + nr;
    // gather E then R; requesters ordered by id so the result does not depend on atomic order
    uint32_t my_id = 0;
    KT my_key = 0;
    if ((uint32_t)tid < ne) {
        my_id = adj[tid];
        my_key = akey[tid];
    } else if ((uint32_t)tid < n) {
        my_id = rid[tid - ne];
        my_key = rkey[tid - ne];
    }
    if (n <= maxm) { // fast path: append (Add, :746-751)
        if ((uint32_t)tid >= ne && (uint32_t)tid < n) {
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nr; j++) rank += rid[j] < my_id ? 1u : 0u;
            adj[ne + rank] = my_id;
            akey[ne + rank] = my_key;
        }
        return;
    }
    // prune: union sorted by distance to the target (:2019-2033), then selectNeighbors
    uint32_t *sh_id = reinterpret_cast<uint32_t *>(p.m1);      // m1/m2 are free until select_neighbors_wg
    KT *sh_key = p.m2;
    if ((uint32_t)tid < n) {
        sh_id[tid] = my_id;
        sh_key[tid] = my_key;
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) rank += key_before(sh_key[j], sh_id[j], my_key, my_id) ? 1u : 0u;
        p.c_id[rank] = my_id;
        p.c_key[rank] = my_key;
    }
    __syncthreads();
    select_neighbors_wg<METRIC, PREC>(v, p, n, maxm);
    const uint32_t nsel = p.misc[0];
    if ((uint32_t)tid < maxm) {
        adj[tid] = (uint32_t)tid < nsel ? p.s_id[tid] : 0u;
        akey[tid] = (uint32_t)tid < nsel ? p.s_key[tid] : (KT)0;
    }
}

// =====================================================================================================================
// Reference linking (kdb_index_add_batch): phases 2 and 3 of addBatchInternal AS WRITTEN (:1864-2060), so that the lists
// can be compared with the restated batch insert (oracle: orc_index_add_batch) link for link:
//   * every new node asks for ALL its efConstruction candidates (direct request), and every candidate gets a reverse
//     request for the new node (:1869-1889) -- not only the neighbours the node keeps, no cap per target;
//   * per (target, level): current links + requested ids, sorted, de-duplicated, without the node itself (:1983-2003);
//     up to maxM of them are stored AS THEY ARE, in ascending id order (:2011-2013); more are scored against the target
//     (distanceBetweenNodes, nil / deleted candidates dropped), sorted by distance -- the unstable sort's tie order restated
//     as (distance, id), as in the oracle -- and pruned by selectNeighbors (:2015-2040).
// A target is one workgroup; its union (<= maxM + batch size entries) is sorted in LDS.
// =====================================================================================================================
constexpr uint32_t RL_UCAP = 4096; // union entries per (target, level) sorted in LDS; longer unions go through HBM scratch (rl_commit_big_kernel)

// combined request counters: [0, n1) level-0 targets by id, [n1, n1 + slots] upper targets by slot
// reuse_id / reuse_levels: the slot the batch's first node took over (hnsw_index.go:1620; 0 = none) and the number of upper
// slots it owns = max(its new level, the level of the node it replaced).  Old links still name it at the replaced node's
// levels, so a walk can meet it ABOVE its new level and ask it for a reverse link there; the reference then grows that node's
// Connections (:2049-2053).  Its slots are allocated up front; *grew (atomicMax) records the highest level that was asked for.
template <typename KT>
__global__ void __launch_bounds__(256)
rl_count_kernel(KdbView v, BuildViewT<KT> bv, uint32_t n1, uint32_t *cnt, uint32_t *slot_owner, uint32_t *cursor /* null: count; else fill */,
                const uint32_t *off, uint32_t *req, uint32_t *err, uint32_t reuse_id, uint32_t reuse_levels, uint32_t *grew) {
    const uint32_t task = blockIdx.x;
    uint32_t node, level;
    task_owner(bv, task, node, level);
    const uint32_t n = bv.cand_cnt[task];
    if (n == 0) return;
    const uint32_t own = level == 0 ? node : n1 + v.up_idx[node] + (level - 1u);
    if (threadIdx.x == 0 && !cursor) {
        atomicAdd(&cnt[own], n); // the direct request: all candidates
        if (level) slot_owner[own - n1] = node;
    }
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint32_t c = bv.cand_id[(size_t)task * bv.efc + i];
        if (cursor) req[off[own] + atomicAdd(&cursor[own], 1u)] = c;
        uint32_t code = c;
        if (level) {
            // a candidate evaluated at a level above its own: only the slot the reference's batch path re-uses (:1620) can be
            // one -- the reference then GROWS that node's Connections; the fixed upper slots here cannot: counted, skipped
            if ((uint32_t)v.levels[c] < level) {
                if (c != reuse_id || level > reuse_levels) { // (cannot happen: only the re-used slot is ever met above its level)
                    if (!cursor) atomicAdd(err, 1u);
                    continue;
                }
                if (!cursor) atomicMax(grew, level);
            }
            code = n1 + v.up_idx[c] + (level - 1u);
            if (!cursor) slot_owner[code - n1] = c;
        }
        if (cursor) req[off[code] + atomicAdd(&cursor[code], 1u)] = node;
        else atomicAdd(&cnt[code], 1u);
    }
}
// exclusive prefix over the counters; touched targets appended (order irrelevant); out[0] = total, out[1] = n_touched
__global__ void __launch_bounds__(1024)
rl_scan_kernel(const uint32_t *cnt, uint32_t L, uint32_t *off, uint32_t *touched, uint32_t *out) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < L; i0 += 1024) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t c = i < L ? cnt[i] : 0u;
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
            if ((threadIdx.x & 63u) >= (uint32_t)o) inc += t;
        }
        if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t base = carry + inc - c;
        for (uint32_t j = 0; j < (threadIdx.x >> 6); j++) base += wsum[j];
        if (i < L) off[i] = base;
        if (c) touched[atomicAdd(&out[1], 1u)] = i;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int j = 0; j < 16; j++) t += wsum[j];
            carry += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = carry;
}

template <typename T>
__device__ __forceinline__ void rl_swap(T &a, T &b) { T t = a; a = b; b = t; }

// One (target, level): current links + requests -> the new list (phase 3 as written, :1975-2055).  The union lives in u_id /
// u_key / u_tmp (`ucap` entries, a power of two): LDS for ordinary targets, HBM scratch for the few whose union outgrows it
// (rl_commit_big_kernel) -- the code is the same, __syncthreads orders both.
template <int METRIC, int PREC>
__device__ void rl_commit_body(const KdbView &v, PruneLdsT<typename BKey<PREC>::T> &p, uint32_t *adj, uint32_t maxm, uint32_t t, uint32_t ne,
                               const uint32_t *req_t, uint32_t nreq, typename BKey<PREC>::T *u_key, uint32_t *u_id, uint32_t *u_tmp, const ScoreLds &sl,
                               uint32_t *sh) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nu = ne + nreq;
    uint32_t P = 64;
    while (P < nu) P <<= 1;
    for (uint32_t i = tid; i < P; i += 256) u_id[i] = i < ne ? adj[i] : i < nu ? req_t[i - ne] : 0xffffffffu;
    __syncthreads();
    // slices.Sort(uniqueIDs) (:1985)
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += 256) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0u;
                    uint32_t x = u_id[i], y = u_id[l];
                    if ((x > y) == up) {
                        u_id[i] = y;
                        u_id[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    // de-duplication without the node itself (:1987-2003); candidates that are nil or deleted never reach the prune
    // (:2019-2024) -- but they DO count for "uniqCount <= maxM" and are stored then, exactly as the reference does
    auto compact = [&](bool drop_deleted) -> uint32_t { // u_id[0..P) sorted -> u_tmp[0..nq) ; returns nq
        if (tid == 0) sh[1] = 0;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < P; i0 += 256) {
            const uint32_t i = i0 + tid;
            const uint32_t x = i < P ? u_id[i] : 0xffffffffu;
            bool keep = x != 0xffffffffu && x != t && (i == 0 || u_id[i - 1] != x);
            if (keep && drop_deleted) keep = !is_deleted(v, x) && x <= v.count;
            const unsigned long long m = __ballot(keep);
            if (lane == 0) sh[4 + wave] = (uint32_t)__builtin_popcountll(m);
            __syncthreads();
            uint32_t base = sh[1];
            for (uint32_t w = 0; w < wave; w++) base += sh[4 + w];
            if (keep) u_tmp[base + kdb_mbcnt(m)] = x;
            __syncthreads();
            if (tid == 0) sh[1] += sh[4] + sh[5] + sh[6] + sh[7];
            __syncthreads();
        }
        return sh[1];
    };
    const uint32_t nq = compact(false);
    if (nq <= maxm) { // the union as it is: ascending ids (:2011-2013)
        if (tid < maxm) adj[tid] = tid < nq ? u_tmp[tid] : 0u;
        return;
    }
    __syncthreads();
    const uint32_t np = compact(true); // the candidates of the prune
    __syncthreads();
    // distanceBetweenNodes(node, candidate) (:297-340): the target's stored row is the query, 16 lanes per candidate row
    const float qnorm = load_row_as_query<PREC, 256>(v, sl.tq, t, tid);
    for (uint32_t i = tid; i < np; i += 256) u_id[i] = u_tmp[i];
    __syncthreads();
    score_ids_wg<METRIC, PREC>(v, sl, qnorm, u_id, np, u_key);
    __syncthreads();
    // slices.SortFunc by distance (:2026-2034); equal distances: by id (the restated tie order)
    sort_by_key_id_wg(u_key, u_id, np);
    p.c_id = u_id;
    p.c_key = u_key;
    select_neighbors_wg<METRIC, PREC>(v, p, np, maxm);
    const uint32_t nsel = p.misc[0];
    if (tid < maxm) adj[tid] = tid < nsel ? p.s_id[tid] : 0u;
}

// which (target, level) a touched code names
__device__ __forceinline__ void rl_target(const KdbView &v, uint32_t code, uint32_t n1, const uint32_t *slot_owner, uint32_t *adj0, uint32_t *adj_up,
                                          uint32_t &t, uint32_t &maxm, uint32_t *&adj) {
    if (code < n1) {
        t = code;
        maxm = v.deg0;
        adj = adj0 + (size_t)t * v.deg0;
    } else {
        const uint32_t ts = code - n1;
        t = slot_owner[ts];
        maxm = v.deg_up;
        adj = adj_up + (size_t)ts * v.deg_up;
    }
}

// ucap: union entries the LDS holds (a power of two); targets beyond it are listed for rl_commit_big_kernel (err[1] counts them)
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
rl_commit_kernel(KdbView v, uint32_t *adj0, uint32_t *adj_up, uint32_t n1, const uint32_t *touched, const uint32_t *cnt, const uint32_t *off,
                 const uint32_t *req, const uint32_t *slot_owner, uint32_t *err, uint32_t ucap, uint32_t *big_list) {
    using KT = typename BKey<PREC>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    size_t o = prune_lds_bytes<KT>();
    KT *u_key = reinterpret_cast<KT *>(smem + o);
    o += (size_t)ucap * sizeof(KT);
    uint32_t *u_id = reinterpret_cast<uint32_t *>(smem + o);
    o += (size_t)ucap * 4;
    uint32_t *u_tmp = reinterpret_cast<uint32_t *>(smem + o); // de-dup scratch
    o += (size_t)ucap * 4;
    const ScoreLds sl = score_carve<PREC == KDB_PREC_I8>(smem + o, v); // the target's row as the query
    __shared__ uint32_t sh[8];
    const uint32_t tid = threadIdx.x;
    const uint32_t code = touched[blockIdx.x];
    uint32_t t, maxm;
    uint32_t *adj;
    rl_target(v, code, n1, slot_owner, adj0, adj_up, t, maxm, adj);
    if (is_deleted(v, t)) return; // "node == nil || node.Deleted: skip" (:1927-1930)
    const uint32_t nreq = cnt[code];
    if (tid == 0) sh[0] = list_len(adj, maxm);
    __syncthreads();
    const uint32_t ne = sh[0];
    if (ne + nreq > ucap) { // a hub of this batch: its union is sorted in HBM scratch by the second kernel
        if (tid == 0) big_list[atomicAdd(err + 1, 1u)] = code;
        return;
    }
    rl_commit_body<METRIC, PREC>(v, p, adj, maxm, t, ne, req + off[code], nreq, u_key, u_id, u_tmp, sl, sh);
}

// the targets rl_commit_kernel passed on: big_list[first + blockIdx.x], union in this workgroup's slice of `scratch`
// (ucap entries: keys | ids | de-dup scratch)
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
rl_commit_big_kernel(KdbView v, uint32_t *adj0, uint32_t *adj_up, uint32_t n1, const uint32_t *big_list, uint32_t first, const uint32_t *cnt,
                     const uint32_t *off, const uint32_t *req, const uint32_t *slot_owner, uint32_t ucap, unsigned char *scratch, uint32_t *err) {
    using KT = typename BKey<PREC>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const ScoreLds sl = score_carve<PREC == KDB_PREC_I8>(smem + prune_lds_bytes<KT>(), v);
    __shared__ uint32_t sh[8];
    unsigned char *mine = scratch + (size_t)blockIdx.x * ucap * (sizeof(KT) + 8);
    KT *u_key = reinterpret_cast<KT *>(mine);
    uint32_t *u_id = reinterpret_cast<uint32_t *>(mine + (size_t)ucap * sizeof(KT));
    uint32_t *u_tmp = u_id + ucap;
    const uint32_t tid = threadIdx.x;
    const uint32_t code = big_list[first + blockIdx.x];
    uint32_t t, maxm;
    uint32_t *adj;
    rl_target(v, code, n1, slot_owner, adj0, adj_up, t, maxm, adj);
    const uint32_t nreq = cnt[code];
    if (tid == 0) sh[0] = list_len(adj, maxm);
    __syncthreads();
    const uint32_t ne = sh[0];
    if (ne + nreq > ucap) { // (cannot happen: ucap covers maxM + every request a batch can send one target)
        if (tid == 0) atomicAdd(err + 2, 1u);
        return;
    }
    rl_commit_body<METRIC, PREC>(v, p, adj, maxm, t, ne, req + off[code], nreq, u_key, u_id, u_tmp, sl, sh);
}

// ---- test hook: selectNeighbors on caller-supplied candidate lists (kdb_test_select_neighbors) -----------------------
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
select_probe_kernel(KdbView v, const uint32_t *cand_id, const typename BKey<PREC>::T *cand_key, const uint32_t *cand_cnt, uint32_t stride,
                    uint32_t maxm, uint32_t *out_id, uint32_t *out_cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<typename BKey<PREC>::T> p;
    prune_carve(smem, p);
    const int tid = (int)threadIdx.x;
    const uint32_t task = blockIdx.x;
    const uint32_t n = cand_cnt[task];
    for (uint32_t i = (uint32_t)tid; i < n; i += 256) {
        p.c_id[i] = cand_id[(size_t)task * stride + i];
        p.c_key[i] = cand_key[(size_t)task * stride + i];
    }
    __syncthreads();
    select_neighbors_wg<METRIC, PREC>(v, p, n, maxm);
    const uint32_t nsel = p.misc[0];
    if ((uint32_t)tid < maxm) out_id[(size_t)task * maxm + tid] = (uint32_t)tid < nsel ? p.s_id[tid] : 0u;
    if (tid == 0) out_cnt[task] = nsel;
}

uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <int METRIC, int PREC>
int build_impl(kdb_index *idx, uint32_t count, const kdb_build_params *bp) {
    using KT = typename BKey<PREC>::T;
    constexpr size_t KB = sizeof(KT);
    hipStream_t s = idx->stream;
    const uint32_t efc = bp && bp->ef_construction ? bp->ef_construction : idx->desc.ef_construction;
    if (efc > KDB_MAX_EFC || efc < 1) {
        kdb_set_error("build: ef_construction must be in 1..%u (got %u)", KDB_MAX_EFC, efc);
        return KDB_ERR_UNSUPPORTED;
    }
    const uint32_t max_batch = bp && bp->batch ? bp->batch : 16384u;
    uint64_t seed = bp ? bp->seed : 1ull;
    const uint32_t m = idx->desc.m;
    const double ml = 1.0 / std::log((double)m);
    // ---- levels (randomLevel, :2616-2625), upper-slot prefix, entry/maxLevel trajectory
    const size_t n1 = (size_t)count + 1;
    std::vector<uint8_t> levels(n1, 0);
    std::vector<uint32_t> up_idx(n1, 0);
    size_t slots = 0;
    int curmax = -1;
    for (uint32_t i = 1; i <= count; i++) {
        double u;
        do { u = (double)(splitmix64(seed) >> 11) * (1.0 / 9007199254740992.0); } while (u <= 0.0);
        int lv = (int)std::floor(-std::log(u) * ml);
        if (lv > curmax + 1) lv = curmax + 1;
        if (lv > 250) lv = 250;
        levels[i] = (uint8_t)lv;
        if (lv > curmax) curmax = lv;
        up_idx[i] = (uint32_t)slots;
        slots += (size_t)lv;
    }
    // ---- graph storage
    if (slots > idx->up_slots_cap || !idx->d_adj_up) {
        if (idx->d_adj_up) KDB_HIP(hipFree(idx->d_adj_up));
        idx->d_adj_up = nullptr;
        KDB_HIP(hipMalloc(&idx->d_adj_up, (slots * idx->deg_up + 4) * 4));
        idx->up_slots_cap = slots;
    }
    idx->up_slots = slots;
    KDB_HIP(hipMemsetAsync(idx->d_adj0, 0, ((size_t)idx->cap + 1) * idx->deg0 * 4, s));
    KDB_HIP(hipMemsetAsync(idx->d_adj_up, 0, (slots * idx->deg_up + 4) * 4, s));
    KDB_HIP(hipMemcpyAsync(idx->d_levels, levels.data(), n1, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(idx->d_up_idx, up_idx.data(), n1 * 4, hipMemcpyHostToDevice, s));
    idx->h_levels = levels; // host copies for the incremental refresh entry points
    idx->h_up_idx = up_idx;
    // ---- workspace
    const size_t max_tasks = (size_t)max_batch * 2 + 64; // level-0 tasks + upper tasks (<< batch)
    KdbCarver c;
    const size_t o_adj0k = c.take(n1 * idx->deg0 * KB), o_adjupk = c.take((slots * idx->deg_up + 4) * KB);
    const size_t o_r0c = c.take(n1 * 4), o_ruc = c.take((slots + 1) * 4);
    const size_t o_r0i = c.take(n1 * RCAP * 4), o_r0k = c.take(n1 * RCAP * KB);
    const size_t o_rui = c.take((slots + 1) * RCAP * 4), o_ruk = c.take((slots + 1) * RCAP * KB);
    const size_t o_touch = c.take(((size_t)max_tasks * PR_MAXSEL + 64) * 4), o_ntouch = c.take(256);
    const size_t o_cid = c.take(max_tasks * efc * 4), o_ckey = c.take(max_tasks * efc * KB), o_ccnt = c.take(max_tasks * 4);
    const size_t o_uptask = c.take((size_t)max_batch * 4 + 64);
    // parked reverse requests of hubs: every selected neighbour of a batch could be one (max_tasks * maxM0); in practice a few hundred
    const size_t ov_cap = max_tasks * (size_t)idx->deg0;
    const size_t o_ovc = c.take(ov_cap * 4), o_ovi = c.take(ov_cap * 4), o_ovk = c.take(ov_cap * KB), o_ovn = c.take(256);
    int rc = ensure_build_ws(idx, c.total());
    if (rc) return rc;
    unsigned char *w = reinterpret_cast<unsigned char *>(idx->d_build);
    KDB_HIP(hipMemsetAsync(w + o_r0c, 0, n1 * 4, s));
    KDB_HIP(hipMemsetAsync(w + o_ruc, 0, (slots + 1) * 4, s));
    BuildViewT<KT> bv;
    bv.adj0 = idx->d_adj0;
    bv.adj_up = idx->d_adj_up;
    bv.adj0_key = reinterpret_cast<KT *>(w + o_adj0k);
    bv.adj_up_key = reinterpret_cast<KT *>(w + o_adjupk);
    bv.rev0_cnt = reinterpret_cast<uint32_t *>(w + o_r0c);
    bv.revup_cnt = reinterpret_cast<uint32_t *>(w + o_ruc);
    bv.rev0_id = reinterpret_cast<uint32_t *>(w + o_r0i);
    bv.rev0_key = reinterpret_cast<KT *>(w + o_r0k);
    bv.revup_id = reinterpret_cast<uint32_t *>(w + o_rui);
    bv.revup_key = reinterpret_cast<KT *>(w + o_ruk);
    bv.touched = reinterpret_cast<uint32_t *>(w + o_touch);
    bv.n_touched = reinterpret_cast<uint32_t *>(w + o_ntouch);
    bv.cand_id = reinterpret_cast<uint32_t *>(w + o_cid);
    bv.cand_key = reinterpret_cast<KT *>(w + o_ckey);
    bv.cand_cnt = reinterpret_cast<uint32_t *>(w + o_ccnt);
    bv.up_task = reinterpret_cast<uint32_t *>(w + o_uptask);
    bv.ov_code = reinterpret_cast<uint32_t *>(w + o_ovc);
    bv.ov_id = reinterpret_cast<uint32_t *>(w + o_ovi);
    bv.ov_key = reinterpret_cast<KT *>(w + o_ovk);
    bv.ov_cnt = reinterpret_cast<uint32_t *>(w + o_ovn);
    bv.ov_cap = (uint32_t)ov_cap;
    bv.efc = efc;

    // ---- launch geometry
    const KdbWalkLds wl = kdb_walk_lds(PREC == KDB_PREC_I8, idx->ld, efc, idx->n_deleted);
    const size_t lds_prune = prune_lds_bytes<KT>();
    auto ksearch = KDB_WALK_KERNEL(build_search_kernel, wl);
    auto kselect = build_select_kernel<METRIC, PREC>;
    auto krev = build_reverse_kernel<METRIC, PREC>;
    if (lds_prune > 64 * 1024) {
        KDB_HIP(hipFuncSetAttribute((const void *)kselect, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_prune));
        KDB_HIP(hipFuncSetAttribute((const void *)krev, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_prune));
    }
    uint32_t slots_vis = 0;
    rc = walk_pool_prepare(idx, ksearch, wl, s, &slots_vis);
    if (rc) return rc;

    // first node: entry point, no links (:656-670)
    idx->count = count;
    idx->entry = 1;
    idx->max_level = (int)levels[1];
    idx->has_graph = true;
    idx->n_deleted = 0;
    KDB_HIP(hipMemsetAsync(idx->d_deleted, 0, ((((size_t)idx->cap + 1 + 31) / 32 + 3) & ~(size_t)3) * 4, s));
    std::vector<uint32_t> up_task;
    uint32_t next = 2;
    while (next <= count) {
        const uint32_t have = next - 1;
        uint32_t nb = have / 4; // a batch never exceeds a quarter of the graph it searches
        if (nb < 1) nb = 1;
        if (nb > max_batch) nb = max_batch;
        if (nb > count - have) nb = count - have;
        // tasks
        up_task.assign(nb, 0);
        uint32_t nup = 0;
        const int frozen_max = idx->max_level;
        for (uint32_t i = 0; i < nb; i++) {
            up_task[i] = nup;
            int lv = (int)levels[next + i];
            if (lv > frozen_max) lv = frozen_max; // links only up to the current top (:694-697)
            nup += (uint32_t)lv;
        }
        const uint32_t n_tasks = nb + nup;
        if (n_tasks > max_tasks) {
            kdb_set_error("build: task overflow (%u > %zu)", n_tasks, max_tasks);
            return KDB_ERR_STATE;
        }
        bv.first = next;
        bv.nb = nb;
        bv.n_tasks = n_tasks;
        KDB_HIP(hipMemcpyAsync(bv.up_task, up_task.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
        KDB_HIP(hipMemsetAsync(bv.cand_cnt, 0, (size_t)n_tasks * 4, s));
        KDB_HIP(hipMemsetAsync(bv.n_touched, 0, 4, s));
        KDB_HIP(hipMemsetAsync(bv.ov_cnt, 0, 4, s));
        KDB_HIP(hipMemsetAsync(kdb_cur(idx).d_work, 0, 4, s));
        KdbView v = kdb_make_view(idx);
        v.count = next + nb - 1;
        uint32_t grid = slots_vis < nb ? slots_vis : nb;
        hipLaunchKernelGGL(ksearch, dim3(grid), dim3(64), wl.bytes, s, v, bv, wl.beam_cap, wl.nr_cap, kdb_cur(idx).d_visited, kdb_cur(idx).d_work);
        KDB_HIP(hipGetLastError());
        hipLaunchKernelGGL(kselect, dim3(n_tasks), dim3(256), lds_prune, s, v, bv);
        KDB_HIP(hipGetLastError());
        uint32_t n_touched = 0;
        KDB_HIP(hipMemcpyAsync(&n_touched, bv.n_touched, 4, hipMemcpyDeviceToHost, s));
        KDB_HIP(hipStreamSynchronize(s));
        if (n_touched) {
            hipLaunchKernelGGL(krev, dim3(n_touched), dim3(256), lds_prune, s, v, bv, n_touched);
            KDB_HIP(hipGetLastError());
        }
        // phase 4: entry point / maxLevel (:2066-2080)
        for (uint32_t i = 0; i < nb; i++) {
            const int lv = (int)levels[next + i];
            if (lv > idx->max_level) {
                idx->max_level = lv;
                idx->entry = next + i;
            }
        }
        next += nb;
    }
    KDB_HIP(hipStreamSynchronize(s));
    return KDB_OK;
}

// addBatchInternal for rows already in place (phases 1-4), reference linking.  Everything that can fail for want of memory is
// done BEFORE the index is touched; a failure behind that point (a HIP error) rolls the handle back to the state it had.
template <int METRIC, int PREC>
int add_batch_ref_impl(kdb_index *idx, uint32_t first, uint32_t nb, const uint8_t *lv_in, uint32_t efc) {
    using KT = typename BKey<PREC>::T;
    constexpr size_t KB = sizeof(KT);
    hipStream_t s = idx->stream;
    const uint32_t new_count = first + nb - 1u;
    const int frozen_max = idx->max_level;
    const bool reuse = first == idx->count; // the batch's first node takes over the last node's slot (:1620 vs :590)
    // ---- phase 1B bookkeeping: levels (randomLevel's own cap, :2620-2623, against the maxLevel the batch started with) and
    //      upper slots of the new nodes.  A node that takes over a slot gets fresh ones -- as many as the HIGHER of its own level
    //      and the replaced node's: old links still name it at those levels, and the reference grows it when asked (:2049-2053)
    std::vector<uint8_t> lv(nb);
    std::vector<uint32_t> up_new(nb), up_task(nb);
    size_t slots = idx->up_slots;
    uint32_t nup = 0, reuse_levels = 0;
    for (uint32_t i = 0; i < nb; i++) {
        int l = lv_in[i];
        if (l > frozen_max + 1) l = frozen_max + 1;
        lv[i] = (uint8_t)l;
        up_new[i] = (uint32_t)slots;
        uint32_t own = (uint32_t)l;
        if (i == 0 && reuse) {
            const uint32_t old_l = idx->h_levels[first];
            reuse_levels = own > old_l ? own : old_l;
            own = reuse_levels;
        }
        slots += (size_t)own;
        up_task[i] = nup;
        nup += (uint32_t)(l < frozen_max ? l : frozen_max); // links only up to the current top (:1829)
    }
    // ---- workspace, kernels, visited pool: every allocation and attribute call of the call, up front
    const size_t n1 = (size_t)idx->cap + 1;
    const size_t L = n1 + slots + 1;
    const uint32_t n_tasks = nb + nup;
    KdbCarver c;
    const size_t o_ckey = c.take((size_t)n_tasks * efc * KB), o_cid = c.take((size_t)n_tasks * efc * 4), o_ccnt = c.take((size_t)n_tasks * 4);
    const size_t o_uptask = c.take((size_t)nb * 4 + 64), o_cnt = c.take(L * 4), o_off = c.take(L * 4), o_cur = c.take(L * 4);
    const size_t o_owner = c.take((slots + 1) * 4), o_touch = c.take(L * 4), o_out = c.take(256), o_big = c.take(L * 4);
    const size_t req_max = (size_t)n_tasks * efc * 2;
    const size_t o_req = c.take(req_max * 4 + 64);
    // unions too long for LDS (a target named by thousands of the batch's nodes) are sorted in HBM scratch, BIG_WG at a time: a
    // union holds at most maxM0 links + the node's own efc candidates + one reverse request per task
    static const uint32_t ucap_lds = [] {
        const char *e = getenv("KDB_RL_UCAP"); // (tests lower it to push ordinary targets through the HBM path)
        uint32_t u = e ? (uint32_t)atoi(e) : RL_UCAP;
        uint32_t p2 = 64;
        while (p2 < u && p2 < RL_UCAP) p2 <<= 1;
        return p2;
    }();
    uint32_t ucap_big = 64;
    while (ucap_big < idx->deg0 + efc + n_tasks) ucap_big <<= 1;
    constexpr uint32_t BIG_WG = 64;
    const size_t o_bigs = c.take((size_t)BIG_WG * ucap_big * (KB + 8));
    int rc = ensure_build_ws(idx, c.total());
    if (rc) return rc;
    const KdbWalkLds wl = kdb_walk_lds(PREC == KDB_PREC_I8, idx->ld, efc, idx->n_deleted);
    auto ksearch = KDB_WALK_KERNEL(build_search_kernel, wl);
    const size_t lds_big = prune_lds_bytes<KT>() + kdb_score_tail(PREC == KDB_PREC_I8, idx->ld).bytes;
    const size_t lds_commit = lds_big + (size_t)ucap_lds * (KB + 8);
    auto kc = rl_commit_kernel<METRIC, PREC>;
    auto kbig = rl_commit_big_kernel<METRIC, PREC>;
    KDB_HIP(hipFuncSetAttribute((const void *)kc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_commit));
    KDB_HIP(hipFuncSetAttribute((const void *)kbig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_big));
    uint32_t slots_vis = 0;
    rc = walk_pool_prepare(idx, ksearch, wl, s, &slots_vis);
    if (rc) return rc;
    rc = grow_upper_pool(idx, slots, true, s); // (the same lists in a larger pool: nothing `undo` would have to put back)
    if (rc) return rc;
    // ---- from here on the index changes; `undo` puts back what the host side knows (the device lists of a batch that failed
    //      half way may hold some of its links: the nodes behind `count` are simply not part of the graph)
    const uint32_t old_count = idx->count, old_entry = idx->entry;
    const int old_max = idx->max_level;
    const size_t old_slots = idx->up_slots;
    const uint8_t old_reuse_level = reuse ? idx->h_levels[first] : 0;
    const uint32_t old_reuse_up = reuse ? idx->h_up_idx[first] : 0;
    auto undo = [&]() {
        (void)hipStreamSynchronize(s);
        idx->count = old_count;
        idx->entry = old_entry;
        idx->max_level = old_max;
        idx->up_slots = old_slots;
        idx->h_levels.resize((size_t)old_count + 1);
        idx->h_up_idx.resize((size_t)old_count + 1);
        if (reuse) {
            idx->h_levels[first] = old_reuse_level;
            idx->h_up_idx[first] = old_reuse_up;
            (void)hipMemcpy(idx->d_levels + first, &old_reuse_level, 1, hipMemcpyHostToDevice);
            (void)hipMemcpy(idx->d_up_idx + first, &old_reuse_up, 4, hipMemcpyHostToDevice);
        }
        idx->graph_epoch++;
    };
#define KDB_TRY(call)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (call);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            kdb_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__);   \
            undo();                                                                                     \
            return _e == hipErrorOutOfMemory ? KDB_ERR_OOM : KDB_ERR_HIP;                               \
        }                                                                                               \
    } while (0)
    KDB_TRY(hipMemsetAsync(idx->d_adj0 + (size_t)first * idx->deg0, 0, (size_t)nb * idx->deg0 * 4, s)); // empty Connections (:1742)
    KDB_TRY(hipMemcpyAsync(idx->d_levels + first, lv.data(), nb, hipMemcpyHostToDevice, s));
    KDB_TRY(hipMemcpyAsync(idx->d_up_idx + first, up_new.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
    if (reuse && idx->n_deleted) { // a node the batch replaces is a NEW node: Deleted starts false (:1742)
        uint32_t w = 0;
        KDB_TRY(hipMemcpyAsync(&w, idx->d_deleted + (first >> 5), 4, hipMemcpyDeviceToHost, s));
        KDB_TRY(hipStreamSynchronize(s));
        if ((w >> (first & 31u)) & 1u) {
            w &= ~(1u << (first & 31u));
            KDB_TRY(hipMemcpyAsync(idx->d_deleted + (first >> 5), &w, 4, hipMemcpyHostToDevice, s));
            KDB_TRY(hipStreamSynchronize(s));
            idx->n_deleted--;
        }
    }
    idx->h_levels.resize((size_t)new_count + 1);
    idx->h_up_idx.resize((size_t)new_count + 1);
    for (uint32_t i = 0; i < nb; i++) {
        idx->h_levels[first + i] = lv[i];
        idx->h_up_idx[first + i] = up_new[i];
    }
    idx->up_slots = slots;
    idx->count = new_count;
    idx->graph_epoch++;
    unsigned char *w = reinterpret_cast<unsigned char *>(idx->d_build);
    BuildViewT<KT> bv{};
    bv.adj0 = idx->d_adj0;
    bv.adj_up = idx->d_adj_up;
    bv.cand_id = reinterpret_cast<uint32_t *>(w + o_cid);
    bv.cand_key = reinterpret_cast<KT *>(w + o_ckey);
    bv.cand_cnt = reinterpret_cast<uint32_t *>(w + o_ccnt);
    bv.up_task = reinterpret_cast<uint32_t *>(w + o_uptask);
    bv.efc = efc;
    bv.first = first;
    bv.nb = nb;
    bv.n_tasks = n_tasks;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(w + o_cnt), *d_off = reinterpret_cast<uint32_t *>(w + o_off);
    uint32_t *d_cur = reinterpret_cast<uint32_t *>(w + o_cur), *d_owner = reinterpret_cast<uint32_t *>(w + o_owner);
    uint32_t *d_touch = reinterpret_cast<uint32_t *>(w + o_touch), *d_out = reinterpret_cast<uint32_t *>(w + o_out);
    uint32_t *d_req = reinterpret_cast<uint32_t *>(w + o_req), *d_big = reinterpret_cast<uint32_t *>(w + o_big);
    KDB_TRY(hipMemcpyAsync(bv.up_task, up_task.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
    KDB_TRY(hipMemsetAsync(bv.cand_cnt, 0, (size_t)n_tasks * 4, s));
    KDB_TRY(hipMemsetAsync(d_cnt, 0, L * 4, s));
    KDB_TRY(hipMemsetAsync(d_cur, 0, L * 4, s));
    KDB_TRY(hipMemsetAsync(d_out, 0, 256, s)); // [0] requests, [1] touched targets, [2] requests above a node's level, [3] big unions, [4] -, [5] grown level
    KDB_TRY(hipMemsetAsync(kdb_cur(idx).d_work, 0, 4, s));
    // ---- phase 1: every new node searches the graph as it was (entry point / maxLevel frozen, :1796-1801)
    KdbView v = kdb_make_view(idx); // count = new_count: the new ids are valid wherever a walk meets them (the re-used slot)
    hipLaunchKernelGGL(ksearch, dim3(slots_vis < nb ? slots_vis : nb), dim3(64), wl.bytes, s, v, bv, wl.beam_cap, wl.nr_cap, kdb_cur(idx).d_visited, kdb_cur(idx).d_work);
    KDB_TRY(hipGetLastError());
    // ---- phases 2 + 3
    const uint32_t reuse_id = reuse ? first : 0u;
    hipLaunchKernelGGL((rl_count_kernel<KT>), dim3(n_tasks), dim3(256), 0, s, v, bv, (uint32_t)n1, d_cnt, d_owner, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                       (uint32_t *)nullptr, d_out + 2, reuse_id, reuse_levels, d_out + 5);
    hipLaunchKernelGGL(rl_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, (uint32_t)L, d_off, d_touch, d_out);
    hipLaunchKernelGGL((rl_count_kernel<KT>), dim3(n_tasks), dim3(256), 0, s, v, bv, (uint32_t)n1, d_cnt, d_owner, d_cur, d_off, d_req, d_out + 2, reuse_id,
                       reuse_levels, d_out + 5);
    KDB_TRY(hipGetLastError());
    uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    KDB_TRY(hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s));
    KDB_TRY(hipStreamSynchronize(s));
    if (out[0] > req_max) { // (cannot happen: two requests per (task, candidate) at most)
        kdb_set_error("add_batch: request overflow");
        undo();
        return KDB_ERR_STATE;
    }
    if (out[1]) {
        hipLaunchKernelGGL(kc, dim3(out[1]), dim3(256), lds_commit, s, v, idx->d_adj0, idx->d_adj_up, (uint32_t)n1, d_touch, d_cnt, d_off, d_req, d_owner,
                           d_out + 2, ucap_lds, d_big);
        KDB_TRY(hipGetLastError());
        KDB_TRY(hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s));
        KDB_TRY(hipStreamSynchronize(s));
        for (uint32_t b0 = 0; b0 < out[3]; b0 += BIG_WG) { // the unions LDS could not hold
            const uint32_t g = out[3] - b0 < BIG_WG ? out[3] - b0 : BIG_WG;
            hipLaunchKernelGGL(kbig, dim3(g), dim3(256), lds_big, s, v, idx->d_adj0, idx->d_adj_up, (uint32_t)n1, d_big, b0, d_cnt, d_off, d_req, d_owner, ucap_big,
                               w + o_bigs, d_out + 2);
            KDB_TRY(hipGetLastError());
        }
    }
    KDB_TRY(hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s));
    KDB_TRY(hipStreamSynchronize(s));
#undef KDB_TRY
    // the re-used slot was asked for links above its new level: it has grown, as the reference's node does (:2049-2053)
    if (reuse && out[5] > (uint32_t)lv[0]) {
        const uint8_t g8 = (uint8_t)out[5];
        idx->h_levels[first] = g8;
        KDB_HIP(hipMemcpy(idx->d_levels + first, &g8, 1, hipMemcpyHostToDevice));
    }
    // ---- phase 4: entry point / maxLevel (:2066-2080)
    for (uint32_t i = 0; i < nb; i++)
        if ((int)lv[i] > idx->max_level) {
            idx->max_level = (int)lv[i];
            idx->entry = first + i;
        }
    if (out[2] || out[4]) { // (neither can happen: see rl_count_kernel / rl_commit_big_kernel)
        kdb_set_error("add_batch: %u requests above a node's level, %u unions beyond the scratch: skipped", out[2], out[4]);
        return KDB_ERR_STATE;
    }
    return KDB_OK;
}

} // namespace

// d_keys: float keys for float32 / float16 indexes, DOUBLE distances for int8 indexes (the reference's float64)
int kdb_select_probe(kdb_index *idx, uint32_t n_lists, uint32_t stride, const uint32_t *d_ids, const void *d_keys,
                     const uint32_t *d_cnt, uint32_t maxm, uint32_t *d_out_ids, uint32_t *d_out_cnt, hipStream_t s) {
    if (maxm == 0 || maxm > PR_MAXSEL || stride > PR_MAXC) {
        kdb_set_error("select probe: maxm must be 1..%d and lists at most %d long", PR_MAXSEL, PR_MAXC);
        return KDB_ERR_INVALID;
    }
    const KdbView v = kdb_make_view(idx);
    return for_metric_prec(idx, [&](auto M, auto P) -> int {
        using KT = typename BKey<P()>::T;
        auto kern = select_probe_kernel<M(), P()>;
        const size_t lds = prune_lds_bytes<KT>();
        KDB_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(n_lists), dim3(256), lds, s, v, d_ids, reinterpret_cast<const KT *>(d_keys), d_cnt, stride, maxm, d_out_ids, d_out_cnt);
        KDB_HIP(hipGetLastError());
        return KDB_OK;
    });
}

int kdb_build_graph(kdb_index *idx, uint32_t count, const kdb_build_params *p) {
    if (count == 0 || count > idx->cap) {
        kdb_set_error("build: count %u outside 1..%u", count, idx->cap);
        return KDB_ERR_INVALID;
    }
    if (idx->deg0 > PR_MAXSEL) {
        kdb_set_error("build: mMax0 %u exceeds %d", idx->deg0, PR_MAXSEL);
        return KDB_ERR_UNSUPPORTED;
    }
    // kernels of callers' streams may still walk the graph this call is about to overwrite (adjacency arrays, the upper
    // pool it may reallocate): wait for the whole device once
    KDB_HIP(hipDeviceSynchronize());
    // (int8: rows, norms and AbsMax must be in place)
    const int rc = for_metric_prec(idx, [&](auto M, auto P) { return build_impl<M(), P()>(idx, count, p); });
    if (rc != KDB_OK) { // a half-linked graph must not answer searches: the handle is back to "rows without a graph"
        (void)hipStreamSynchronize(idx->stream);
        idx->has_graph = false;
        idx->entry = 0;
        idx->max_level = -1;
        idx->h_levels.clear();
        idx->h_up_idx.clear();
    }
    return rc;
}

// addBatchInternal (hnsw_index.go:1479-2088) for rows ALREADY uploaded at ids first_id .. first_id+n-1, linked exactly as the
// reference links them (see "Reference linking" above).  levels: len(Connections)-1 of every new node as drawn by the caller
// (randomLevel, :2616-2625).  first_id = count+1 appends; first_id = count re-uses the last node's slot, which is what the
// reference's id arithmetic does for the first batch after single Adds (:1620, :590).
int kdb_add_batch_ref(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels, uint32_t ef_construction) {
    const uint32_t efc = ef_construction ? ef_construction : idx->desc.ef_construction;
    if (!idx->has_graph || idx->max_level < 0 || idx->h_levels.size() != (size_t)idx->count + 1) {
        kdb_set_error("add_batch: the index needs a graph to add to (upload or build one: the reference inserts its first efConstruction nodes one by one, hnsw_index.go:1505-1516)");
        return KDB_ERR_STATE;
    }
    if (n == 0) return KDB_OK;
    if (!levels || (first_id != idx->count && first_id != idx->count + 1) || first_id == 0 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("add_batch: ids must start at count (%u, re-using the last slot) or count+1 and stay within capacity %u", idx->count, idx->cap);
        return KDB_ERR_INVALID;
    }
    if (efc < 1 || efc > KDB_MAX_EFC || idx->deg0 > PR_MAXSEL) {
        kdb_set_error("add_batch: ef_construction in 1..%u, mMax0 <= %d", KDB_MAX_EFC, PR_MAXSEL);
        return KDB_ERR_UNSUPPORTED;
    }
    KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read the lists this call rewrites
    return for_metric_prec(idx, [&](auto M, auto P) { return add_batch_ref_impl<M(), P()>(idx, first_id, n, levels, efc); });
}
