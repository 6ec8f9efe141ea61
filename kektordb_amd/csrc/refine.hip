// refine.hip -- graph maintenance on the device for gfx950: Refine and Vacuum.  The walk, selectNeighbors and the host helpers
// are the construction family's (kdb_graph_build.cuh; build.hip describes selectNeighbors on a workgroup).
#include "kdb_graph_build.cuh"
#include <algorithm>
#include <vector>

namespace {

// =====================================================================================================================
// Refine (kdb_index_refine): GraphOptimizer.Refine / computeNewConnections (pkg/core/hnsw/optimizer.go:288-560) for a set of
// nodes against the graph AS THE CALL FOUND IT.  Per selected node x and level l <= level(x):
//   searchLayer(row of x, entry point, ef, l) from the entry point ON level l, no descent (:490); the current neighbours of x
//   that the walk did not return, exist and are not deleted are appended with their node-to-node distance (:497-522); x itself
//   is dropped (:524-536); the rest is sorted -- sort.Slice leaves equal distances undefined, restated as (distance, id), the
//   rule of the reference linking (build.hip) -- and pruned by selectNeighbors (:549).  Links are one-directional.
// Phase 1 of the reference computes every list before phase 2 commits any (:354-461): here the new lists are staged in HBM and
// one kernel copies them into the adjacency after the last node has been searched and selected.  Only the candidate arrays are
// chunked (refine_impl), so the result cannot depend on the chunk size.
// =====================================================================================================================
template <typename KT>
struct RefineViewT {
    const uint32_t *nodes;   // [n_nodes] the selected nodes: live, every id once
    const uint32_t *task_of; // [n_nodes + 1] first task of a node; level l of nodes[i] is task task_of[i] + l
    const uint32_t *owner;   // [n_tasks] index into nodes
    uint32_t *cand_id;       // [chunk tasks * efc] candidates of the chunk in flight
    KT *cand_key;
    uint32_t *cand_cnt;      // [chunk tasks]
    uint32_t *stage_id;      // [n_tasks * mMax0] the new lists, staged until every node is done
    uint32_t *stage_cnt;     // [n_tasks]
    uint32_t efc;
    uint32_t c0, cn;         // the chunk: nodes [c0, c0 + cn)
    uint32_t t0;             // its first task
    uint32_t n_tasks;
};

// one wave per node of the chunk; every level restarts at the entry point with a visited set of its own
template <int METRIC, int BS, int PREC>
__global__ void __launch_bounds__(64)
refine_search_kernel(KdbView v, RefineViewT<typename BKey<PREC>::T> rv, uint32_t beam_cap, uint32_t nr_cap, uint32_t *visited_pool, uint32_t *work) {
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
        if (bi >= rv.cn) break;
        const uint32_t ni = rv.c0 + bi;
        const uint32_t node = rv.nodes[ni];
        const uint32_t t_first = rv.task_of[ni], n_lev = rv.task_of[ni + 1] - t_first;
        WalkBeam<BS, I8> b;
        const float qnorm = walk_start<PREC>(v, s, vis, b, node, lane); // the row as stored: not normalised again
        QCtr ctr{};
        // upper levels first: a layer above 0 un-marks what it marked (VisBitset::end_layer), level 0 starts from a clean set
        for (int l = (int)n_lev - 1; l >= 0; l--) {
            search_layer<PREC, METRIC, 0>(v, s, b, vis, nullptr, v.entry, l, rv.efc, qnorm, ctr, EpKnown());
            const size_t at = (size_t)(t_first - rv.t0 + (uint32_t)l) * rv.efc;
            uint32_t nc;
            if constexpr (I8) nc = b.write_results(rv.efc, rv.cand_id + at, nullptr, false, rv.cand_key + at);
            else nc = b.write_results(rv.efc, rv.cand_id + at, rv.cand_key + at, false);
            if (lane == 0) rv.cand_cnt[t_first - rv.t0 + (uint32_t)l] = nc;
        }
    }
}

// one workgroup per (node, level) of the chunk: candidates + surviving current links -> sorted -> selectNeighbors -> staging
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
refine_select_kernel(KdbView v, RefineViewT<typename BKey<PREC>::T> rv) {
    using KT = typename BKey<PREC>::T;
    constexpr bool I8 = PREC == KDB_PREC_I8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tl = blockIdx.x, task = rv.t0 + tl;
    const uint32_t oi = rv.owner[task], node = rv.nodes[oi], level = task - rv.task_of[oi];
    const uint32_t maxm = level == 0 ? v.deg0 : v.deg_up;
    const uint32_t *adj = adj_of(v.adj0, v.adj_up, v, node, level);
    const uint32_t n = rv.cand_cnt[tl];
    // until select_neighbors_wg runs its tiles are free: the union lives in the row tile, the merge's small arrays in m1
    KT *u_key = reinterpret_cast<KT *>(p.rows);                     // [PR_MAXC]
    uint32_t *u_id = reinterpret_cast<uint32_t *>(u_key + PR_MAXC); // [PR_MAXC]
    float *tq = p.rows + RF_TQ_OFF;                                 // the node's row as the query of the extra distances
    uint32_t *w_cur = reinterpret_cast<uint32_t *>(p.m1);           // [64] the current list
    uint32_t *w_in = w_cur + 64;                                    // [64] 1: the walk returned it
    uint32_t *w_ex = w_cur + 128;                                   // [128] the neighbours to append (64 used)
    float *w_d = reinterpret_cast<float *>(w_cur + 256);            // [64] their keys
    uint32_t *w_lo = w_cur + 320;                                   // [64] int8: low words
    uint32_t &sh_ne = p.misc[2], &sh_self = p.misc[3];
    for (uint32_t i = tid; i < n; i += 256) {
        u_id[i] = rv.cand_id[(size_t)tl * rv.efc + i];
        u_key[i] = rv.cand_key[(size_t)tl * rv.efc + i];
    }
    if (tid < 64) {
        w_cur[tid] = tid < maxm ? adj[tid] : 0u;
        w_in[tid] = 0u;
        w_ex[tid] = 0u;
        w_ex[64 + tid] = 0u;
    }
    if (tid == 0) {
        sh_ne = 0u;
        sh_self = 0u;
    }
    __syncthreads();
    { // "alreadyIn" (:506-513): four threads per current neighbour, a quarter of the candidates each
        const uint32_t nb = w_cur[lane];
        if (nb) {
            bool hit = false;
            for (uint32_t i = tid >> 6; i < n; i += 4) hit = hit || (u_id[i] == nb);
            if (hit) w_in[lane] = 1u;
        }
    }
    __syncthreads();
    if (tid < 64) { // the neighbours to append, in list order: they exist and are not deleted (:516-517)
        const uint32_t nb = w_cur[tid];
        bool keep = nb != 0u && nb <= v.count && !w_in[tid] && !is_deleted(v, nb);
        if (keep) // (a list that names a node twice: the first mention is in the union by the time the second is looked at)
            for (uint32_t j = 0; j < tid; j++)
                if (w_cur[j] == nb) {
                    keep = false;
                    break;
                }
        const unsigned long long mk = __ballot(keep);
        if (keep) w_ex[kdb_mbcnt(mk)] = nb;
        if (tid == 0) sh_ne = (uint32_t)__builtin_popcountll(mk);
    }
    __syncthreads();
    const uint32_t ne = sh_ne;
    if (ne) { // distanceBetweenNodes(x, neighbour) (:518): the node's stored row is the query, 16 lanes per row
        const float qnorm = load_row_as_query<PREC, 256>(v, tq, node, tid);
        __syncthreads();
        if (tid < 64) {
            WaveLds s{};
            s.q = tq;
            s.nb_id = w_ex;
            s.nb_d = w_d;
            s.nb_lo = I8 ? w_lo : nullptr;
            compute_dists<PREC, METRIC, 0>(v, s, ne, qnorm);
            wave_lds_fence();
            if (tid < ne) {
                u_id[n + tid] = w_ex[tid];
                if constexpr (I8) u_key[n + tid] = kdb_i8_key_double(w_d[tid], w_lo[tid]);
                else u_key[n + tid] = w_d[tid];
            }
        }
        __syncthreads();
    }
    // without x itself (:526), ascending by (distance, id): every entry counts the entries before it
    const uint32_t nu = n + ne;
    for (uint32_t i = tid; i < nu; i += 256) {
        const uint32_t id = u_id[i];
        if (id == node) {
            atomicAdd(&sh_self, 1u);
            continue;
        }
        const KT k = u_key[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nu; j++) {
            const uint32_t idj = u_id[j];
            rank += (idj != node && key_before(u_key[j], idj, k, id)) ? 1u : 0u;
        }
        p.c_id[rank] = id;
        p.c_key[rank] = k;
    }
    __syncthreads();
    const uint32_t nv = nu - sh_self; // (from here on the tiles the union lived in are select_neighbors_wg's again)
    select_neighbors_wg<METRIC, PREC>(v, p, nv, maxm);
    const uint32_t nsel = p.misc[0];
    if (tid < nsel) rv.stage_id[(size_t)task * v.deg0 + tid] = p.s_id[tid];
    if (tid == 0) rv.stage_cnt[task] = nsel;
}

// the staged lists replace the stored ones, tails zero-filled; one wave per (node, level).  out[0]: lists whose words changed,
// out[1]: links of the old lists that named a deleted (or no) node
template <typename KT>
__global__ void __launch_bounds__(256)
refine_commit_kernel(KdbView v, RefineViewT<KT> rv, uint32_t *adj0, uint32_t *adj_up, unsigned long long *out) {
    __shared__ uint32_t sh[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < 2) sh[tid] = 0u;
    __syncthreads();
    const uint32_t task = blockIdx.x * 4u + (tid >> 6);
    if (task < rv.n_tasks) {
        const uint32_t oi = rv.owner[task], node = rv.nodes[oi], level = task - rv.task_of[oi];
        const uint32_t maxm = level == 0 ? v.deg0 : v.deg_up;
        uint32_t *adj = adj_of(adj0, adj_up, v, node, level);
        const uint32_t cnt = rv.stage_cnt[task];
        const uint32_t old = lane < maxm ? adj[lane] : 0u;
        const uint32_t nw = lane < cnt ? rv.stage_id[(size_t)task * v.deg0 + lane] : 0u;
        const bool dead = old != 0u && (old > v.count || is_deleted(v, old));
        const bool changed = __ballot(old != nw) != 0ull;
        const uint32_t n_dead = (uint32_t)__builtin_popcountll(__ballot(dead));
        if (lane < maxm) adj[lane] = nw;
        if (lane == 0) {
            if (changed) atomicAdd(&sh[0], 1u);
            if (n_dead) atomicAdd(&sh[1], n_dead);
        }
    }
    __syncthreads();
    if (tid < 2 && sh[tid]) atomicAdd(&out[tid], (unsigned long long)sh[tid]);
}

// nodes: live, unique, 1..count.  Every allocation and attribute call comes first; the adjacency is written by the last kernel only.
template <int METRIC, int PREC>
int refine_impl(kdb_index *idx, const std::vector<uint32_t> &nodes, uint32_t efc, uint32_t chunk_nodes, kdb_refine_stats *out) {
    using KT = typename BKey<PREC>::T;
    constexpr size_t KB = sizeof(KT);
    hipStream_t s = idx->stream;
    const uint32_t nn = (uint32_t)nodes.size();
    std::vector<uint32_t> task_of((size_t)nn + 1), owner;
    owner.reserve((size_t)nn + nn / 8 + 16);
    for (uint32_t i = 0; i < nn; i++) {
        task_of[i] = (uint32_t)owner.size();
        int lv = (int)idx->h_levels[nodes[i]];
        if (lv > idx->max_level) lv = idx->max_level;
        owner.insert(owner.end(), (size_t)lv + 1, i);
    }
    if (owner.size() > 0xfffffff0ull) {
        kdb_set_error("refine: too many (node, level) lists for one call");
        return KDB_ERR_UNSUPPORTED;
    }
    const uint32_t n_tasks = (uint32_t)owner.size();
    task_of[nn] = n_tasks;
    if (chunk_nodes == 0) chunk_nodes = 65536u;
    if (chunk_nodes > nn) chunk_nodes = nn;
    uint32_t chunk_tasks = 0;
    for (uint32_t c0 = 0; c0 < nn; c0 += chunk_nodes) {
        const uint32_t c1 = nn - c0 < chunk_nodes ? nn : c0 + chunk_nodes;
        chunk_tasks = std::max(chunk_tasks, task_of[c1] - task_of[c0]);
    }
    KdbCarver c;
    const size_t o_ckey = c.take((size_t)chunk_tasks * efc * KB), o_cid = c.take((size_t)chunk_tasks * efc * 4), o_ccnt = c.take((size_t)chunk_tasks * 4);
    const size_t o_nodes = c.take((size_t)nn * 4), o_taskof = c.take(((size_t)nn + 1) * 4), o_owner = c.take((size_t)n_tasks * 4);
    const size_t o_stage = c.take((size_t)n_tasks * idx->deg0 * 4), o_scnt = c.take((size_t)n_tasks * 4), o_out = c.take(256);
    int rc = ensure_build_ws(idx, c.total());
    if (rc) return rc;
    const KdbWalkLds wl = kdb_walk_lds(PREC == KDB_PREC_I8, idx->ld, efc, idx->n_deleted);
    const size_t lds_prune = prune_lds_bytes<KT>();
    auto ksearch = KDB_WALK_KERNEL(refine_search_kernel, wl);
    auto kselect = refine_select_kernel<METRIC, PREC>;
    if (lds_prune > 64 * 1024) KDB_HIP(hipFuncSetAttribute((const void *)kselect, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_prune));
    uint32_t slots_vis = 0;
    rc = walk_pool_prepare(idx, ksearch, wl, s, &slots_vis);
    if (rc) return rc;
    unsigned char *w = reinterpret_cast<unsigned char *>(idx->d_build);
    RefineViewT<KT> rv{};
    rv.nodes = reinterpret_cast<uint32_t *>(w + o_nodes);
    rv.task_of = reinterpret_cast<uint32_t *>(w + o_taskof);
    rv.owner = reinterpret_cast<uint32_t *>(w + o_owner);
    rv.cand_id = reinterpret_cast<uint32_t *>(w + o_cid);
    rv.cand_key = reinterpret_cast<KT *>(w + o_ckey);
    rv.cand_cnt = reinterpret_cast<uint32_t *>(w + o_ccnt);
    rv.stage_id = reinterpret_cast<uint32_t *>(w + o_stage);
    rv.stage_cnt = reinterpret_cast<uint32_t *>(w + o_scnt);
    rv.efc = efc;
    rv.n_tasks = n_tasks;
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(w + o_out);
    KDB_HIP(hipMemcpyAsync(w + o_nodes, nodes.data(), (size_t)nn * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(w + o_taskof, task_of.data(), ((size_t)nn + 1) * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(w + o_owner, owner.data(), (size_t)n_tasks * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemsetAsync(d_out, 0, 256, s));
    const KdbView v = kdb_make_view(idx);
    // ---- every node searches and selects against the graph as it is: nothing below writes an adjacency word ...
    for (uint32_t c0 = 0; c0 < nn; c0 += chunk_nodes) {
        rv.c0 = c0;
        rv.cn = nn - c0 < chunk_nodes ? nn - c0 : chunk_nodes;
        rv.t0 = task_of[c0];
        const uint32_t ct = task_of[c0 + rv.cn] - rv.t0;
        KDB_HIP(hipMemsetAsync(rv.cand_cnt, 0, (size_t)ct * 4, s));
        KDB_HIP(hipMemsetAsync(kdb_cur(idx).d_work, 0, 4, s));
        hipLaunchKernelGGL(ksearch, dim3(slots_vis < rv.cn ? slots_vis : rv.cn), dim3(64), wl.bytes, s, v, rv, wl.beam_cap, wl.nr_cap, kdb_cur(idx).d_visited, kdb_cur(idx).d_work);
        KDB_HIP(hipGetLastError());
        hipLaunchKernelGGL(kselect, dim3(ct), dim3(256), lds_prune, s, v, rv);
        KDB_HIP(hipGetLastError());
    }
    KDB_HIP(hipStreamSynchronize(s)); // (a fault of a walk shows here, before the graph is touched)
    // ---- ... and one kernel commits
    hipLaunchKernelGGL((refine_commit_kernel<KT>), dim3((n_tasks + 3u) / 4u), dim3(256), 0, s, v, rv, idx->d_adj0, idx->d_adj_up, d_out);
    KDB_HIP(hipGetLastError());
    unsigned long long h_out[2] = {0, 0};
    KDB_HIP(hipMemcpyAsync(h_out, d_out, 16, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    out->nodes_refined = nn;
    out->lists_written = n_tasks;
    out->lists_changed = h_out[0];
    out->dead_links_dropped = h_out[1];
    return KDB_OK;
}

// =====================================================================================================================
// Vacuum (kdb_index_vacuum, kdb_index_dead_link_scan): GraphOptimizer.Vacuum (pkg/core/hnsw/optimizer.go:133-277).  The
// census (:165-193) and the physical cleanup (:256-273) are the two kernels below; the repair (:200-221, reconnectNode
// :565-674) is refine_impl over the census' nodes, the entry point (:232-250) is elected on the host (kdb_vacuum_graph).
// =====================================================================================================================
// The census: one wave per word of the flag bitmap = 32 consecutive ids, so every word has one writer and the result is a
// bitmap, not a list appended to in arrival order.  A lane takes one adjacency word; groups of `1 << lg` lanes (the first power
// of two that holds deg0, at least 16) share a node, 64 >> lg nodes per pass, and the ballot of the pass is folded into the
// nodes' bits.  Dead link = a non-zero word that names no node (nb - 1 >= count) or a deleted one; the zero words behind a list's
// end are padding.  Deleted nodes are skipped: their lists are cleared, not repaired.  Levels above max_level are not looked
// at -- refine_impl does not write them either.  out[0] += the dead links of the live nodes.
__global__ void __launch_bounds__(256)
vacuum_scan_kernel(KdbView v, uint32_t up_slots, uint32_t lg, uint32_t *flags, unsigned long long *out) {
    __shared__ uint32_t sh_dead;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid == 0) sh_dead = 0u;
    __syncthreads();
    const uint32_t w = blockIdx.x * 4u + (tid >> 6);
    uint32_t mine = 0u; // dead links this lane saw
    if (w <= (v.count >> 5)) {
        const uint32_t base = w << 5, last = v.count - base; // base <= count
        uint32_t live = ~v.deleted[w];
        if (w == 0) live &= ~1u;                           // id 0 is no node
        if (last < 31u) live &= (2u << last) - 1u;         // ids above count are no nodes
        uint32_t flag = 0u;
        const uint32_t gs = 1u << lg, sub = lane >> lg, j = lane & (gs - 1u), per = 64u >> lg;
        const unsigned long long gmask = gs == 64u ? ~0ull : (1ull << gs) - 1ull;
        for (uint32_t i = 0; i < 32u; i += per) {
            const uint32_t bit = i + sub;
            uint32_t nb = 0u;
            if (((live >> bit) & 1u) && j < v.deg0) nb = v.adj0[(size_t)(base + bit) * v.deg0 + j];
            const bool dead = nb != 0u && (nb - 1u >= v.count || is_deleted(v, nb));
            const unsigned long long m = __ballot(dead);
            mine += dead ? 1u : 0u;
            for (uint32_t g = 0; g < per; g++)
                if ((m >> (g << lg)) & gmask) flag |= 1u << (i + g);
        }
        // the upper lists of a node are consecutive slots of the pool: levels 1..lv in one run of lv * deg_up words
        uint32_t lv = 0u;
        if (lane < 32u && ((live >> lane) & 1u)) {
            lv = v.levels[base + lane];
            if ((int)lv > v.max_level) lv = (uint32_t)v.max_level;
        }
        unsigned long long up = __ballot(lv > 0u);
        while (up) {
            const int b = __builtin_ctzll(up);
            up &= up - 1ull;
            uint32_t nl = (uint32_t)__shfl((int)lv, b, 64);
            const uint32_t slot = v.up_idx[base + (uint32_t)b];
            if (slot >= up_slots) nl = 0u;
            else if (nl > up_slots - slot) nl = up_slots - slot;
            const uint32_t *lists = v.adj_up + (size_t)slot * v.deg_up;
            uint32_t here = 0u;
            for (uint32_t e = lane; e < nl * v.deg_up; e += 64u) {
                const uint32_t nb = lists[e];
                if (nb != 0u && (nb - 1u >= v.count || is_deleted(v, nb))) here++;
            }
            mine += here;
            if (__ballot(here != 0u)) flag |= 1u << b;
        }
        if (lane == 0) flags[w] = flag;
    }
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&sh_dead, mine);
    __syncthreads();
    if (tid == 0 && sh_dead) atomicAdd(out, (unsigned long long)sh_dead);
}

// The cleanup: one wave per id; a deleted id loses its lists on every level it owns (zero words = empty), its stored row and its
// row of the half-precision ranking copy (rows16 null: there is none) and of the walk planes (walk_hi null: there are none; a zero
// row's planes are zero and its bound is 0).  Its deleted bit stays: that is the mirror's "no node here".
__global__ void __launch_bounds__(256)
vacuum_clear_kernel(KdbView v, uint32_t up_slots, uint32_t *adj0, uint32_t *adj_up, unsigned char *rows, uint32_t row_bytes, uint16_t *rows16, uint32_t ld16,
                    uint16_t *walk_hi, uint16_t *walk_lo, float *walk_err) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t node = blockIdx.x * 4u + (threadIdx.x >> 6) + 1u;
    if (node > v.count) return;
    if (!is_deleted(v, node)) return;
    if (lane < v.deg0) adj0[(size_t)node * v.deg0 + lane] = 0u;
    uint32_t nl = v.levels[node];
    const uint32_t slot = v.up_idx[node];
    if (nl && slot >= up_slots) nl = 0u;
    else if (nl > up_slots - slot) nl = up_slots - slot;
    for (uint32_t e = lane; e < nl * v.deg_up; e += 64u) adj_up[(size_t)slot * v.deg_up + e] = 0u;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    uint4 *r = reinterpret_cast<uint4 *>(rows + (size_t)node * row_bytes); // ld is a multiple of 16 elements: whole 16-byte words
    for (uint32_t i = lane; i < (row_bytes >> 4); i += 64u) r[i] = z;
    if (rows16) {
        uint4 *h = reinterpret_cast<uint4 *>(rows16 + (size_t)node * ld16); // ld16: whole 128-byte slabs
        for (uint32_t i = lane; i < (ld16 >> 3); i += 64u) h[i] = z;
    }
    if (walk_hi) {
        uint4 *h = reinterpret_cast<uint4 *>(walk_hi + (size_t)node * v.ld), *l = reinterpret_cast<uint4 *>(walk_lo + (size_t)node * v.ld);
        for (uint32_t i = lane; i < (v.ld >> 3); i += 64u) h[i] = l[i] = z; // (ld: a multiple of 128 halves)
        if (lane == 0u) walk_err[node] = 0.f;
    }
}

// the census into scratch: flag bitmap ((count >> 5) + 1 words) | one 64-bit counter.  Enqueued on s, not waited for.
int vacuum_scan_launch(kdb_index *idx, hipStream_t s, uint32_t **d_flags, unsigned long long **d_links) {
    const size_t fw = ((size_t)idx->count >> 5) + 1, fb = (fw * 4 + 255) & ~(size_t)255;
    int rc = kdb_ensure_scratch(idx, fb + 256);
    if (rc) return rc;
    *d_flags = reinterpret_cast<uint32_t *>(kdb_cur(idx).d_scratch);
    *d_links = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch) + fb);
    KDB_HIP(hipMemsetAsync(*d_links, 0, 8, s));
    uint32_t lg = 4;
    while ((1u << lg) < idx->deg0) lg++;
    hipLaunchKernelGGL(vacuum_scan_kernel, dim3((uint32_t)((fw + 3) / 4)), dim3(256), 0, s, kdb_make_view(idx), (uint32_t)idx->up_slots, lg, *d_flags, *d_links);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}

// ascending ids of the set bits of a census bitmap
void vacuum_ids_of(const std::vector<uint32_t> &flags, std::vector<uint32_t> &ids) {
    for (size_t w = 0; w < flags.size(); w++)
        for (uint32_t f = flags[w]; f; f &= f - 1u) ids.push_back((uint32_t)(w << 5) + (uint32_t)__builtin_ctz(f));
}

} // namespace

// what Refine and Vacuum's repair share beside refine_limits (nodes: live, unique, 1..count, not empty)
static int refine_dispatch(kdb_index *idx, const std::vector<uint32_t> &nodes, uint32_t efc, uint32_t chunk_nodes, kdb_refine_stats *st) {
    return for_metric_prec(idx, [&](auto M, auto P) { return refine_impl<M(), P()>(idx, nodes, efc, chunk_nodes, st); });
}

// GraphOptimizer.Refine (optimizer.go:288-464) for the nodes `ids` (null: every node 1..count), deleted ones skipped (:341)
int kdb_refine_graph(kdb_index *idx, const uint32_t *ids, uint32_t n, uint32_t ef_construction, uint32_t chunk_nodes, kdb_refine_stats *out) {
    const uint32_t efc = ef_construction ? ef_construction : idx->desc.ef_construction;
    kdb_refine_stats st{};
    if (!idx->has_graph || idx->max_level < 0 || idx->entry == 0 || idx->h_levels.size() != (size_t)idx->count + 1) {
        kdb_set_error("refine: the index holds no graph");
        return KDB_ERR_STATE;
    }
    int rc = refine_limits(idx, efc, "refine");
    if (rc) return rc;
    if (ids)
        for (uint32_t i = 0; i < n; i++)
            if (ids[i] == 0 || ids[i] > idx->count) {
                kdb_set_error("refine: ids[%u] = %u outside 1..%u", i, ids[i], idx->count);
                return KDB_ERR_INVALID;
            }
    KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read the lists this call rewrites
    const size_t dw = ((size_t)idx->count >> 5) + 1;
    std::vector<uint32_t> del(dw, 0u);
    if (idx->n_deleted) KDB_HIP(hipMemcpy(del.data(), idx->d_deleted, dw * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> seen(ids ? dw : 0, 0u), nodes;
    const uint32_t total = ids ? n : idx->count;
    nodes.reserve(total);
    for (uint32_t i = 0; i < total; i++) {
        const uint32_t x = ids ? ids[i] : i + 1u;
        if ((del[x >> 5] >> (x & 31u)) & 1u) continue;
        if (ids) { // a node named twice is refined once: both results would come from the same snapshot
            if ((seen[x >> 5] >> (x & 31u)) & 1u) continue;
            seen[x >> 5] |= 1u << (x & 31u);
        }
        nodes.push_back(x);
    }
    if (!nodes.empty()) rc = refine_dispatch(idx, nodes, efc, chunk_nodes, &st);
    if (rc == KDB_OK && out) *out = st;
    return rc;
}

// the census of Vacuum (optimizer.go:165-193) read back: the deleted bits, the flagged nodes in ascending order, the dead links
static int vacuum_census(kdb_index *idx, std::vector<uint32_t> &del, std::vector<uint32_t> &nodes, uint64_t *n_links, uint64_t *n_dead) {
    hipStream_t s = idx->stream;
    const size_t dw = ((size_t)idx->count >> 5) + 1;
    uint32_t *d_flags = nullptr;
    unsigned long long *d_links = nullptr, links = 0;
    int rc = vacuum_scan_launch(idx, s, &d_flags, &d_links);
    if (rc) return rc;
    std::vector<uint32_t> flags(dw, 0u);
    del.assign(dw, 0u);
    KDB_HIP(hipMemcpyAsync(flags.data(), d_flags, dw * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipMemcpyAsync(&links, d_links, 8, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipMemcpyAsync(del.data(), idx->d_deleted, dw * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    del[0] &= ~1u; // ids 1..count only
    if ((idx->count & 31u) != 31u) del[dw - 1] &= (2u << (idx->count & 31u)) - 1u;
    uint64_t nd = 0;
    for (uint32_t w : del) nd += (uint64_t)__builtin_popcount(w);
    nodes.clear();
    vacuum_ids_of(flags, nodes);
    *n_links = links;
    *n_dead = nd;
    return KDB_OK;
}

static bool vacuum_has_graph(const kdb_index *idx) {
    return idx->has_graph && idx->max_level >= 0 && idx->entry != 0 && idx->count != 0 && idx->h_levels.size() == (size_t)idx->count + 1;
}

// kdb_index_dead_link_scan: the census alone, nothing written
int kdb_dead_link_scan_graph(kdb_index *idx, uint32_t *out_ids, uint32_t cap, uint32_t *n_nodes, uint64_t *n_dead_links, uint64_t *n_dead) {
    std::vector<uint32_t> del, nodes;
    uint64_t links = 0, nd = 0;
    if (vacuum_has_graph(idx)) {
        int rc = vacuum_census(idx, del, nodes, &links, &nd);
        if (rc) return rc;
    }
    if (out_ids)
        for (size_t i = 0; i < nodes.size() && i < cap; i++) out_ids[i] = nodes[i];
    if (n_nodes) *n_nodes = (uint32_t)nodes.size();
    if (n_dead_links) *n_dead_links = links;
    if (n_dead) *n_dead = nd;
    return KDB_OK;
}

// GraphOptimizer.Vacuum (optimizer.go:133-277): census, repair = refine_impl over the census' nodes (snapshot; the reference's
// one-by-one order is not mirrored, see kektor_hip.h), entry point, cleanup.  The census is read-only and its scratch comes
// first; the repair's workspace depends on |R| and is allocated by refine_impl before ITS first launch; from refine_impl's last
// check on (commit, cleanup, host fields) nothing is allocated, and the host fields change after the final synchronisation.
int kdb_vacuum_graph(kdb_index *idx, uint32_t ef_construction, uint32_t flags, uint32_t chunk_nodes, kdb_vacuum_stats *out) {
    const uint32_t efc = ef_construction ? ef_construction : idx->desc.ef_construction;
    kdb_vacuum_stats st{};
    int rc = refine_limits(idx, efc, "vacuum");
    if (rc) return rc;
    if (!vacuum_has_graph(idx) || idx->n_deleted == 0) { // nothing to do (:151): all-zero statistics
        if (out) *out = st;
        return KDB_OK;
    }
    KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read the lists this call rewrites
    std::vector<uint32_t> del, nodes;
    uint64_t links = 0, nd = 0;
    rc = vacuum_census(idx, del, nodes, &links, &nd);
    if (rc) return rc;
    if (nd == 0) {
        if (out) *out = st;
        return KDB_OK;
    }
    st.dead_nodes = nd;
    st.dead_links_found = links;
    st.nodes_repaired = nodes.size();
    // the entry point, from what the host already holds (:232-250): only a deleted entry is replaced
    auto dead = [&](uint32_t x) { return ((del[x >> 5] >> (x & 31u)) & 1u) != 0u; };
    uint32_t entry = idx->entry;
    int32_t max_level = idx->max_level;
    if (dead(entry)) {
        entry = 0;
        max_level = -1;
        for (uint32_t x = 1; x <= idx->count; x++) {
            if (dead(x)) continue;
            const int32_t lv = (int32_t)idx->h_levels[x];
            if (!(flags & KDB_VACUUM_ELECT_TOP_LEVEL)) { // the reference's rule: the first live node it meets, with ITS level
                entry = x;
                max_level = lv;
                break;
            }
            if (lv > max_level) { // the live node of the highest level, the lowest id among equals
                entry = x;
                max_level = lv;
            }
        }
        st.entry_changed = 1;
    }
    if (!nodes.empty()) { // the walks start at the entry point as the call found it, dead or not
        kdb_refine_stats rs{};
        rc = refine_dispatch(idx, nodes, efc, chunk_nodes, &rs);
        if (rc) return rc;
        st.lists_written = rs.lists_written;
        st.lists_changed = rs.lists_changed;
        st.dead_links_dropped = rs.dead_links_dropped;
    }
    hipStream_t s = idx->stream;
    hipLaunchKernelGGL(vacuum_clear_kernel, dim3((idx->count + 3u) / 4u), dim3(256), 0, s, kdb_make_view(idx), (uint32_t)idx->up_slots, idx->d_adj0, idx->d_adj_up,
                       reinterpret_cast<unsigned char *>(idx->d_rows), (uint32_t)((size_t)idx->ld * idx->elem), idx->d_rows16, idx->ld16,
                       idx->d_walk_hi, idx->d_walk_lo, idx->d_walk_err);
    KDB_HIP(hipGetLastError());
    KDB_HIP(hipStreamSynchronize(s));
    idx->entry = entry; // (no live node left: entry 0, max_level -1 -- an index whose graph is empty)
    idx->max_level = max_level;
    st.entry = entry;
    st.max_level = max_level;
    if (out) *out = st;
    return KDB_OK;
}
