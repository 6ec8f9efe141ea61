// add.hip -- the sequential Add on the device for gfx950.  The walk, selectNeighbors and the host helpers are the construction
// family's (kdb_graph_build.cuh; build.hip describes selectNeighbors on a workgroup).
#include "kdb_graph_build.cuh"
#include "kdb_add_plan.h"
#include <vector>

namespace {

// =====================================================================================================================
// Add (kdb_index_add): the sequential single insert (pkg/core/hnsw/hnsw_index.go:472-809), one node after another.  Node i+1 must
// see node i's links, so the inserts are a CHAIN -- kept on the stream, not on the host: two launches per (node, level), their
// arguments (capped level, the entry point and maxLevel the node finds) known up front from kdb_add_plan.h.
//   add_link_kernel     one workgroup: wave 0 walks (on the node's first linked level the ef = 1 descent first, :685-690; on the
//                       levels below, the entry point is the previous level's nearest candidate, left in the state block), the
//                       workgroup runs selectNeighbors, writes x's list (:711-722) and leaves the selection in the state block;
//   add_reverse_kernel  maxM workgroups, one per possible selected neighbour r (:725-783): each owns r's list at that level, so
//                       no two write the same list; appends x, or prunes [live links in stored order, x].
// No workgroup waits for another; what orders the steps is the stream.  Every loop is bounded by ef, maxM or the list capacity.
// State block (device words): 0 ep | 1 its distance is known | 2 key | 3 key, low word (int8) | 4 a walk of this node tied |
// 5 selected count | 8.. selected ids.  Counters (64-bit): 0 appended | 1 pruned | 2 tied nodes | 3 skipped (level below l).
// =====================================================================================================================
constexpr uint32_t AD_SEL = 8; // first selected id in the state block
constexpr uint32_t AD_STATE_WORDS = AD_SEL + PR_MAXSEL;

template <typename KT>
__host__ __device__ constexpr size_t add_prune_bytes() { return (prune_lds_bytes<KT>() + 15) & ~(size_t)15; }

// from_level: the maxLevel the node found when `level` is its first linked level (the descent starts there), -1 on the levels below
template <int METRIC, int BS, int PREC>
__global__ void __launch_bounds__(256)
add_link_kernel(KdbView v, uint32_t *adj0, uint32_t *adj_up, uint32_t node, int level, int from_level, uint32_t entry, uint32_t efc, uint32_t beam_cap,
                uint32_t nr_cap, uint32_t *visited, uint32_t *st, unsigned long long *ctr) {
    using KT = typename BKey<PREC>::T;
    constexpr bool I8 = PREC == KDB_PREC_I8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = uni(tid >> 6); // (scalar: the walk below is one wave's, behind a scalar branch)
    if (wave == 0u) {
        WaveLds s;
        VisBitset vis;
        walk_carve<BS, I8>(smem + add_prune_bytes<KT>(), v, beam_cap, nr_cap, visited, s, vis);
        const int lane = kdb_lane();
        const bool first = from_level >= level;
        WalkBeam<BS, I8> b;
        // (the levels below the first find the visited set clean: a layer above 0 un-marks what it marked)
        const float qnorm = walk_start<PREC>(v, s, vis, b, node, lane, first);
        QCtr qc{};
        uint32_t ep = entry;
        EpKnown epk;
        if (first) {
            for (int l = from_level; l > level; l--) { // zoom in, :685-690
                search_layer<PREC, METRIC, 0>(v, s, b, vis, nullptr, ep, l, 1u, qnorm, qc, epk);
                walk_nearest(b, ep, epk);
            }
        } else {
            ep = uni(st[0]);
            epk.known = uni(st[1]) != 0u;
            epk.key = unif(__uint_as_float(st[2]));
            epk.lo = uni(st[3]);
            b.tied = uni(st[4]);
        }
        uint32_t nc = 0;
        if (ep - 1u < v.count) { // (never an address from an id that names no node)
            search_layer<PREC, METRIC, 0>(v, s, b, vis, nullptr, ep, level, efc, qnorm, qc, epk);
            if constexpr (I8) nc = b.write_results(efc, p.c_id, nullptr, false, p.c_key);
            else nc = b.write_results(efc, p.c_id, p.c_key, false);
            walk_nearest(b, ep, epk);
        }
        if (lane == 0) {
            p.misc[6] = nc;
            st[0] = ep;
            st[1] = epk.known ? 1u : 0u;
            st[2] = __float_as_uint(epk.key);
            st[3] = epk.lo;
            st[4] = b.tied;
            if (level == 0 && b.tied) atomicAdd(ctr + 2, 1ull); // level 0 is a node's last walk
        }
    }
    __syncthreads();
    const uint32_t n = p.misc[6];
    const uint32_t maxm = level == 0 ? v.deg0 : v.deg_up;
    select_neighbors_wg<METRIC, PREC>(v, p, n, maxm);
    const uint32_t nsel = p.misc[0];
    uint32_t *adj = adj_of(adj0, adj_up, v, node, (uint32_t)level);
    if (tid < maxm) adj[tid] = tid < nsel ? p.s_id[tid] : 0u;
    if (tid < (uint32_t)PR_MAXSEL) st[AD_SEL + tid] = tid < nsel ? p.s_id[tid] : 0u;
    if (tid == 0) st[5] = nsel;
}

// workgroup b: the b-th selected neighbour of `node` at `level`
template <int METRIC, int PREC>
__global__ void __launch_bounds__(256)
add_reverse_kernel(KdbView v, uint32_t *adj0, uint32_t *adj_up, uint32_t node, uint32_t level, const uint32_t *st, unsigned long long *ctr) {
    using KT = typename BKey<PREC>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PruneLdsT<KT> p;
    prune_carve(smem, p);
    const ScoreLds sl = score_carve<PREC == KDB_PREC_I8>(smem + add_prune_bytes<KT>(), v); // r's row as the query of the node-to-node distances
    __shared__ uint32_t sh[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t maxm = level == 0 ? v.deg0 : v.deg_up;
    uint32_t nsel = st[5];
    if (nsel > maxm) nsel = maxm;
    if (blockIdx.x >= nsel) return;
    const uint32_t r = st[AD_SEL + blockIdx.x];
    if (r - 1u >= v.count || r == node) return;                // never an address from an id that names no node
    if (is_deleted(v, r)) return;                              // "neighbor == nil || Deleted: continue" (a walk never returns one)
    if (level > 0u && (uint32_t)v.levels[r] < level) {         // the reference grows r (:775-779): not mirrored, counted
        if (tid == 0) atomicAdd(ctr + 3, 1ull);
        return;
    }
    uint32_t *adj = adj_of(adj0, adj_up, v, r, level);
    if (tid < 64u) { // the list as stored; its live links, in that order (:756-761)
        const uint32_t w = tid < maxm ? adj[tid] : 0u;
        const unsigned long long holes = ~__ballot(w != 0u);
        const uint32_t ne = holes ? (uint32_t)__builtin_ctzll(holes) : 64u; // packed from the front: the first zero word ends it
        const bool live = tid < ne && w - 1u < v.count && w != node && !is_deleted(v, w);
        const unsigned long long lm = __ballot(live);
        if (live) p.c_id[kdb_mbcnt(lm)] = w;
        if (tid == 0) {
            sh[0] = ne;
            sh[1] = (uint32_t)__builtin_popcountll(lm);
        }
    }
    __syncthreads();
    const uint32_t ne = sh[0];
    if (ne < maxm) { // room: x at the end (:748-752)
        if (tid == 0) {
            adj[ne] = node;
            atomicAdd(ctr + 0, 1ull);
        }
        return;
    }
    const uint32_t na = sh[1] + 1u; // live links, then x (:762)
    if (tid == 0) p.c_id[na - 1u] = node;
    const float qnorm = load_row_as_query<PREC, 256>(v, sl.tq, r, tid);
    __syncthreads();
    score_ids_wg<METRIC, PREC>(v, sl, qnorm, p.c_id, na, p.c_key);
    __syncthreads();
    select_neighbors_wg<METRIC, PREC>(v, p, na, maxm); // NOT sorted first: the stored order is the order given
    const uint32_t ns2 = p.misc[0];
    if (tid < maxm) adj[tid] = tid < ns2 ? p.s_id[tid] : 0u;
    if (tid == 0) atomicAdd(ctr + 1, 1ull);
}

} // namespace

// Add for rows already in place.  Everything that can fail for want of memory comes before the first launch; the host side of the
// handle (level tables, slot count, count, entry point, maxLevel) changes after the final synchronisation succeeded.
template <int METRIC, int PREC>
static int add_impl(kdb_index *idx, uint32_t first, uint32_t nb, const uint8_t *lv_in, uint32_t efc, kdb_add_stats *out) {
    using KT = typename BKey<PREC>::T;
    hipStream_t s = idx->stream;
    const uint32_t new_count = first + nb - 1u;
    const bool bare = idx->h_levels.size() != (size_t)idx->count + 1; // rows without a graph: nodes of level 0 without links
    // ---- the plan: capped levels, the entry point and maxLevel every node finds (kdb_add_plan.h), upper slots
    std::vector<KdbAddStep> steps(nb);
    uint32_t entry = idx->has_graph ? idx->entry : 0u;
    int32_t max_level = idx->has_graph ? idx->max_level : -1;
    kdb_add_plan(&entry, &max_level, first, lv_in, nb, steps.data());
    std::vector<uint8_t> lv(nb);
    std::vector<uint32_t> up_new(nb);
    size_t slots = bare ? 0 : idx->up_slots;
    for (uint32_t i = 0; i < nb; i++) {
        lv[i] = steps[i].level;
        up_new[i] = (uint32_t)slots;
        slots += (size_t)lv[i];
    }
    // ---- LDS of the two kernels against the device's limit, before anything is allocated or touched
    const KdbWalkLds wl = kdb_walk_lds(PREC == KDB_PREC_I8, idx->ld, efc, idx->n_deleted);
    const size_t lds_link = add_prune_bytes<KT>() + wl.bytes;
    const size_t lds_rev = add_prune_bytes<KT>() + kdb_score_tail(PREC == KDB_PREC_I8, idx->ld).bytes;
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, idx->device) != hipSuccess || lds_max <= 0) lds_max = 64 * 1024;
    if (lds_link > (size_t)lds_max || lds_rev > (size_t)lds_max) {
        kdb_set_error("add: rows of %u elements with ef_construction %u and %u deleted nodes need %zu bytes of LDS per workgroup, the device has %d",
                      idx->ld, efc, idx->n_deleted, lds_link > lds_rev ? lds_link : lds_rev, lds_max);
        return KDB_ERR_UNSUPPORTED;
    }
    // ---- workspace, kernels, visited set: every allocation and attribute call of the call, up front
    const size_t ws_bytes = 256 + (size_t)AD_STATE_WORDS * 4;
    int rc = ensure_build_ws(idx, ws_bytes);
    if (rc) return rc;
    unsigned long long *d_ctr = reinterpret_cast<unsigned long long *>(idx->d_build);
    uint32_t *d_st = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(idx->d_build) + 256);
    auto klink = KDB_WALK_KERNEL(add_link_kernel, wl);
    auto krev = add_reverse_kernel<METRIC, PREC>;
    KDB_HIP(hipFuncSetAttribute((const void *)klink, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_link));
    KDB_HIP(hipFuncSetAttribute((const void *)krev, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rev));
    rc = kdb_ensure_visited(idx, 1u, s); // one bitset for the call: the walks are a chain
    if (rc) return rc;
    rc = grow_upper_pool(idx, slots, !bare, s);
    if (rc) return rc;
    // ---- the new nodes on the device, as kdb_index_append_nodes registers them: empty lists, levels, first upper slots
    if (bare && idx->count) {
        KDB_HIP(hipMemsetAsync(idx->d_adj0, 0, ((size_t)idx->count + 1) * idx->deg0 * 4, s));
        KDB_HIP(hipMemsetAsync(idx->d_levels, 0, (size_t)idx->count + 1, s));
        KDB_HIP(hipMemsetAsync(idx->d_up_idx, 0, ((size_t)idx->count + 1) * 4, s));
    }
    KDB_HIP(hipMemsetAsync(idx->d_adj0 + (size_t)first * idx->deg0, 0, (size_t)nb * idx->deg0 * 4, s));
    KDB_HIP(hipMemcpyAsync(idx->d_levels + first, lv.data(), nb, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(idx->d_up_idx + first, up_new.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemsetAsync(idx->d_build, 0, ws_bytes, s));
    KdbView v = kdb_make_view(idx);
    v.count = new_count; // the new ids are valid wherever a later node's walk meets them
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    // the derived upper-slot table is a function of levels / up_idx / the upper lists: nodes that only exist at level 0 change
    // none of its inputs (kdb_index_append_nodes' rule), so the first search after such an insert pays no rebuild
    if (slots != (bare ? 0 : idx->up_slots) || bare) idx->graph_epoch++;
    // ---- the chain; an error behind the first launch waits for what is queued before it returns
    auto chain = [&]() -> int {
    for (uint32_t i = 0; i < nb; i++) {
        const KdbAddStep &st = steps[i];
        if (st.max_level < 0) continue; // the first node of an empty graph: entry point, no links (:657-670)
        const int top = (int)st.level < st.max_level ? (int)st.level : st.max_level; // links only up to the current top (:694-697)
        for (int l = top; l >= 0; l--) {
            hipLaunchKernelGGL(klink, dim3(1), dim3(256), lds_link, s, v, idx->d_adj0, idx->d_adj_up, first + i, l, l == top ? st.max_level : -1, st.entry, efc,
                               wl.beam_cap, wl.nr_cap, kdb_cur(idx).d_visited, d_st, d_ctr);
            hipLaunchKernelGGL(krev, dim3(l == 0 ? idx->deg0 : idx->deg_up), dim3(256), lds_rev, s, v, idx->d_adj0, idx->d_adj_up, first + i, (uint32_t)l,
                               (const uint32_t *)d_st, d_ctr);
        }
        KDB_HIP(hipGetLastError());
    }
    KDB_HIP(hipMemcpyAsync(h_ctr, d_ctr, 32, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    return KDB_OK;
    };
    rc = chain();
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    // ---- the host side of the handle
    if (bare) {
        idx->h_levels.assign((size_t)idx->count + 1, 0);
        idx->h_up_idx.assign((size_t)idx->count + 1, 0);
    }
    idx->h_levels.insert(idx->h_levels.end(), lv.begin(), lv.end());
    idx->h_up_idx.insert(idx->h_up_idx.end(), up_new.begin(), up_new.end());
    idx->up_slots = slots;
    idx->count = new_count;
    idx->entry = entry;
    idx->max_level = max_level;
    idx->has_graph = true;
    if (out) {
        out->nodes_added = nb;
        out->forward_lists = kdb_add_plan_lists(steps.data(), nb);
        out->reverse_appended = h_ctr[0];
        out->reverse_pruned = h_ctr[1];
        out->tied_nodes = h_ctr[2];
        out->reverse_skipped = h_ctr[3];
        out->entry = entry;
        out->max_level = max_level;
    }
    return KDB_OK;
}

// Add (hnsw_index.go:472-809) for rows ALREADY uploaded at ids first_id .. first_id+n-1: see kektor_hip.h
int kdb_add_graph(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels, uint32_t ef_construction, kdb_add_stats *out) {
    const uint32_t efc = ef_construction ? ef_construction : idx->desc.ef_construction;
    if (n == 0) {
        if (out) {
            *out = kdb_add_stats{};
            out->entry = idx->entry;
            out->max_level = idx->max_level;
        }
        return KDB_OK;
    }
    if (!levels || first_id != idx->count + 1 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("add: ids must continue at count+1 = %u and stay within capacity %u, levels must be given", idx->count + 1, idx->cap);
        return KDB_ERR_INVALID;
    }
    int rc = refine_limits(idx, efc, "add");
    if (rc) return rc;
    if (idx->has_graph && idx->max_level >= 0 && idx->h_levels.size() != (size_t)idx->count + 1) {
        kdb_set_error("add: the index holds a graph without its host-side level table");
        return KDB_ERR_STATE;
    }
    KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read the lists this call rewrites
    return for_metric_prec(idx, [&](auto M, auto P) { return add_impl<M(), P()>(idx, first_id, n, levels, efc, out); });
}
