// kdb_api_query.hip -- host side of the C ABI (include/kektor_hip.h): the query entry points -- graph search, exact scan, distances,
// by-id, decode, consensus, belief -- each as a _dev call on the caller's stream and as a host-pointer call (kdb_api_calls.hip).
#include "kdb_internal.h"
#include "kdb_host.h"
#include <string.h>

// ---------------------------------------------------------------------------------------------
// Search
// ---------------------------------------------------------------------------------------------
static size_t qrow_bytes(const kdb_index *idx) {
    return idx->desc.precision == KDB_PREC_I8 ? ((size_t)idx->ld + 15) / 16 * 16 : (size_t)idx->ld * 4;
}

// prepared queries live in kdb_cur(idx).d_qbuf: [Bpad rows][qrow_bytes] then qnorm [Bpad]
int kdb_prepare_queries(kdb_index *idx, const KdbView &v, const float *d_queries, uint32_t B, uint32_t Bpad,
                        uint32_t flags, void **d_q, float **d_qnorm, hipStream_t s) {
    const size_t qb = qrow_bytes(idx);
    KdbCarver cv;
    const size_t o_q = cv.take((size_t)Bpad * qb), o_qnorm = cv.take((size_t)Bpad * 4);
    int rc = kdb_ensure_qbuf(idx, cv.total() + 256);
    if (rc) return rc;
    *d_q = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_qbuf) + o_q;
    *d_qnorm = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(kdb_cur(idx).d_qbuf) + o_qnorm);
    if (Bpad > B) KDB_HIP(hipMemsetAsync(reinterpret_cast<unsigned char *>(kdb_cur(idx).d_qbuf) + (size_t)B * qb, 0, (size_t)(Bpad - B) * qb, s));
    return kdb_launch_prep_queries(v, d_queries, B, *d_q, *d_qnorm, (flags & KDB_SEARCH_PREPARED) ? 0 : 1, s);
}

static uint32_t effective_ef(uint32_t ef, uint32_t flags) { // (max(ef, k) is the launchers': they know k)
    return kdb_mixed_effective_ef(ef, 0u, (flags & KDB_SEARCH_NEEDS_REFINE) != 0u); // hnsw_index.go:387-399
}

int kdb_search_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                          const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist,
                          uint32_t *d_out_count, hipStream_t s, const MultiLists *ml, const KdbDone *done,
                          const MixedKeys *mx) {
    KdbView v = kdb_make_view(idx);
    if (B == 0) return KDB_OK;
    if (k == 0) {
        kdb_set_error("search: k must be >= 1");
        return KDB_ERR_INVALID;
    }
    if (idx->max_level < 0 || idx->count == 0) { // empty index returns [] (hnsw_index.go:383-385)
        KDB_HIP(hipMemsetAsync(d_out_count, 0, (size_t)B * 4, s));
        KDB_HIP(hipMemsetAsync(d_out_ids, 0, (size_t)B * k * 4, s));
        if (done) { // (combined callers watch their completion words: publish them behind the zeros, from the host)
            KDB_HIP(hipStreamSynchronize(s));
            for (uint32_t b = 0; b < B; b++) __atomic_store_n(done->flags + b, done->gen, __ATOMIC_RELEASE);
        }
        return KDB_OK;
    }
    if (!idx->has_graph) {
        kdb_set_error("search: no graph uploaded or built");
        return KDB_ERR_STATE;
    }
    uint32_t entry = idx->entry;
    {
        int rc = kdb_ensure_up_slots(idx, s); // (a host compare unless the graph changed since the last search)
        if (rc) return rc;
        v.adj_up_slot = idx->d_adj_up_slot;
    }
    const uint32_t *d_allow = reinterpret_cast<const uint32_t *>(d_allow_bits);
    KdbMultiAllow ma;
    if (done) {
        ma.done_flags = done->flags;
        ma.done_gen = done->gen;
        ma.sess_ctl = done->sess_ctl;
        ma.sess_gen = done->sess_gen;
        ma.sess_grid = done->sess_grid;
    }
    if (ml && ml->G) { // one entry point per list, chosen on the device: no host round trip for any of the G lists
        int rc = kdb_ensure_group_entries(idx, ml->G);
        if (rc) return rc;
        rc = kdb_launch_group_entries(v, d_allow, ml->G, (uint32_t)(ml->words64 * 2), entry, kdb_cur(idx).d_gentry, s);
        if (rc) return rc;
        ma.of_query = ml->d_of_query;
        ma.group_entry = kdb_cur(idx).d_gentry;
        ma.words32 = (uint32_t)(ml->words64 * 2);
    } else if (d_allow) { // Smart Entry Point Selection (hnsw_index.go:437-447), decided on the device: an empty bitmap,
        // or one whose smallest id names no vector while the entry point is not allowed, yields no results
        const uint32_t words32 = 2u * ((idx->count >> 6) + 1u);
        int rc = kdb_ensure_group_entries(idx, 1);
        if (rc) return rc;
        rc = kdb_launch_group_entries(v, d_allow, 1, words32, entry, kdb_cur(idx).d_gentry, s);
        if (rc) return rc;
        ma.group_entry = kdb_cur(idx).d_gentry; // of_query stays null: every query uses list 0
        ma.words32 = words32;
    }
    // float32 / float16 indexes: the search kernel prepares each query itself while it loads it into LDS (normalise for
    // cosine, f16 round trip) straight from the caller's buffer; int8 needs the quantised copy + the query norms
    const void *d_q = d_queries;
    float *d_qnorm = nullptr;
    uint32_t raw = 1u | ((idx->desc.metric == KDB_METRIC_COSINE && !(flags & KDB_SEARCH_PREPARED)) ? 2u : 0u);
    int rc = KDB_OK;
    if (idx->desc.precision == KDB_PREC_I8) {
        void *d_qp = nullptr;
        rc = kdb_prepare_queries(idx, v, d_queries, B, B, flags, &d_qp, &d_qnorm, s);
        if (rc) return rc;
        d_q = d_qp;
        raw = (flags & KDB_SEARCH_DIST_F64) ? 4u : 0u; // bit 2: d_out_dist is a double array
    } else if (flags & KDB_SEARCH_DIST_F64) {
        kdb_set_error("search: KDB_SEARCH_DIST_F64 applies to int8 indexes (the other precisions compute float32 distances)");
        return KDB_ERR_INVALID;
    }
    if (flags & KDB_SEARCH_TIE_FLAG) raw |= 8u;    // bit 31 of out_count: the walk met equal distances
    if (flags & KDB_SEARCH_HEAP_ORDER) raw |= 16u; // ... and such queries are re-walked in the reference's heap order
    uint32_t ef_launch = effective_ef(ef, flags);
    if (mx) { // every query's own k and ef: the kernels apply the boost and max(ef, k) per query (bit 6 of raw: the boost)
        ma.k_of_query = mx->d_k;
        ma.ef_of_query = mx->d_ef;
        ef_launch = mx->ef_cap;
        if (flags & KDB_SEARCH_NEEDS_REFINE) raw |= 64u;
    }
    uint32_t *tr_nd = nullptr, *tr_nh = nullptr;
    if (idx->trace_ndist && idx->trace_on_device) {
        tr_nd = idx->trace_ndist;
        tr_nh = idx->trace_nhops;
    } else if (idx->trace_ndist) {
        rc = kdb_ensure_scratch(idx, (size_t)B * 8 + 64);
        if (rc) return rc;
        tr_nd = reinterpret_cast<uint32_t *>(kdb_cur(idx).d_scratch);
        tr_nh = tr_nd + B;
    }
    rc = kdb_launch_search(idx, v, d_q, d_qnorm, raw, B, k, ef_launch, d_allow, ma, entry, d_out_ids, d_out_dist,
                           d_out_count, tr_nd, tr_nh, s);
    if (rc) return rc;
    if (idx->trace_ndist && !idx->trace_on_device) {
        KDB_HIP(hipMemcpyAsync(idx->trace_ndist, tr_nd, (size_t)B * 4, hipMemcpyDeviceToHost, s));
        if (idx->trace_nhops) KDB_HIP(hipMemcpyAsync(idx->trace_nhops, tr_nh, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    }
    return KDB_OK;
}

extern "C" int kdb_search_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                                    const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids,
                                    float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B && (!d_queries || !d_out_ids || !d_out_dist || !d_out_count)) {
        kdb_set_error("search: null buffer");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    return kdb_search_dev_locked(idx, d_queries, B, k, ef, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, call.s);
}

extern "C" int kdb_search_batch_multi_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                                          const uint64_t *d_allow_lists, uint32_t G, uint64_t words_per_list,
                                          const uint32_t *d_allow_of_query, uint32_t flags, uint32_t *d_out_ids,
                                          float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!d_queries || !d_out_ids || !d_out_dist || !d_out_count || k == 0) {
        kdb_set_error("search_multi: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    if (flags & KDB_SEARCH_DIST_F64) {
        kdb_set_error("search_multi: KDB_SEARCH_DIST_F64 is an option of kdb_search_batch[_dev] and kdb_flat_scan_batch[_dev]");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    if (G == 0 || !d_allow_lists || !d_allow_of_query) // no lists: the plain batch
        return kdb_search_dev_locked(idx, d_queries, B, k, ef, nullptr, flags, d_out_ids, d_out_dist, d_out_count, s);
    if (words_per_list < ((uint64_t)(idx->count >> 6) + 1)) {
        kdb_set_error("search_multi: words_per_list %llu < (count>>6)+1 = %llu", (unsigned long long)words_per_list,
                      (unsigned long long)(idx->count >> 6) + 1);
        return KDB_ERR_INVALID;
    }
    MultiLists ml;
    ml.G = G;
    ml.words64 = words_per_list;
    ml.d_of_query = d_allow_of_query;
    return kdb_search_dev_locked(idx, d_queries, B, k, ef, d_allow_lists, flags, d_out_ids, d_out_dist, d_out_count, s, &ml);
}

extern "C" int kdb_search_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef,
                                const uint64_t *allow_bits, uint32_t flags, uint32_t *out_ids, float *out_dist,
                                uint32_t *out_count) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!queries || !out_ids || !out_dist || !out_count || k == 0) {
        kdb_set_error("search: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    static const uint32_t chunk_min = [] { const char *e = getenv("KDB_HOST_CHUNK_MIN"); return e ? (uint32_t)atoi(e) : 8192u; }();
    const bool traced = idx->trace_ndist != nullptr; // (set by the caller's own thread before the call: kdb_search_set_trace)
    if (B >= chunk_min && chunk_min > 0 && !traced && !(flags & KDB_SEARCH_FAIL_ON_DROP)) {
        uint32_t chunk = ((B + 3u) / 4u + 255u) & ~255u; // four chunks, not below 4096 queries each
        if (chunk < 4096u) chunk = 4096u;
        return kdb_search_staged_chunks(idx, queries, B, k, ef, allow_bits, flags, out_ids, out_dist, out_count, chunk);
    }
    const size_t dist_bytes = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    auto run = [&](float *d_q, uint64_t *d_allow, uint32_t *d_ids, float *d_dist, uint32_t *d_cnt, hipStream_t s, uint32_t nq, const uint32_t *, const uint32_t *) {
        return kdb_search_dev_locked(idx, d_q, nq, k, ef, d_allow, flags, d_ids, d_dist, d_cnt, s);
    };
    if (traced || (flags & KDB_SEARCH_FAIL_ON_DROP) || !kdb_fits_a_slot(idx, B, k, allow_bits != nullptr, dist_bytes))
        return staged_big_call(idx, queries, B, k, allow_bits, out_ids, out_dist, out_count, dist_bytes, (flags & KDB_SEARCH_FAIL_ON_DROP) != 0, run);
    static const uint32_t combine_max_b = [] { const char *e = getenv("KDB_COMBINE_MAX_B"); return e ? (uint32_t)atoi(e) : 16u; }();
    if (!allow_bits && B <= combine_max_b && B <= KDB_GROUP_CAP) return kdb_combined_search_call(idx, queries, B, k, ef, flags, out_ids, out_dist, out_count);
    return staged_slot_call(idx, queries, B, k, allow_bits, out_ids, out_dist, out_count, dist_bytes, true, run);
}

// ---- mixed batches: every query its own k and efSearch, one launch (kdb_mixed_plan.h) ---------------------------------------
// Host pointers.  Validated here, before anything is staged; the launch's capacity comes from the arrays; k and ef travel beside the
// queries (StagedLayout::o_keys).  Routes: a slot, or a turn on the index's staging buffer when the call is traced, asks for
// KDB_SEARCH_FAIL_ON_DROP or does not fit a slot -- ONE launch either way: a large batch is not cut into chunks (chunks of a
// mixed batch would each need the capacity of the whole), and a small one does not join other callers' launches.
extern "C" int kdb_search_batch_mixed(kdb_index *idx, const float *queries, uint32_t B, const uint32_t *k, const uint32_t *ef, uint32_t k_stride,
                                      const uint64_t *allow_bits, uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!queries || !k || !ef || !out_ids || !out_dist || !out_count || k_stride == 0) {
        kdb_set_error("search_mixed: null buffer or k_stride == 0");
        return KDB_ERR_INVALID;
    }
    const bool refine = (flags & KDB_SEARCH_NEEDS_REFINE) != 0u;
    uint32_t eff_max = 0;
    bool distinct = false;
    for (uint32_t b = 0; b < B; b++) {
        if (!kdb_mixed_query_valid(k[b], 0u, k_stride, 0u)) {
            kdb_set_error("search_mixed: k[%u] = %u is outside 1..k_stride (%u)", b, k[b], k_stride);
            return KDB_ERR_INVALID;
        }
        const uint32_t e = kdb_mixed_effective_ef(ef[b], k[b], refine);
        if (e > eff_max) eff_max = e;
        if (k[b] != k[0] || e != kdb_mixed_effective_ef(ef[0], k[0], refine)) distinct = true;
    }
    MixedKeys mx;
    mx.ef_cap = kdb_mixed_ef_cap(eff_max);
    KDB_HIP(hipSetDevice(idx->device));
    const size_t dist_bytes = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    const HostKeys hk{k, ef};
    auto run = [&](float *d_q, uint64_t *d_allow, uint32_t *d_ids, float *d_dist, uint32_t *d_cnt, hipStream_t s, uint32_t nq, const uint32_t *d_k,
                   const uint32_t *d_ef) {
        MixedKeys m = mx;
        m.d_k = d_k;
        m.d_ef = d_ef;
        const int rc = kdb_search_dev_locked(idx, d_q, nq, k_stride, 0u, d_allow, flags, d_ids, d_dist, d_cnt, s, nullptr, nullptr, &m);
        if (rc == KDB_OK && distinct && idx->has_graph && idx->count) { // (under idx->mu, as every enqueue)
            idx->n_mixed_launches++;
            idx->n_mixed_calls++;
        }
        return rc;
    };
    const bool traced = idx->trace_ndist != nullptr; // (set by the caller's own thread before the call: kdb_search_set_trace)
    if (traced || (flags & KDB_SEARCH_FAIL_ON_DROP) || !kdb_fits_a_slot(idx, B, k_stride, allow_bits != nullptr, dist_bytes, true))
        return staged_big_call(idx, queries, B, k_stride, allow_bits, out_ids, out_dist, out_count, dist_bytes, (flags & KDB_SEARCH_FAIL_ON_DROP) != 0, run, &hk);
    return staged_slot_call(idx, queries, B, k_stride, allow_bits, out_ids, out_dist, out_count, dist_bytes, true, run, &hk);
}

// Device pointers: the arrays cannot be read here, so the caller states the largest effective ef it sends; the kernels refuse the
// queries that break the launch's bounds (KDB_MIXED_BAD_QUERY).  Per-query allow lists as kdb_search_batch_multi_dev has them.
extern "C" int kdb_search_batch_mixed_dev(kdb_index *idx, const float *d_queries, uint32_t B, const uint32_t *d_k, const uint32_t *d_ef, uint32_t k_stride,
                                          uint32_t ef_max, const uint64_t *d_allow_lists, uint32_t G, uint64_t words_per_list,
                                          const uint32_t *d_allow_of_query, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count,
                                          void *stream) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!d_queries || !d_k || !d_ef || !d_out_ids || !d_out_dist || !d_out_count || k_stride == 0 || ef_max == 0) {
        kdb_set_error("search_mixed: null buffer, k_stride == 0 or ef_max == 0");
        return KDB_ERR_INVALID;
    }
    if (G != 0 && (!d_allow_lists || !d_allow_of_query)) {
        kdb_set_error("search_mixed: G = %u lists without d_allow_lists / d_allow_of_query", G);
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    MixedKeys mx;
    mx.d_k = d_k;
    mx.d_ef = d_ef;
    mx.ef_cap = kdb_mixed_ef_cap(ef_max);
    if (G == 0) return kdb_search_dev_locked(idx, d_queries, B, k_stride, 0u, d_allow_lists, flags, d_out_ids, d_out_dist, d_out_count, call.s, nullptr, nullptr, &mx);
    if (words_per_list < ((uint64_t)(idx->count >> 6) + 1)) {
        kdb_set_error("search_mixed: words_per_list %llu < (count>>6)+1 = %llu", (unsigned long long)words_per_list,
                      (unsigned long long)(idx->count >> 6) + 1);
        return KDB_ERR_INVALID;
    }
    MultiLists ml;
    ml.G = G;
    ml.words64 = words_per_list;
    ml.d_of_query = d_allow_of_query;
    return kdb_search_dev_locked(idx, d_queries, B, k_stride, 0u, d_allow_lists, flags, d_out_ids, d_out_dist, d_out_count, call.s, &ml, nullptr, &mx);
}

int kdb_flat_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, const uint64_t *d_allow_bits,
                        uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, hipStream_t s) {
    KdbView v = kdb_make_view(idx);
    if (B == 0) return KDB_OK;
    if (idx->count == 0) {
        KDB_HIP(hipMemsetAsync(d_out_count, 0, (size_t)B * 4, s));
        KDB_HIP(hipMemsetAsync(d_out_ids, 0, (size_t)B * k * 4, s));
        return KDB_OK;
    }
    const uint32_t *d_allow = reinterpret_cast<const uint32_t *>(d_allow_bits);
    const uint32_t *d_first = nullptr;
    if (d_allow) { // allowList.IsEmpty() => no filter (vector_index.go:130): decided on the device, no host round trip
        int rc = kdb_launch_first_allowed(d_allow, 2 * ((idx->count >> 6) + 1), kdb_cur(idx).d_work + 8, s);
        if (rc) return rc;
        d_first = kdb_cur(idx).d_work + 8;
    }
    const uint32_t Bpad = (B + 255u) & ~255u; // whole query tiles of either tile kernel (128 / 256 queries), zero rows behind B
    void *d_q = nullptr;
    float *d_qnorm = nullptr;
    int rc = kdb_ensure_rows16(idx, s);
    if (rc) return rc;
    rc = kdb_prepare_queries(idx, v, d_queries, B, Bpad, flags, &d_q, &d_qnorm, s);
    if (rc) return rc;
    if ((flags & KDB_SEARCH_DIST_F64) && idx->desc.precision != KDB_PREC_I8) {
        kdb_set_error("flat scan: KDB_SEARCH_DIST_F64 applies to int8 indexes (the other precisions compute float32 distances)");
        return KDB_ERR_INVALID;
    }
    rc = kdb_launch_flat_scan(idx, v, d_q, d_qnorm, B, k, d_allow, d_first, d_out_ids, d_out_dist, d_out_count,
                              ((flags & KDB_SEARCH_PREPARED) ? 0 : 1) | ((flags & KDB_SEARCH_DIST_F64) ? 2 : 0), s);
    if (rc) return rc;
    // a query that is not finite once prepared gets no results, as from a walk (include/kektor_hip.h, "Conventions")
    return kdb_launch_void_dead_queries(d_qnorm, B, k, d_out_ids, d_out_dist, d_out_count, (flags & KDB_SEARCH_DIST_F64) != 0, s);
}

extern "C" int kdb_flat_scan_groups_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t G,
                                        const uint32_t *group_offsets, const uint64_t *d_allow_lists,
                                        uint64_t words_per_list, uint64_t max_total_allowed, uint32_t flags,
                                        uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!d_queries || !d_out_ids || !d_out_dist || !d_out_count || !group_offsets || !d_allow_lists || G == 0) {
        kdb_set_error("flat_scan_groups: null buffer or no group");
        return KDB_ERR_INVALID;
    }
    if (flags & KDB_SEARCH_DIST_F64) {
        kdb_set_error("flat_scan_groups: KDB_SEARCH_DIST_F64 is an option of kdb_search_batch[_dev] and kdb_flat_scan_batch[_dev]");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    if (words_per_list < ((uint64_t)(idx->count >> 6) + 1)) {
        kdb_set_error("flat_scan_groups: words_per_list %llu < (count>>6)+1", (unsigned long long)words_per_list);
        return KDB_ERR_INVALID;
    }
    KdbView v = kdb_make_view(idx);
    if (idx->count == 0) {
        KDB_HIP(hipMemsetAsync(d_out_count, 0, (size_t)B * 4, s));
        KDB_HIP(hipMemsetAsync(d_out_ids, 0, (size_t)B * k * 4, s));
        return KDB_OK;
    }
    const uint32_t Bpad = (B + 127u) & ~127u;
    void *d_q = nullptr;
    float *d_qnorm = nullptr;
    int rc = kdb_ensure_rows16(idx, s);
    if (rc) return rc;
    rc = kdb_prepare_queries(idx, v, d_queries, B, Bpad, flags, &d_q, &d_qnorm, s);
    if (rc) return rc;
    rc = kdb_launch_flat_scan_groups(idx, v, d_q, d_qnorm, B, k, G, group_offsets,
                                     reinterpret_cast<const uint32_t *>(d_allow_lists), (uint32_t)(words_per_list * 2),
                                     max_total_allowed, d_out_ids, d_out_dist, d_out_count,
                                     (flags & KDB_SEARCH_PREPARED) ? 0 : 1, s);
    if (rc) return rc;
    return kdb_launch_void_dead_queries(d_qnorm, B, k, d_out_ids, d_out_dist, d_out_count, false, s);
}

extern "C" int kdb_flat_scan_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k,
                                       const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids,
                                       float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B && (!d_queries || !d_out_ids || !d_out_dist || !d_out_count)) {
        kdb_set_error("flat_scan: null buffer");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    return kdb_flat_dev_locked(idx, d_queries, B, k, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, call.s);
}

extern "C" int kdb_flat_scan_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k,
                                   const uint64_t *allow_bits, uint32_t flags, uint32_t *out_ids, float *out_dist,
                                   uint32_t *out_count) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!queries || !out_ids || !out_dist || !out_count || k == 0) {
        kdb_set_error("flat_scan: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    const size_t dist_bytes = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    auto run = [&](float *d_q, uint64_t *d_allow, uint32_t *d_ids, float *d_dist, uint32_t *d_cnt, hipStream_t s, uint32_t nq, const uint32_t *, const uint32_t *) {
        return kdb_flat_dev_locked(idx, d_q, nq, k, d_allow, flags, d_ids, d_dist, d_cnt, s);
    };
    if (!kdb_fits_a_slot(idx, B, k, allow_bits != nullptr, dist_bytes)) return staged_big_call(idx, queries, B, k, allow_bits, out_ids, out_dist, out_count, dist_bytes, false, run);
    return staged_slot_call(idx, queries, B, k, allow_bits, out_ids, out_dist, out_count, dist_bytes, false, run);
}

static int distance_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, const uint32_t *d_ids, uint32_t C,
                               uint32_t flags, float *d_out, hipStream_t s) {
    KdbView v = kdb_make_view(idx);
    void *d_q = nullptr;
    float *d_qnorm = nullptr;
    int rc = kdb_prepare_queries(idx, v, d_queries, B, B, flags, &d_q, &d_qnorm, s);
    if (rc) return rc;
    (void)kdb_stats_begin(idx, 3, B, C);
    KDB_HIP(hipEventRecord(idx->ev0, s));
    rc = kdb_launch_distance(v, d_q, d_qnorm, B, d_ids, C, d_out, s);
    if (rc) return rc;
    KDB_HIP(hipEventRecord(idx->ev1, s));
    return KDB_OK;
}

extern "C" int kdb_distance_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, const uint32_t *d_ids,
                                      uint32_t C, uint32_t flags, float *d_out, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B == 0 || C == 0) return KDB_OK;
    if (!d_queries || !d_ids || !d_out) {
        kdb_set_error("distance_batch: null buffer");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    return distance_dev_locked(idx, d_queries, B, d_ids, C, flags, d_out, call.s);
}

extern "C" int kdb_distance_batch(kdb_index *idx, const float *queries, uint32_t B, const uint32_t *ids, uint32_t C,
                                  uint32_t flags, float *out) {
    KDB_CHECK_IDX(idx);
    if (B == 0 || C == 0) return KDB_OK;
    if (!queries || !ids || !out) {
        kdb_set_error("distance_batch: null buffer");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion q, cand, res;
    KdbTurnOpt opt;
    opt.slack = 256;
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            q = st.in(queries, (size_t)B * idx->desc.dim * 4);
            cand = st.in(ids, (size_t)B * C * 4);
            res = st.out(out, (size_t)B * C * 4);
            return KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) { return distance_dev_locked(idx, q.at<float>(d), B, cand.at<uint32_t>(d), C, flags, res.at<float>(d), s); });
}

// ---------------------------------------------------------------------------------------------
// Stored rows as queries (by_id.hip): the Gardener's "more like this" loop (pkg/cognitive/gardener.go:803-869 pages ids, reads
// their vectors with VGetMany and searches with each) without the rows leaving HBM.  A COMPOSITION: the source rows are decoded to
// float32 -- the vector GetNodeData returns (hnsw_index.go:2909-2959) -- into a buffer of the call's scratch lane that neither the
// walk nor the scan uses (d_byid), then kdb_search_dev_locked / kdb_flat_dev_locked run unchanged on that buffer, query prep included.
// ---------------------------------------------------------------------------------------------
static int by_id_dev_locked(kdb_index *idx, bool flat, const uint32_t *d_ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *d_allow_bits,
                            uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, hipStream_t s) {
    const char *who = flat ? "flat_scan_by_id" : "search_by_id";
    if (B == 0) return KDB_OK;
    if (k == 0) {
        kdb_set_error("%s: k must be >= 1", who);
        return KDB_ERR_INVALID;
    }
    if (flags & KDB_SEARCH_PREPARED) {
        kdb_set_error("%s: KDB_SEARCH_PREPARED is not accepted (a decoded row goes through the normal query prep, as GetNodeData's vector does in the reference)", who);
        return KDB_ERR_INVALID;
    }
    const bool drop = (flags & KDB_BY_ID_DROP_SELF) != 0;
    const uint32_t inner = flags & ~(uint32_t)KDB_BY_ID_DROP_SELF;
    if (drop && (k == 0xffffffffu || (flat && k + 1u > KDB_FLAT_MAX_K))) {
        kdb_set_error("%s: KDB_BY_ID_DROP_SELF runs the call with k + 1 = %llu, above the limit of %u", who, (unsigned long long)k + 1u, flat ? KDB_FLAT_MAX_K : 0xffffffffu);
        return KDB_ERR_INVALID;
    }
    if ((flags & KDB_SEARCH_DIST_F64) && idx->desc.precision != KDB_PREC_I8) {
        kdb_set_error("%s: KDB_SEARCH_DIST_F64 applies to int8 indexes (the other precisions compute float32 distances)", who);
        return KDB_ERR_INVALID;
    }
    const uint32_t kin = drop ? k + 1u : k;
    const size_t db = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    KdbCarver cv; // decoded rows | found flags | with drop: the inner call's k + 1 answers
    const size_t o_q = cv.take((size_t)B * idx->desc.dim * 4), o_found = cv.take(B), o_ids = cv.take(drop ? (size_t)B * kin * 4 : 0),
                 o_dist = cv.take(drop ? (size_t)B * kin * db : 0), o_cnt = cv.take(drop ? (size_t)B * 4 : 0);
    int rc = kdb_ensure_byid(idx, cv.total());
    if (rc) return rc;
    unsigned char *const p = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_byid);
    float *const d_q = reinterpret_cast<float *>(p + o_q);
    uint8_t *const d_found = p + o_found;
    uint32_t *const i_ids = drop ? reinterpret_cast<uint32_t *>(p + o_ids) : d_out_ids;
    float *const i_dist = drop ? reinterpret_cast<float *>(p + o_dist) : d_out_dist;
    uint32_t *const i_cnt = drop ? reinterpret_cast<uint32_t *>(p + o_cnt) : d_out_count;
    // A source that is not found (id 0, above count, deleted) must get no results.  Graph search: its decoded row is a quiet NaN in
    // every column, and the documented guarantee for queries that are not finite (kektor_hip.h, "Conventions") does the rest -- no
    // results, a zeroed id row, no walk, no counter touched, the other queries answered bit for bit as alone.  The exact scan still
    // scans such a query before it voids the answer: there the row is zeros (an ordinary query) and the epilogue kernel discards it.
    const KdbView v = kdb_make_view(idx);
    rc = kdb_launch_decode_rows(v, d_ids, B, d_q, d_found, flat ? 0u : 0x7fc00000u, s);
    if (rc) return rc;
    rc = flat ? kdb_flat_dev_locked(idx, d_q, B, kin, d_allow_bits, inner, i_ids, i_dist, i_cnt, s)
              : kdb_search_dev_locked(idx, d_q, B, kin, ef, d_allow_bits, inner, i_ids, i_dist, i_cnt, s);
    if (rc) return rc;
    if (flat || drop)
        rc = kdb_launch_by_id_finish(d_ids, d_found, B, k, kin, (uint32_t)(db / 4), i_ids, i_dist, i_cnt, d_out_ids, d_out_dist, d_out_count, s);
    return rc;
}

static int by_id_dev_call(kdb_index *idx, bool flat, const uint32_t *d_ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *d_allow_bits,
                          uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    if (B && (!d_ids || !d_out_ids || !d_out_dist || !d_out_count)) {
        kdb_set_error("%s: null buffer", flat ? "flat_scan_by_id" : "search_by_id");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    return by_id_dev_locked(idx, flat, d_ids, B, k, ef, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, call.s);
}

extern "C" int kdb_search_by_id_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *d_allow_bits,
                                    uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream) {
    return by_id_dev_call(idx, false, d_ids, B, k, ef, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, stream);
}
extern "C" int kdb_flat_scan_by_id_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t B, uint32_t k, const uint64_t *d_allow_bits, uint32_t flags,
                                       uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream) {
    return by_id_dev_call(idx, true, d_ids, B, k, 0, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, stream);
}

// Host pointers: a turn on the staging buffer (HostTurn).  What crosses the bus: 4 bytes per query in, the answers out.  Never part
// of a combined group (the ids are not queries a group's kernel could read).
static int by_id_host_call(kdb_index *idx, bool flat, const uint32_t *ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                           uint32_t flags, uint32_t *out_ids, void *out_dist, uint32_t *out_count) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!ids || !out_ids || !out_dist || !out_count || k == 0) {
        kdb_set_error("%s: null buffer or k == 0", flat ? "flat_scan_by_id" : "search_by_id");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    const size_t db = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    KdbRegion src, allow, r_ids, r_dist, r_cnt;
    KdbTurnOpt opt;
    opt.drop_who = !flat && (flags & KDB_SEARCH_FAIL_ON_DROP) ? "search_by_id" : nullptr;
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            src = st.in(ids, (size_t)B * 4);
            allow = st.in(allow_bits, kdb_bits_bytes(idx->count));
            r_ids = st.out(out_ids, (size_t)B * k * 4);
            r_dist = st.out(out_dist, (size_t)B * k * db);
            r_cnt = st.out(out_count, (size_t)B * 4);
            return KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return by_id_dev_locked(idx, flat, src.at<uint32_t>(d), B, k, ef, allow.at<uint64_t>(d), flags & ~(uint32_t)KDB_SEARCH_FAIL_ON_DROP, r_ids.at<uint32_t>(d),
                                    r_dist.at<float>(d), r_cnt.at<uint32_t>(d), s);
        });
}

extern "C" int kdb_search_by_id(kdb_index *idx, const uint32_t *ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits, uint32_t flags,
                                uint32_t *out_ids, float *out_dist, uint32_t *out_count) {
    return by_id_host_call(idx, false, ids, B, k, ef, allow_bits, flags, out_ids, out_dist, out_count);
}
extern "C" int kdb_flat_scan_by_id(kdb_index *idx, const uint32_t *ids, uint32_t B, uint32_t k, const uint64_t *allow_bits, uint32_t flags,
                                   uint32_t *out_ids, float *out_dist, uint32_t *out_count) {
    return by_id_host_call(idx, true, ids, B, k, 0, allow_bits, flags, out_ids, out_dist, out_count);
}

// GetNodeData(...).Vector / the vectors of VGetMany for n ids (by_id.hip).  Reads only: ordered like a search.
extern "C" int kdb_index_decode_rows_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t n, float *d_out, uint8_t *d_out_found, void *stream) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!d_ids || !d_out) {
        kdb_set_error("decode_rows: null buffer");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    return kdb_launch_decode_rows(kdb_make_view(idx), d_ids, n, d_out, d_out_found, 0u, call.s);
}

extern "C" int kdb_index_decode_rows(kdb_index *idx, const uint32_t *ids, uint32_t n, float *out, uint8_t *out_found) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!ids || !out) {
        kdb_set_error("decode_rows: null buffer");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    HostTurn turn(idx);
    // in pieces of at most 64 MiB of vectors (VGetMany pages 500 ids; a caller that asks for a million rows must not make the
    // staging buffer as large as the index)
    const size_t row_b = (size_t)idx->desc.dim * 4;
    size_t per = ((size_t)64 << 20) / row_b;
    if (per < 1) per = 1;
    if (per > n) per = n;
    KdbStage st; // (the layout only: every piece is copied in and out by the loop below)
    const KdbRegion r_ids = st.dev(per * 4), r_rows = st.dev(per * row_b), r_found = st.dev(per);
    unsigned char *const d = turn.stage(st.total());
    if (!d) return turn.rc;
    uint32_t *const d_ids = r_ids.at<uint32_t>(d);
    float *const d_rows = r_rows.at<float>(d);
    uint8_t *const d_found = r_found.at<uint8_t>(d);
    hipStream_t s = idx->stream;
    const KdbView v = kdb_make_view(idx); // (the call is counted: writers stay out, count, rows and deleted bits cannot move)
    turn.lk.unlock();
    int rc;
    for (size_t i0 = 0; i0 < n; i0 += per) {
        const uint32_t m = (uint32_t)(n - i0 < per ? n - i0 : per);
        KDB_HIP(hipMemcpyAsync(d_ids, ids + i0, (size_t)m * 4, hipMemcpyHostToDevice, s));
        rc = kdb_launch_decode_rows(v, d_ids, m, d_rows, d_found, 0u, s);
        if (rc) return rc;
        KDB_HIP(hipMemcpyAsync(out + i0 * idx->desc.dim, d_rows, (size_t)m * row_b, hipMemcpyDeviceToHost, s));
        if (out_found) KDB_HIP(hipMemcpyAsync(out_found + i0, d_found, m, hipMemcpyDeviceToHost, s));
    }
    KDB_HIP(hipStreamSynchronize(s));
    return KDB_OK;
}

// ---------------------------------------------------------------------------------------------
// CalculateConsensus for id lists (consensus.hip) and VBeliefState's search + consensus as one call.  The consensus kernel reads
// the lists, the rows and the queries where they are and needs no scratch; kdb_belief_batch is a COMPOSITION like the by-id calls:
// kdb_search_dev_locked unchanged, then the kernel on its answers.
// ---------------------------------------------------------------------------------------------
static int consensus_check(const char *who, uint32_t B, uint32_t stride, uint32_t flags, const void *ids, const void *queries, const void *out,
                           const void *out_similarity) {
    if (stride > KDB_CONSENSUS_MAX_K) {
        kdb_set_error("%s: %u entries per list, above KDB_CONSENSUS_MAX_K (%u)", who, stride, KDB_CONSENSUS_MAX_K);
        return KDB_ERR_INVALID;
    }
    if (flags) {
        kdb_set_error("%s: flags must be 0", who);
        return KDB_ERR_INVALID;
    }
    if (!queries && out_similarity) {
        kdb_set_error("%s: out_similarity needs the queries", who);
        return KDB_ERR_INVALID;
    }
    if (B && ((!ids && stride) || !out)) {
        kdb_set_error("%s: null buffer", who);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}

extern "C" int kdb_consensus_batch_dev(kdb_index *idx, const uint32_t *d_ids, const uint32_t *d_counts, uint32_t B, uint32_t stride,
                                       const float *d_queries, const uint64_t *d_active_bits, uint32_t flags, kdb_consensus *d_out,
                                       double *d_out_similarity, float *d_out_centroid, double *d_out_gram, void *stream) {
    KDB_CHECK_IDX(idx);
    int rc = consensus_check("consensus", B, stride, flags, d_ids, d_queries, d_out, d_out_similarity);
    if (rc) return rc;
    if (B == 0) return KDB_OK;
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    return kdb_launch_consensus(kdb_make_view(idx), d_ids, d_counts, B, stride, d_queries, reinterpret_cast<const uint32_t *>(d_active_bits), d_out,
                                d_out_similarity, d_out_centroid, d_out_gram, call.s);
}

extern "C" int kdb_consensus_batch(kdb_index *idx, const uint32_t *ids, const uint32_t *counts, uint32_t B, uint32_t stride, const float *queries,
                                   const uint64_t *active_bits, uint32_t flags, kdb_consensus *out, double *out_similarity, float *out_centroid,
                                   double *out_gram) {
    KDB_CHECK_IDX(idx);
    int rc = consensus_check("consensus", B, stride, flags, ids, queries, out, out_similarity);
    if (rc) return rc;
    if (counts)
        for (uint32_t b = 0; b < B; b++)
            if ((counts[b] & KDB_COUNT_MASK) > stride) {
                kdb_set_error("consensus: list %u has %u entries, more than the stride %u", b, counts[b] & KDB_COUNT_MASK, stride);
                return KDB_ERR_INVALID;
            }
    if (B == 0) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    const size_t dim = idx->desc.dim, gw = (size_t)stride + 1;
    KdbRegion r_ids, r_cnt, r_q, r_act, r_out, r_sim, r_cen, r_gram;
    KdbView v;
    KdbTurnOpt opt;
    opt.lane = false; // the kernel reads the lists, the rows and the queries where they are: no scratch, launched outside idx->mu
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) { // (stride == 0: the lists and the similarities are empty regions -- null to the kernel, which reads and writes none of them)
            r_ids = st.in(ids, (size_t)B * stride * 4);
            r_cnt = st.in(counts, (size_t)B * 4);
            r_q = st.in(queries, (size_t)B * dim * 4);
            r_act = st.in(active_bits, kdb_bits_bytes(idx->count));
            r_out = st.out(out, (size_t)B * sizeof(kdb_consensus));
            r_sim = st.out(out_similarity, (size_t)B * stride * 8);
            r_cen = st.out(out_centroid, (size_t)B * dim * 4);
            r_gram = st.out(out_gram, (size_t)B * gw * gw * 8);
            v = kdb_make_view(idx); // (once staged the call is counted: writers stay out, count, rows and deleted bits cannot move)
            return KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return kdb_launch_consensus(v, r_ids.at<uint32_t>(d), r_cnt.at<uint32_t>(d), B, stride, r_q.at<float>(d), r_act.at<uint32_t>(d), r_out.at<kdb_consensus>(d),
                                        r_sim.at<double>(d), r_cen.at<float>(d), r_gram.at<double>(d), s);
        });
}

static int belief_check(uint32_t B, uint32_t k, uint32_t flags, const void *queries, const void *out_ids, const void *out_dist, const void *out_count,
                        const void *out) {
    if (k == 0 || k > KDB_CONSENSUS_MAX_K) {
        kdb_set_error("belief: k = %u outside 1..KDB_CONSENSUS_MAX_K (%u)", k, KDB_CONSENSUS_MAX_K);
        return KDB_ERR_INVALID;
    }
    if (flags & KDB_SEARCH_PREPARED) {
        kdb_set_error("belief: KDB_SEARCH_PREPARED is not accepted (the similarities are defined on the raw query, epistemic.go:81)");
        return KDB_ERR_INVALID;
    }
    if (B && (!queries || !out_ids || !out_dist || !out_count || !out)) {
        kdb_set_error("belief: null buffer");
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}

static int belief_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *d_allow_bits,
                             const uint64_t *d_active_bits, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count,
                             kdb_consensus *d_out, double *d_out_similarity, hipStream_t s) {
    int rc = kdb_search_dev_locked(idx, d_queries, B, k, ef, d_allow_bits, flags, d_out_ids, d_out_dist, d_out_count, s);
    if (rc) return rc;
    return kdb_launch_consensus(kdb_make_view(idx), d_out_ids, d_out_count, B, k, d_queries, reinterpret_cast<const uint32_t *>(d_active_bits), d_out,
                                d_out_similarity, nullptr, nullptr, s);
}

extern "C" int kdb_belief_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *d_allow_bits,
                                    const uint64_t *d_active_bits, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count,
                                    kdb_consensus *d_out, double *d_out_similarity, void *stream) {
    KDB_CHECK_IDX(idx);
    int rc = belief_check(B, k, flags, d_queries, d_out_ids, d_out_dist, d_out_count, d_out);
    if (rc) return rc;
    if (B == 0) return KDB_OK;
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    return belief_dev_locked(idx, d_queries, B, k, ef, d_allow_bits, d_active_bits, flags, d_out_ids, d_out_dist, d_out_count, d_out, d_out_similarity,
                             call.s);
}

extern "C" int kdb_belief_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                                const uint64_t *active_bits, uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count, kdb_consensus *out,
                                double *out_similarity) {
    KDB_CHECK_IDX(idx);
    int rc = belief_check(B, k, flags, queries, out_ids, out_dist, out_count, out);
    if (rc) return rc;
    if (B == 0) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    const size_t db = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    KdbRegion q, allow, act, r_ids, r_dist, r_cnt, r_out, r_sim;
    KdbTurnOpt opt;
    opt.drop_who = (flags & KDB_SEARCH_FAIL_ON_DROP) ? "belief" : nullptr;
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            q = st.in(queries, (size_t)B * idx->desc.dim * 4);
            allow = st.in(allow_bits, kdb_bits_bytes(idx->count));
            act = st.in(active_bits, kdb_bits_bytes(idx->count));
            r_ids = st.out(out_ids, (size_t)B * k * 4);
            r_dist = st.out(out_dist, (size_t)B * k * db);
            r_cnt = st.out(out_count, (size_t)B * 4);
            r_out = st.out(out, (size_t)B * sizeof(kdb_consensus));
            r_sim = st.out(out_similarity, (size_t)B * k * 8);
            return KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return belief_dev_locked(idx, q.at<float>(d), B, k, ef, allow.at<uint64_t>(d), act.at<uint64_t>(d), flags & ~(uint32_t)KDB_SEARCH_FAIL_ON_DROP, r_ids.at<uint32_t>(d),
                                     r_dist.at<float>(d), r_cnt.at<uint32_t>(d), r_out.at<kdb_consensus>(d), r_sim.at<double>(d), s);
        });
}
