// kdb_api_filter.hip -- host side of the C ABI (include/kektor_hip.h): metadata columns and filters.
#include "kdb_internal.h"
#include "kdb_host.h"
#include "kdb_filter_plan.h"
#include <string.h>
#include <math.h>
#include <cmath>

// ---------------------------------------------------------------------------------------------
// Metadata filters on the device (filter.hip, kdb_filter_plan.h): the columns AddMetadataUnlocked (pkg/core/core.go:1640-1758) keeps
// as an inverted index and a B-tree, the allow lists FindIDsByFilter (:1766-1839) builds from them, and the filtered request as one
// call.  Columns are per-id arrays of cap + 1 entries that live and move with the index's other per-id arrays.
// ---------------------------------------------------------------------------------------------
static size_t col_elem(uint32_t kind) { return kind == KDB_COL_F64 ? 8 : 4; }

static int set_column_impl(kdb_index *idx, uint32_t col, uint32_t kind, uint32_t first_id, uint32_t n, const void *values, hipMemcpyKind dir) {
    KDB_CHECK_IDX(idx);
    if (col >= KDB_MAX_COLUMNS || (kind != KDB_COL_F64 && kind != KDB_COL_CODE)) {
        kdb_set_error("set_column: slot %u / kind %u (slots 0..%u, KDB_COL_F64 or KDB_COL_CODE)", col, kind, KDB_MAX_COLUMNS - 1u);
        return KDB_ERR_INVALID;
    }
    if (n && (!values || first_id == 0 || (uint64_t)first_id + n - 1 > idx->cap)) {
        kdb_set_error("set_column: ids %u..%llu outside 1..%u (or null values)", first_id, (unsigned long long)first_id + n - 1, idx->cap);
        return KDB_ERR_INVALID;
    }
    if (dir == hipMemcpyHostToDevice && kind == KDB_COL_F64) { // JSON carries no infinity (NaN = no value)
        const double *v = reinterpret_cast<const double *>(values);
        for (uint32_t i = 0; i < n; i++)
            if (std::isinf(v[i])) {
                kdb_set_error("set_column: values[%u] is infinite (a float64 metadata value is finite; NaN = no value)", i);
                return KDB_ERR_INVALID;
            }
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (idx->col_kind[col] && idx->col_kind[col] != kind) {
        kdb_set_error("set_column: slot %u holds kind %u (drop it first)", col, idx->col_kind[col]);
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    const size_t n1 = (size_t)idx->cap + 1, eb = col_elem(kind);
    if (!idx->d_col[col]) { // first upload: the slot, filled with "absent"
        void *p = nullptr;
        KDB_HIP(hipMalloc(&p, n1 * eb));
        const int rc = kdb_launch_col_fill(p, kind, 0, n1, s);
        if (rc) {
            (void)hipFree(p);
            return rc;
        }
        idx->d_col[col] = p;
        idx->col_kind[col] = kind;
    }
    if (n) KDB_HIP(hipMemcpyAsync(reinterpret_cast<unsigned char *>(idx->d_col[col]) + (size_t)first_id * eb, values, (size_t)n * eb, dir, s));
    KDB_HIP(hipStreamSynchronize(s)); // host values are consumed; later calls on callers' streams see the column
    return KDB_OK;
}
extern "C" int kdb_index_set_column(kdb_index *idx, uint32_t col, uint32_t kind, uint32_t first_id, uint32_t n, const void *values) {
    return set_column_impl(idx, col, kind, first_id, n, values, hipMemcpyHostToDevice);
}
extern "C" int kdb_index_set_column_dev(kdb_index *idx, uint32_t col, uint32_t kind, uint32_t first_id, uint32_t n, const void *d_values) {
    return set_column_impl(idx, col, kind, first_id, n, d_values, hipMemcpyDeviceToDevice);
}
extern "C" int kdb_index_drop_column(kdb_index *idx, uint32_t col) {
    KDB_CHECK_IDX(idx);
    if (col >= KDB_MAX_COLUMNS) {
        kdb_set_error("drop_column: slot %u (slots 0..%u)", col, KDB_MAX_COLUMNS - 1u);
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx);
    if (!idx->d_col[col]) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    KDB_HIP(hipDeviceSynchronize()); // filter kernels of callers' streams may still read the column
    (void)hipFree(idx->d_col[col]);
    idx->d_col[col] = nullptr;
    idx->col_kind[col] = 0;
    return KDB_OK;
}
extern "C" int kdb_index_column_info(kdb_index *idx, uint32_t col, uint32_t *kind, uint64_t *bytes) {
    KDB_CHECK_IDX(idx);
    if (col >= KDB_MAX_COLUMNS) {
        kdb_set_error("column_info: slot %u (slots 0..%u)", col, KDB_MAX_COLUMNS - 1u);
        return KDB_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    if (kind) *kind = idx->col_kind[col];
    if (bytes) *bytes = idx->d_col[col] ? ((uint64_t)idx->cap + 1) * col_elem(idx->col_kind[col]) : 0;
    return KDB_OK;
}

// arguments of a filter call that the host can judge without the device (the programs themselves: kdb_launch_filter_eval, under the lock)
static int filter_args_check(const char *who, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P) {
    if (!terms || !prog_offsets || P == 0 || P > KDB_FILTER_MAX_PROGRAMS) {
        kdb_set_error("%s: null terms / prog_offsets, or P = %u outside 1..%u", who, P, KDB_FILTER_MAX_PROGRAMS);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}
static int filter_words_check(const char *who, const kdb_index *idx, uint64_t words_per_list) {
    if (words_per_list < kdb_filter_min_words(idx->count) || words_per_list > KDB_FILTER_MAX_WORDS) {
        kdb_set_error("%s: words_per_list %llu outside (count>>6)+1 = %llu .. 2^30", who, (unsigned long long)words_per_list,
                      (unsigned long long)kdb_filter_min_words(idx->count));
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}

extern "C" int kdb_filter_eval_dev(kdb_index *idx, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P, uint64_t *d_lists,
                                   uint64_t words_per_list, uint32_t *d_card, void *stream) {
    KDB_CHECK_IDX(idx);
    int rc = filter_args_check("filter_eval", terms, prog_offsets, P);
    if (rc) return rc;
    if (!d_lists) {
        kdb_set_error("filter_eval: null d_lists");
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    rc = filter_words_check("filter_eval", idx, words_per_list);
    if (rc) return rc;
    return kdb_launch_filter_eval(idx, terms, prog_offsets, P, d_lists, words_per_list, d_card, call.s);
}

extern "C" int kdb_filter_eval(kdb_index *idx, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P, uint64_t *out_lists,
                               uint64_t words_per_list, uint32_t *out_card) {
    KDB_CHECK_IDX(idx);
    int rc = filter_args_check("filter_eval", terms, prog_offsets, P);
    if (rc) return rc;
    if (!out_lists && !out_card) {
        kdb_set_error("filter_eval: out_lists and out_card are both null");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion lists, card;
    KdbTurnOpt opt;
    opt.launch_first = true; // (the programs are staged by the launcher itself, into the lane's scratch: nothing to copy in here)
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) { // the kernel writes both whatever the caller asked for: an output nobody wants stays on the device
            if (const int wrc = filter_words_check("filter_eval", idx, words_per_list)) return wrc;
            const size_t lb = (size_t)P * words_per_list * 8, cb = (size_t)P * 4;
            lists = out_lists ? st.out(out_lists, lb) : st.dev(lb);
            card = out_card ? st.out(out_card, cb) : st.dev(cb);
            return (int)KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return kdb_launch_filter_eval(idx, terms, prog_offsets, P, lists.at<uint64_t>(d), words_per_list, card.at<uint32_t>(d), s);
        });
}

// Engine.VSearch with a filter, from programs to answers: a COMPOSITION like the by-id calls.  The programs are evaluated into the
// call's staging buffer, the P cardinalities come back (the one read-back routing needs), and each query goes -- with its program's
// list, in place -- to the entry point its program's cardinality selects: the multi-list walk, the grouped exact scan (float32 /
// float16, k <= 128) or the one-list exact scan (int8; 128 < k <= 1024), which run unchanged.  The host orders the queries by route
// before they are uploaded and scatters the answers back.  A program that matches nothing is answered here: the exact scan would
// read its empty list as "no filter" (vector_index.go:130).
extern "C" int kdb_search_filtered(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, const kdb_filter_term *terms,
                                   const uint32_t *prog_offsets, uint32_t P, const uint32_t *prog_of_query, double flat_selectivity, uint32_t flags,
                                   uint32_t *out_ids, float *out_dist, uint32_t *out_count, uint8_t *out_route, uint32_t *out_card) {
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (!queries || !out_ids || !out_dist || !out_count || !prog_of_query || k == 0) {
        kdb_set_error("search_filtered: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    int rc = filter_args_check("search_filtered", terms, prog_offsets, P);
    if (rc) return rc;
    if (flags & ~(uint32_t)(KDB_SEARCH_NEEDS_REFINE | KDB_SEARCH_TIE_FLAG | KDB_SEARCH_HEAP_ORDER)) {
        kdb_set_error("search_filtered: flags 0x%x (KDB_SEARCH_NEEDS_REFINE, KDB_SEARCH_TIE_FLAG and KDB_SEARCH_HEAP_ORDER are accepted)", flags);
        return KDB_ERR_INVALID;
    }
    if (!(flat_selectivity >= 0.0 && flat_selectivity <= 1.0)) {
        kdb_set_error("search_filtered: flat_selectivity must be within 0..1");
        return KDB_ERR_INVALID;
    }
    for (uint32_t b = 0; b < B; b++)
        if (prog_of_query[b] != KDB_NO_FILTER && prog_of_query[b] >= P) {
            kdb_set_error("search_filtered: prog_of_query[%u] = %u names no program (P = %u)", b, prog_of_query[b], P);
            return KDB_ERR_INVALID;
        }
    KDB_HIP(hipSetDevice(idx->device));
    HostTurn turn(idx);
    const uint32_t count = idx->count, dim = idx->desc.dim;
    const uint64_t wpl = kdb_filter_min_words(count);
    const size_t lb = (size_t)wpl * 8, qb = (size_t)dim * 4;
    KdbCarver cv; // lists of all programs | lists of the scanned programs, compact | cardinalities | queries by route | list of every walked query | answers by route
    const size_t o_lists = cv.take((size_t)P * lb), o_slists = cv.take((size_t)P * lb), o_card = cv.take((size_t)P * 4), o_q = cv.take((size_t)B * qb),
                 o_of = cv.take((size_t)B * 4), o_ids = cv.take((size_t)B * k * 4), o_dist = cv.take((size_t)B * k * 4), o_cnt = cv.take((size_t)B * 4);
    unsigned char *const d = turn.stage(cv.total());
    if (!d) return turn.rc;
    hipStream_t s = idx->stream;
    uint64_t *const d_lists = reinterpret_cast<uint64_t *>(d + o_lists);
    {
        KdbLaneGuard lane(idx, s);
        if (lane.rc) return lane.rc;
        rc = kdb_launch_filter_eval(idx, terms, prog_offsets, P, d_lists, wpl, reinterpret_cast<uint32_t *>(d + o_card), s);
    }
    if (rc) return rc;
    turn.lk.unlock();
    std::vector<uint32_t> card(P);
    KDB_HIP(hipMemcpyAsync(card.data(), d + o_card, (size_t)P * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    if (out_card) memcpy(out_card, card.data(), (size_t)P * 4);
    // order: walked queries (caller order) | scanned queries, program by program
    const KdbFilterRoute R = kdb_filter_route(card.data(), P, prog_of_query, B, count, k, flat_selectivity, KDB_FLAT_MAX_K);
    const std::vector<uint32_t> &order = R.order, &of_query = R.of_query, &scan_progs = R.scan_progs, &group_offsets = R.group_offsets;
    const uint32_t n_walk = R.n_walk, n_scan = R.n_scan, n_run = n_walk + n_scan;
    for (uint32_t b = 0; b < B; b++) { // what no launch writes: programs that match nothing
        const uint8_t r = R.route_of_query(prog_of_query[b]);
        if (out_route) out_route[b] = r;
        if (r != 2) continue;
        out_count[b] = 0;
        for (uint32_t j = 0; j < k; j++) {
            out_ids[(size_t)b * k + j] = 0u;
            out_dist[(size_t)b * k + j] = INFINITY;
        }
    }
    if (n_run == 0) return KDB_OK;
    std::vector<float> q((size_t)n_run * dim);
    for (uint32_t i = 0; i < n_run; i++) memcpy(q.data() + (size_t)i * dim, queries + (size_t)order[i] * dim, qb);
    float *const d_q = reinterpret_cast<float *>(d + o_q);
    uint32_t *const d_ids = reinterpret_cast<uint32_t *>(d + o_ids), *const d_cnt = reinterpret_cast<uint32_t *>(d + o_cnt);
    float *const d_dist = reinterpret_cast<float *>(d + o_dist);
    KDB_HIP(hipMemcpyAsync(d_q, q.data(), (size_t)n_run * qb, hipMemcpyHostToDevice, s));
    if (n_walk) KDB_HIP(hipMemcpyAsync(d + o_of, of_query.data(), (size_t)n_walk * 4, hipMemcpyHostToDevice, s));
    const bool grouped = idx->desc.precision != KDB_PREC_I8 && k <= 128u;
    uint64_t scan_total = 0;
    for (size_t g = 0; g < scan_progs.size(); g++) {
        scan_total += card[scan_progs[g]];
        if (grouped) // the grouped scan takes its lists back to back
            KDB_HIP(hipMemcpyAsync(d + o_slists + g * lb, d + o_lists + (size_t)scan_progs[g] * lb, lb, hipMemcpyDeviceToDevice, s));
    }
    turn.lk.lock();
    {
        KdbLaneGuard lane(idx, s);
        if (lane.rc) return lane.rc;
        if (n_walk) {
            MultiLists ml;
            ml.G = P;
            ml.words64 = wpl;
            ml.d_of_query = reinterpret_cast<const uint32_t *>(d + o_of);
            rc = kdb_search_dev_locked(idx, d_q, n_walk, k, ef, d_lists, flags, d_ids, d_dist, d_cnt, s, &ml);
        }
        if (!rc && n_scan && grouped) {
            const KdbView v = kdb_make_view(idx);
            const uint32_t Bpad = (n_scan + 127u) & ~127u;
            void *d_pq = nullptr;
            float *d_qnorm = nullptr;
            rc = kdb_ensure_rows16(idx, s);
            if (!rc) rc = kdb_prepare_queries(idx, v, d_q + (size_t)n_walk * dim, n_scan, Bpad, 0, &d_pq, &d_qnorm, s);
            if (!rc)
                rc = kdb_launch_flat_scan_groups(idx, v, d_pq, d_qnorm, n_scan, k, (uint32_t)scan_progs.size(), group_offsets.data(),
                                                 reinterpret_cast<const uint32_t *>(d + o_slists), (uint32_t)(wpl * 2), scan_total, d_ids + (size_t)n_walk * k,
                                                 d_dist + (size_t)n_walk * k, d_cnt + n_walk, 1, s);
            if (!rc) rc = kdb_launch_void_dead_queries(d_qnorm, n_scan, k, d_ids + (size_t)n_walk * k, d_dist + (size_t)n_walk * k, d_cnt + n_walk, false, s);
        } else if (!rc && n_scan) {
            for (size_t g = 0; g < scan_progs.size() && !rc; g++) {
                const size_t a = (size_t)n_walk + group_offsets[g];
                rc = kdb_flat_dev_locked(idx, d_q + a * dim, group_offsets[g + 1] - group_offsets[g], k, d_lists + (size_t)scan_progs[g] * wpl, 0, d_ids + a * k,
                                     d_dist + a * k, d_cnt + a, s);
            }
        }
    }
    turn.lk.unlock();
    if (rc) return rc;
    std::vector<uint32_t> r_ids((size_t)n_run * k), r_cnt(n_run);
    std::vector<float> r_dist((size_t)n_run * k);
    KDB_HIP(hipMemcpyAsync(r_ids.data(), d_ids, (size_t)n_run * k * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipMemcpyAsync(r_dist.data(), d_dist, (size_t)n_run * k * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipMemcpyAsync(r_cnt.data(), d_cnt, (size_t)n_run * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n_run; i++) {
        const uint32_t b = order[i];
        memcpy(out_ids + (size_t)b * k, r_ids.data() + (size_t)i * k, (size_t)k * 4);
        memcpy(out_dist + (size_t)b * k, r_dist.data() + (size_t)i * k, (size_t)k * 4);
        out_count[b] = r_cnt[i];
    }
    return KDB_OK;
}
