// kdb_api_text.hip -- host side of the C ABI (include/kektor_hip.h): text snapshots, BM25 search and the hybrid request.
#include "kdb_internal.h"
#include "kdb_host.h"
#include "kdb_text_plan.h"
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <vector>

// ---------------------------------------------------------------------------------------------
// The text index in HBM (text.hip, kdb_text_plan.h): textIndex[index][field] and TextIndexStats (pkg/core/core.go:944) as posting
// arrays in ONE allocation per field.  Everything a call can judge without the index is judged BEFORE the handle is looked at, so the
// checks run -- and are tested -- on a machine without a device.
// ---------------------------------------------------------------------------------------------
static int text_field_check(const char *who, uint32_t field) {
    if (field >= KDB_MAX_TEXT_FIELDS) {
        kdb_set_error("%s: field %u (fields 0..%u)", who, field, KDB_MAX_TEXT_FIELDS - 1u);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}

extern "C" int kdb_index_set_text(kdb_index *idx, uint32_t field, const kdb_text_view *v) {
    int rc = text_field_check("set_text", field);
    if (rc) return rc;
    uint32_t bad = 0;
    const int vrc = kdb_text_validate_view(v, idx ? idx->cap : 0xffffffffu, &bad);
    if (vrc) {
        kdb_set_error("set_text: %s (token %u)", kdb_text_strerror(vrc), bad);
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    const uint32_t V = v->n_tokens;
    const uint64_t np = v->post_off[V];
    std::vector<double> idf(V);
    for (uint32_t t = 0; t < V; t++) idf[t] = v->idf ? v->idf[t] : kdb_bm25_idf(v->total_docs, v->post_off[t + 1] - v->post_off[t]);
    KdbCarver cv; // post_off | idf | post_doc | post_tf | doc_len
    const size_t o_off = cv.take(((size_t)V + 1) * 8), o_idf = cv.take((size_t)V * 8), o_doc = cv.take((size_t)np * 4), o_tf = cv.take((size_t)np * 4),
                 o_len = cv.take(((size_t)v->n_ids + 1) * 4);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (v->n_ids > idx->cap) {
        kdb_set_error("set_text: n_ids %u above the index's capacity %u", v->n_ids, idx->cap);
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    unsigned char *p = nullptr;
    KDB_HIP(hipMalloc(reinterpret_cast<void **>(&p), cv.total()));
    hipError_t e = hipMemcpyAsync(p + o_off, v->post_off, ((size_t)V + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && V) e = hipMemcpyAsync(p + o_idf, idf.data(), (size_t)V * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && np) e = hipMemcpyAsync(p + o_doc, v->post_doc, (size_t)np * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && np) e = hipMemcpyAsync(p + o_tf, v->post_tf, (size_t)np * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p + o_len, v->doc_len, ((size_t)v->n_ids + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // host values are consumed
    if (e == hipSuccess) e = hipDeviceSynchronize();  // text kernels of callers' streams may still read the snapshot this one replaces
    if (e != hipSuccess) {
        (void)hipFree(p);
        kdb_set_error("set_text: upload failed: %s", hipGetErrorString(e));
        return KDB_ERR_HIP;
    }
    kdb_text_slot &sl = idx->text[field];
    if (sl.blob) (void)hipFree(sl.blob);
    sl = kdb_text_slot{};
    sl.blob = p;
    sl.dev.post_off = reinterpret_cast<const uint64_t *>(p + o_off);
    sl.dev.idf = reinterpret_cast<const double *>(p + o_idf);
    sl.dev.post_doc = reinterpret_cast<const uint32_t *>(p + o_doc);
    sl.dev.post_tf = reinterpret_cast<const uint32_t *>(p + o_tf);
    sl.dev.doc_len = reinterpret_cast<const uint32_t *>(p + o_len);
    sl.dev.avg_len = v->avg_len;
    sl.dev.n_tokens = V;
    sl.dev.n_ids = v->n_ids;
    sl.n_postings = np;
    sl.bytes = cv.total();
    sl.h_post_off.assign(v->post_off, v->post_off + V + 1);
    for (uint32_t t = 0; t < V; t++) sl.longest = std::max<uint64_t>(sl.longest, v->post_off[t + 1] - v->post_off[t]);
    return KDB_OK;
}

extern "C" int kdb_index_drop_text(kdb_index *idx, uint32_t field) {
    int rc = text_field_check("drop_text", field);
    if (rc) return rc;
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx);
    kdb_text_slot &sl = idx->text[field];
    if (!sl.blob) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    KDB_HIP(hipDeviceSynchronize()); // text kernels of callers' streams may still read the snapshot
    (void)hipFree(sl.blob);
    sl = kdb_text_slot{};
    return KDB_OK;
}

extern "C" int kdb_index_text_info(kdb_index *idx, uint32_t field, uint32_t *n_tokens, uint64_t *n_postings, uint64_t *bytes) {
    int rc = text_field_check("text_info", field);
    if (rc) return rc;
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    const kdb_text_slot &sl = idx->text[field];
    if (n_tokens) *n_tokens = sl.dev.n_tokens;
    if (n_postings) *n_postings = sl.n_postings;
    if (bytes) *bytes = sl.bytes;
    return KDB_OK;
}

// ---------------------------------------------------------------------------------------------
// FindIDsByTextSearch cut at k (bm25_topk_kernel).  The kernel reads the snapshot, the tokens and the allow list where they are; with
// one workgroup per query it needs no scratch: the _dev form takes no lane, the host-pointer form takes one turn and launches outside
// idx->mu, like the consensus.  A call of few queries with long lists gives every query several workgroups (kdb_text_split_plan):
// their partial lists are one more region of the turn -- or, for the _dev form, the scratch of a lane it then takes.
// ---------------------------------------------------------------------------------------------
static int text_call_check(const char *who, uint32_t field, uint32_t B, uint32_t t_stride, uint32_t k, const void *tokens, const void *n_tokens,
                           const void *out_ids, const void *out_score, const void *out_count) {
    if (const char *why = kdb_text_call_check(field, t_stride, k)) {
        kdb_set_error("%s: %s (field %u, t_stride %u, k %u)", who, why, field, t_stride, k);
        return KDB_ERR_INVALID;
    }
    if (B && (!n_tokens || (!tokens && t_stride) || !out_ids || !out_score || !out_count)) {
        kdb_set_error("%s: null buffer", who);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}
static int text_slot_check(const char *who, const kdb_index *idx, uint32_t field) { // under idx->mu
    if (!idx->text[field].blob) {
        kdb_set_error("%s: text field %u holds no snapshot (kdb_index_set_text)", who, field);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}
static int text_lengths_check(const char *who, const uint32_t *n_tokens, uint32_t B, uint32_t t_stride) {
    for (uint32_t b = 0; b < B; b++)
        if (n_tokens[b] > t_stride) {
            kdb_set_error("%s: query %u has %u tokens, more than t_stride %u", who, b, n_tokens[b], t_stride);
            return KDB_ERR_INVALID;
        }
    return KDB_OK;
}

// What the split plan (kdb_text_plan.h: kdb_text_split_plan) decides from; under idx->mu.  postings_bound: what the caller knows, or
// 0 = the bound of a call whose tokens are on the device, the slot's longest list times the tokens a query can have.
// KDB_TEXT_SPLIT is read per call: tests toggle it inside one process (0: never split; N: N parts, whatever the size).
static KdbTextSplitIn text_split_in(const kdb_index *idx, uint32_t field, uint32_t B, uint32_t t_stride, uint32_t k, uint64_t postings_bound) {
    const kdb_text_slot &sl = idx->text[field];
    KdbTextSplitIn in{};
    in.B = B, in.k = k;
    in.n_ids = sl.dev.n_ids;
    in.n_cus = (uint32_t)idx->n_cu;
    in.postings_bound = postings_bound ? postings_bound : sl.longest * std::min(t_stride, (uint32_t)KDB_TEXT_MAX_TOKENS);
    in.forced = -1;
    if (const char *e = getenv("KDB_TEXT_SPLIT")) in.forced = std::max(0, atoi(e));
    return in;
}
// the most postings one query of a host-pointer call sweeps, exactly (at least 1: 0 asks text_split_in for the other bound)
static uint64_t text_postings_bound(const kdb_text_slot &sl, const uint32_t *tokens, const uint32_t *n_tokens, uint32_t B, uint32_t t_stride) {
    uint64_t most = 1;
    for (uint32_t b = 0; b < B; b++) {
        uint64_t sum = 0;
        for (uint32_t t = 0; t < n_tokens[b] && t < KDB_TEXT_MAX_TOKENS; t++) {
            const uint32_t tok = tokens[(size_t)b * t_stride + t];
            if (tok < sl.dev.n_tokens) sum += sl.h_post_off[tok + 1u] - sl.h_post_off[tok];
        }
        most = std::max(most, sum);
    }
    return most;
}

// TEST HOOK: the plan a text call of B queries would launch with; launches nothing
extern "C" int kdb_probe_text_plan(kdb_index *idx, uint32_t field, uint32_t B, uint32_t t_stride, uint32_t k, uint64_t postings_bound, uint64_t *out) {
    if (const char *why = kdb_text_call_check(field, t_stride, k)) {
        kdb_set_error("probe_text_plan: %s (field %u, t_stride %u, k %u)", why, field, t_stride, k);
        return KDB_ERR_INVALID;
    }
    if (!out) {
        kdb_set_error("probe_text_plan: null buffer");
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    if (const int rc = text_slot_check("probe_text_plan", idx, field)) return rc;
    const KdbTextSplitIn in = text_split_in(idx, field, B, t_stride, k, postings_bound);
    const KdbTextSplitPlan plan = kdb_text_split_plan(in);
    out[0] = plan.parts, out[1] = plan.scratch_bytes, out[2] = plan.merge_lds, out[3] = in.postings_bound;
    return KDB_OK;
}

extern "C" int kdb_text_search_batch_dev(kdb_index *idx, uint32_t field, const uint32_t *d_tokens, const uint32_t *d_n_tokens, uint32_t B,
                                         uint32_t t_stride, uint32_t k, const uint64_t *d_allow_bits, uint32_t *d_out_ids, double *d_out_score,
                                         uint32_t *d_out_count, double *d_out_max, uint32_t *d_out_ncand, void *stream) {
    int rc = text_call_check("text_search", field, B, t_stride, k, d_tokens, d_n_tokens, d_out_ids, d_out_score, d_out_count);
    if (rc) return rc;
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    rc = text_slot_check("text_search", idx, field);
    if (rc) return rc;
    const KdbTextSplitPlan plan = kdb_text_split_plan(text_split_in(idx, field, B, t_stride, k, 0));
    void *d_parts = nullptr;
    if (plan.parts > 1u) { // the partial lists live in a scratch lane: only a split call takes one
        if ((rc = call.take_lane()) || (rc = kdb_ensure_scratch(idx, plan.scratch_bytes))) return rc;
        d_parts = kdb_cur(idx).d_scratch;
    }
    return kdb_launch_bm25_topk(idx->text[field].dev, d_tokens, d_n_tokens, B, t_stride, k, reinterpret_cast<const uint32_t *>(d_allow_bits), idx->count,
                                d_out_ids, d_out_score, d_out_count, d_out_max, d_out_ncand, plan, d_parts, call.s);
}

extern "C" int kdb_text_search_batch(kdb_index *idx, uint32_t field, const uint32_t *tokens, const uint32_t *n_tokens, uint32_t B, uint32_t t_stride,
                                     uint32_t k, const uint64_t *allow_bits, uint32_t *out_ids, double *out_score, uint32_t *out_count, double *out_max,
                                     uint32_t *out_ncand) {
    int rc = text_call_check("text_search", field, B, t_stride, k, tokens, n_tokens, out_ids, out_score, out_count);
    if (rc) return rc;
    if (B && (rc = text_lengths_check("text_search", n_tokens, B, t_stride))) return rc;
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion r_tok, r_nt, r_allow, r_ids, r_score, r_cnt, r_max, r_nc, r_parts;
    KdbTextDev tx;
    KdbTextSplitPlan plan{};
    uint32_t count = 0;
    KdbTurnOpt opt;
    opt.lane = false; // (a split call's partial lists are a region of the turn: still no lane)
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            if (const int src = text_slot_check("text_search", idx, field)) return src;
            r_tok = st.in(tokens, (size_t)B * t_stride * 4);
            r_nt = st.in(n_tokens, (size_t)B * 4);
            r_allow = st.in(allow_bits, kdb_bits_bytes(idx->count));
            r_ids = st.out(out_ids, (size_t)B * k * 4);
            r_score = st.out(out_score, (size_t)B * k * 8);
            r_cnt = st.out(out_count, (size_t)B * 4);
            r_max = st.out(out_max, (size_t)B * 8);
            r_nc = st.out(out_ncand, (size_t)B * 4);
            plan = kdb_text_split_plan(text_split_in(idx, field, B, t_stride, k, text_postings_bound(idx->text[field], tokens, n_tokens, B, t_stride)));
            r_parts = st.dev(plan.scratch_bytes);
            tx = idx->text[field].dev; // (once staged the call is counted: writers stay out, the snapshot and count cannot move)
            count = idx->count;
            return (int)KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return kdb_launch_bm25_topk(tx, r_tok.at<uint32_t>(d), r_nt.at<uint32_t>(d), B, t_stride, k, r_allow.at<uint32_t>(d), count, r_ids.at<uint32_t>(d),
                                        r_score.at<double>(d), r_cnt.at<uint32_t>(d), r_max.at<double>(d), r_nc.at<uint32_t>(d), plan, r_parts.at<unsigned char>(d), s);
        });
}

// ---------------------------------------------------------------------------------------------
// searchWithFusion (pkg/engine/ops.go:897-1209) without time decay, as ONE call: a COMPOSITION like kdb_belief_batch.
// kdb_search_dev_locked runs unchanged, bm25_topk_kernel with the same k and allow list, then hybrid_fuse_kernel on both answers;
// the two intermediate answers live in one region of the turn's buffer and never cross the bus.
// ---------------------------------------------------------------------------------------------
extern "C" int kdb_hybrid_search_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, uint32_t field, const uint32_t *tokens,
                                       const uint32_t *n_tokens, uint32_t t_stride, double alpha, const uint64_t *allow_bits, uint32_t flags,
                                       uint32_t *out_ids, double *out_score, uint32_t *out_count) {
    int rc = text_call_check("hybrid_search", field, B, t_stride, k, tokens, n_tokens, out_ids, out_score, out_count);
    if (rc) return rc;
    if (alpha != alpha) {
        kdb_set_error("hybrid_search: alpha is NaN");
        return KDB_ERR_INVALID;
    }
    if (flags & (KDB_SEARCH_PREPARED | KDB_SEARCH_DIST_F64 | KDB_SEARCH_FAIL_ON_DROP)) {
        kdb_set_error("hybrid_search: flags 0x%x (KDB_SEARCH_PREPARED, KDB_SEARCH_DIST_F64 and KDB_SEARCH_FAIL_ON_DROP are not accepted)", flags);
        return KDB_ERR_INVALID;
    }
    if (B && !queries) {
        kdb_set_error("hybrid_search: null buffer");
        return KDB_ERR_INVALID;
    }
    if (B && (rc = text_lengths_check("hybrid_search", n_tokens, B, t_stride))) return rc;
    KDB_CHECK_IDX(idx);
    if (B == 0) return KDB_OK;
    if (alpha < 0 || alpha > 1) alpha = 0.5; // ops.go:1089
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion r_q, r_tok, r_nt, r_allow, r_ids, r_score, r_cnt, r_work;
    KdbCarver wc; // the region only the device uses: vector ids | distances | counts | text ids | scores | counts | maxima | partial lists
    const size_t o_vi = wc.take((size_t)B * k * 4), o_vd = wc.take((size_t)B * k * 4), o_vc = wc.take((size_t)B * 4), o_ti = wc.take((size_t)B * k * 4),
                 o_ts = wc.take((size_t)B * k * 8), o_tc = wc.take((size_t)B * 4), o_tm = wc.take((size_t)B * 8);
    size_t o_parts = 0; // (sized under idx->mu: the split plan reads the slot)
    KdbTextSplitPlan plan{};
    KdbTurnOpt opt;
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            if (const int src = text_slot_check("hybrid_search", idx, field)) return src;
            r_q = st.in(queries, (size_t)B * idx->desc.dim * 4);
            r_tok = st.in(tokens, (size_t)B * t_stride * 4);
            r_nt = st.in(n_tokens, (size_t)B * 4);
            r_allow = st.in(allow_bits, kdb_bits_bytes(idx->count));
            r_ids = st.out(out_ids, (size_t)B * k * 4);
            r_score = st.out(out_score, (size_t)B * k * 8);
            r_cnt = st.out(out_count, (size_t)B * 4);
            plan = kdb_text_split_plan(text_split_in(idx, field, B, t_stride, k, text_postings_bound(idx->text[field], tokens, n_tokens, B, t_stride)));
            o_parts = wc.take(plan.scratch_bytes);
            r_work = st.dev(wc.total());
            return (int)KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            unsigned char *const w = r_work.at<unsigned char>(d);
            uint32_t *const v_ids = reinterpret_cast<uint32_t *>(w + o_vi), *const v_cnt = reinterpret_cast<uint32_t *>(w + o_vc);
            float *const v_dist = reinterpret_cast<float *>(w + o_vd);
            uint32_t *const t_ids = reinterpret_cast<uint32_t *>(w + o_ti), *const t_cnt = reinterpret_cast<uint32_t *>(w + o_tc);
            double *const t_score = reinterpret_cast<double *>(w + o_ts), *const t_max = reinterpret_cast<double *>(w + o_tm);
            const KdbTextDev &tx = idx->text[field].dev;
            int lrc = kdb_search_dev_locked(idx, r_q.at<float>(d), B, k, ef, r_allow.at<uint64_t>(d), flags, v_ids, v_dist, v_cnt, s);
            if (lrc) return lrc;
            lrc = kdb_launch_bm25_topk(tx, r_tok.at<uint32_t>(d), r_nt.at<uint32_t>(d), B, t_stride, k, r_allow.at<uint32_t>(d), idx->count, t_ids, t_score, t_cnt,
                                       t_max, nullptr, plan, w + o_parts, s);
            if (lrc) return lrc;
            const uint32_t one_minus_dot = idx->desc.precision == KDB_PREC_F32 && idx->desc.metric == KDB_METRIC_COSINE; // "Conventions": 1.0 - float64(dot)
            return kdb_launch_hybrid_fuse(tx, r_tok.at<uint32_t>(d), r_nt.at<uint32_t>(d), B, t_stride, k, alpha, one_minus_dot, v_ids, v_dist, v_cnt, t_ids, t_score,
                                          t_cnt, t_max, r_ids.at<uint32_t>(d), r_score.at<double>(d), r_cnt.at<uint32_t>(d), s);
        });
}
