// kdb_api_merge.hip -- host side of the C ABI (include/kektor_hip.h): the merge of the shards' answers, on the host and on the device.
#include "kdb_internal.h"
#include "kdb_host.h"
#include <math.h>
#include <algorithm>

extern "C" int kdb_merge_topk(uint32_t metric, uint32_t precision, uint32_t G, uint32_t B, uint32_t k,
                              const uint32_t *in_ids, const float *in_dist, const uint32_t *in_count,
                              const uint32_t *id_base, uint32_t *out_ids, float *out_dist, uint32_t *out_count) {
    // Host-side shard merge (G*k entries per query; no vector arithmetic).  Total order (key, id)
    // with key = raw value, or -dot for the f32 cosine path -- identical to merge_topk_kernel.
    if (!in_ids || !in_dist || !in_count || !out_ids || !out_dist || !out_count || k == 0) {
        kdb_set_error("merge_topk: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    const bool negate = metric == KDB_METRIC_COSINE && precision == KDB_PREC_F32;
    struct E { float key; uint32_t id; float d; };
    std::vector<E> buf;
    for (uint32_t q = 0; q < B; q++) {
        buf.clear();
        uint32_t tied = 0; // bit 31 of a shard's count (KDB_COUNT_TIED) is not part of the length; the merged count carries it
        for (uint32_t g = 0; g < G; g++) {
            uint32_t c = in_count[(size_t)g * B + q] & KDB_COUNT_MASK;
            tied |= in_count[(size_t)g * B + q] & KDB_COUNT_TIED;
            if (c > k) c = k;
            for (uint32_t i = 0; i < c; i++) {
                const size_t off = ((size_t)g * B + q) * k + i;
                buf.push_back({negate ? -in_dist[off] : in_dist[off], in_ids[off] + (id_base ? id_base[g] : 0u), in_dist[off]});
            }
        }
        std::sort(buf.begin(), buf.end(), [](const E &a, const E &b) { return a.key < b.key || (a.key == b.key && a.id < b.id); });
        const uint32_t n = buf.size() < k ? (uint32_t)buf.size() : k;
        for (uint32_t i = 0; i < k; i++) {
            out_ids[(size_t)q * k + i] = i < n ? buf[i].id : 0u;
            out_dist[(size_t)q * k + i] = i < n ? buf[i].d : INFINITY;
        }
        out_count[q] = n | tied;
    }
    return KDB_OK;
}

// The same for int8 shards, whose distances the reference computes and ORDERS as float64 (hnsw_index.go:2429-2454): doubles in,
// doubles out, total order (distance, global id).
extern "C" int kdb_merge_topk_f64(uint32_t G, uint32_t B, uint32_t k, const uint32_t *in_ids, const double *in_dist, const uint32_t *in_count,
                                  const uint32_t *id_base, uint32_t *out_ids, double *out_dist, uint32_t *out_count) {
    if (!in_ids || !in_dist || !in_count || !out_ids || !out_dist || !out_count || k == 0) {
        kdb_set_error("merge_topk_f64: null buffer or k == 0");
        return KDB_ERR_INVALID;
    }
    struct E { double d; uint32_t id; };
    std::vector<E> buf;
    for (uint32_t q = 0; q < B; q++) {
        buf.clear();
        uint32_t tied = 0; // bit 31 of a shard's count (KDB_COUNT_TIED) is not part of the length; the merged count carries it
        for (uint32_t g = 0; g < G; g++) {
            uint32_t c = in_count[(size_t)g * B + q] & KDB_COUNT_MASK;
            tied |= in_count[(size_t)g * B + q] & KDB_COUNT_TIED;
            if (c > k) c = k;
            for (uint32_t i = 0; i < c; i++) {
                const size_t off = ((size_t)g * B + q) * k + i;
                buf.push_back({in_dist[off], in_ids[off] + (id_base ? id_base[g] : 0u)});
            }
        }
        std::sort(buf.begin(), buf.end(), [](const E &a, const E &b) { return a.d < b.d || (a.d == b.d && a.id < b.id); });
        const uint32_t n = buf.size() < k ? (uint32_t)buf.size() : k;
        for (uint32_t i = 0; i < k; i++) {
            out_ids[(size_t)q * k + i] = i < n ? buf[i].id : 0u;
            out_dist[(size_t)q * k + i] = i < n ? buf[i].d : (double)INFINITY;
        }
        out_count[q] = n | tied;
    }
    return KDB_OK;
}

extern "C" int kdb_merge_topk_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_in_ids,
                                  const float *d_in_dist, const uint32_t *d_in_count, const uint32_t *d_id_base,
                                  uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const int negate = idx->desc.metric == KDB_METRIC_COSINE && idx->desc.precision == KDB_PREC_F32;
    return kdb_launch_merge_topk(negate, G, B, k, d_in_ids, d_in_dist, d_in_count, 0, 0, d_id_base, d_out_ids, d_out_dist,
                                 d_out_count, s);
}

extern "C" int kdb_merge_topk_packed_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_packed,
                                         uint64_t stride_words, const uint32_t *d_id_base, uint32_t *d_out_ids,
                                         float *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    const uint64_t block = 2ull * B * k + B;
    if (!d_packed || !d_out_ids || !d_out_dist || !d_out_count || k == 0 || stride_words < block) {
        kdb_set_error("merge_topk_packed: null buffer, k == 0 or stride %llu < 2*B*k+B = %llu", (unsigned long long)stride_words,
                      (unsigned long long)block);
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const int negate = idx->desc.metric == KDB_METRIC_COSINE && idx->desc.precision == KDB_PREC_F32;
    const size_t bk = (size_t)B * k;
    return kdb_launch_merge_topk(negate, G, B, k, d_packed, reinterpret_cast<const float *>(d_packed + bk), d_packed + 2 * bk,
                                 (size_t)stride_words, (size_t)stride_words, d_id_base, d_out_ids, d_out_dist, d_out_count, s);
}

// int8 shards: the block one all-gather delivers carries float64 distances -- dist64[B][k] | ids[B][k] | count[B], stride in
// 32-bit words (even, >= 3*B*k + B) -- and the merge orders doubles; d_out_dist receives doubles
extern "C" int kdb_merge_topk_packed_f64_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_packed,
                                             uint64_t stride_words, const uint32_t *d_id_base, uint32_t *d_out_ids,
                                             double *d_out_dist, uint32_t *d_out_count, void *stream) {
    KDB_CHECK_IDX(idx);
    const uint64_t block = 3ull * B * k + B;
    if (!d_packed || !d_out_ids || !d_out_dist || !d_out_count || k == 0 || stride_words < block || (stride_words & 1ull)) {
        kdb_set_error("merge_topk_packed_f64: null buffer, k == 0, odd stride or stride %llu < 3*B*k+B = %llu", (unsigned long long)stride_words,
                      (unsigned long long)block);
        return KDB_ERR_INVALID;
    }
    DevCall call(idx, stream, false);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const size_t bk = (size_t)B * k;
    return kdb_launch_merge_topk_f64(G, B, k, d_packed + 2 * bk, reinterpret_cast<const double *>(d_packed), d_packed + 3 * bk, (size_t)stride_words,
                                     (size_t)stride_words / 2, (size_t)stride_words, d_id_base, d_out_ids, d_out_dist, 1, d_out_count, s);
}
