// by_id.hip -- stored rows as queries: the device side of GetNodeData / VGetMany (pkg/core/hnsw/hnsw_index.go:2909-2959) and the
// small epilogue of the by-id entry points (kdb_search_by_id / kdb_flat_scan_by_id, kdb_api_query.hip).
//
//   decode_rows_kernel   ids[n] -> out[n][dim] float32, the vector GetNodeData hands to its callers: float32 rows as stored, float16
//                        rows widened, int8 rows through Quantizer.Dequantize (quantizer.go:181-198).  An id that is 0, above count
//                        or marked deleted is "not found" (:2921-2931): found[i] = 0 and the row is filled with `miss` -- zeros for
//                        the public decode and the exact scan, a quiet NaN for the graph search (see kdb_api_query.hip).
//   by_id_finish_kernel  the [B][k] answers of the caller from the [B][kin] answers of the inner call: not-found sources get no
//                        results; KDB_BY_ID_DROP_SELF (kin = k + 1) removes the source's own id, or else the last entry.
//
// Nothing here computes a distance: the walk and the scan are the existing ones, fed from the decode buffer.
#include "kdb_internal.h"
#include "kdb_decode.cuh"

namespace {

// One gather per id: 16 lanes per row, one 16-byte load per lane and trip (4 floats / 8 halfs / 16 int8 values), 16 rows per
// 256-thread workgroup.  The id is range-checked -- and its deleted bit read -- before a row address is formed.  Rows start on
// 16-byte boundaries for every precision (ld is a multiple of 16 elements).  The output has no padding: row i starts at
// out + i * dim, so it is written as float4 only when dim is a multiple of 4 (then every row start is 16-byte aligned with the
// base), column by column otherwise; either way the 16 lanes of a row write one contiguous run.
// The 16 bytes become floats in kdb_decode16 (kdb_decode.cuh), which the consensus kernel shares.
template <int PREC>
__global__ void __launch_bounds__(256)
decode_rows_kernel(KdbView v, const uint32_t *__restrict__ ids, uint32_t n, float *__restrict__ out, uint8_t *__restrict__ found,
                   uint32_t miss_bits, int vec_out) {
    constexpr uint32_t E = KdbDecode<PREC>::E; // elements per 16-byte load
    const uint32_t t = threadIdx.x & 15u;
    const uint32_t r = blockIdx.x * 16u + (threadIdx.x >> 4);
    if (r >= n) return;
    const uint32_t id = ids[r];
    const bool ok = kdb_row_found(v, id); // 1 <= id <= count, not deleted
    if (t == 0 && found) found[r] = ok ? 1 : 0;
    float *const o = out + (size_t)r * v.dim;
    const float miss = __uint_as_float(miss_bits);
    const uint4 *row = nullptr;
    if (ok) row = kdb_row_ptr16<PREC>(v, id);
    for (uint32_t c = t * E; c < v.ld; c += 16u * E) {
        float x[E];
        if (ok) {
            kdb_decode16<PREC>(row[c / E], v.q_absmax, x);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < E; j++) x[j] = miss;
        }
        if (vec_out) { // dim % 4 == 0: whole float4s are inside or outside the row
#pragma unroll
            for (uint32_t j = 0; j < E; j += 4)
                if (c + j < v.dim) *reinterpret_cast<float4 *>(o + c + j) = make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < E; j++)
                if (c + j < v.dim) o[c + j] = x[j];
        }
    }
}

// One wave per query, four queries per workgroup.  in_*: [B][kin] (distances of dw 32-bit words each: 1 = float, 2 = double),
// out_*: [B][k], kin == k (in place allowed: only not-found sources are rewritten) or kin == k + 1 (drop_self; never in place).
// Entries behind the count are written as the walk writes them: id 0, distance +Inf.  Bit 31 of the count (KDB_COUNT_TIED) stays.
__global__ void __launch_bounds__(256)
by_id_finish_kernel(const uint32_t *__restrict__ src_ids, const uint8_t *__restrict__ found, uint32_t B, uint32_t k, uint32_t kin,
                    uint32_t dw, const uint32_t *in_ids, const uint32_t *in_dist, const uint32_t *in_cnt, uint32_t *out_ids,
                    uint32_t *out_dist, uint32_t *out_cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= B) return;
    const uint32_t *ii = in_ids + (size_t)b * kin;
    const uint32_t *id_ = in_dist + (size_t)b * kin * dw;
    uint32_t *oi = out_ids + (size_t)b * k;
    uint32_t *od = out_dist + (size_t)b * k * dw;
    const uint32_t raw = in_cnt[b];
    uint32_t c = raw & KDB_COUNT_MASK;
    if (c > kin) c = kin;
    uint32_t nc = c, p = 0xffffffffu;
    const bool drop = kin != k;
    if (!found[b]) nc = 0;
    else if (drop) {
        const uint32_t self = src_ids[b];
        for (uint32_t j = lane; j < c; j += 64u)
            if (ii[j] == self && j < p) p = j;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t q = (uint32_t)__shfl_xor((int)p, o, 64);
            p = q < p ? q : p;
        }
        nc = p < c ? c - 1u : (c < k ? c : k); // the source's own entry leaves, else the last of k + 1
    } else {
        return; // found, nothing to drop: the inner call's answer is the answer (in place)
    }
    for (uint32_t j = lane; j < k; j += 64u) {
        if (j < nc) {
            const uint32_t s = j + (j >= p ? 1u : 0u);
            oi[j] = ii[s];
            for (uint32_t w = 0; w < dw; w++) od[(size_t)j * dw + w] = id_[(size_t)s * dw + w];
        } else {
            oi[j] = 0u;
            if (dw == 1) od[j] = 0x7f800000u;
            else {
                od[(size_t)j * 2] = 0u;
                od[(size_t)j * 2 + 1] = 0x7ff00000u;
            }
        }
    }
    if (lane == 0) out_cnt[b] = nc | (found[b] ? (raw & KDB_COUNT_TIED) : 0u);
}

} // namespace

int kdb_launch_decode_rows(const KdbView &v, const uint32_t *d_ids, uint32_t n, float *d_out, uint8_t *d_found, uint32_t miss_bits,
                           hipStream_t s) {
    if (n == 0) return KDB_OK;
    const dim3 grid((n + 15u) / 16u), block(256);
    const int vec_out = (v.dim & 3u) == 0u && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0u;
    if (v.precision == KDB_PREC_F32) hipLaunchKernelGGL(decode_rows_kernel<KDB_PREC_F32>, grid, block, 0, s, v, d_ids, n, d_out, d_found, miss_bits, vec_out);
    else if (v.precision == KDB_PREC_F16) hipLaunchKernelGGL(decode_rows_kernel<KDB_PREC_F16>, grid, block, 0, s, v, d_ids, n, d_out, d_found, miss_bits, vec_out);
    else if (v.precision == KDB_PREC_I8) hipLaunchKernelGGL(decode_rows_kernel<KDB_PREC_I8>, grid, block, 0, s, v, d_ids, n, d_out, d_found, miss_bits, vec_out);
    else {
        kdb_set_error("decode_rows: unsupported precision %u", v.precision);
        return KDB_ERR_UNSUPPORTED;
    }
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}

int kdb_launch_by_id_finish(const uint32_t *d_src_ids, const uint8_t *d_found, uint32_t B, uint32_t k, uint32_t kin, uint32_t dist_words,
                            const uint32_t *d_in_ids, const void *d_in_dist, const uint32_t *d_in_cnt, uint32_t *d_out_ids, void *d_out_dist,
                            uint32_t *d_out_cnt, hipStream_t s) {
    if (B == 0) return KDB_OK;
    hipLaunchKernelGGL(by_id_finish_kernel, dim3((B + 3u) / 4u), dim3(256), 0, s, d_src_ids, d_found, B, k, kin, dist_words, d_in_ids,
                       reinterpret_cast<const uint32_t *>(d_in_dist), d_in_cnt, d_out_ids, reinterpret_cast<uint32_t *>(d_out_dist), d_out_cnt);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}
