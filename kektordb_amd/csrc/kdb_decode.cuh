// kdb_decode.cuh -- one 16-byte piece of a stored row as the float32 values GetNodeData hands to its callers
// (pkg/core/hnsw/hnsw_index.go:2909-2959): float32 as stored, float16 widened, int8 through Quantizer.Dequantize
// (quantizer.go:181-198).  Shared by decode_rows_kernel (by_id.hip) and consensus_kernel (consensus.hip): whatever reads a stored
// row as "the node's vector" reads it through this routine, so the two cannot drift apart.
#pragma once
#include "kdb_internal.h"

// elements of one 16-byte load: 4 floats / 8 halfs / 16 int8 values
template <int PREC>
struct KdbDecode {
    static constexpr uint32_t E = PREC == KDB_PREC_F32 ? 4u : PREC == KDB_PREC_F16 ? 8u : 16u;
};

// int8: (float(v) / 127.0f) * abs_max in that order.  The division must be the correctly rounded one: hipcc's default
// (-fhip-fp32-correctly-rounded-divide-sqrt); the Makefile passes neither its negation nor -ffast-math, and -ffp-contract=off keeps the
// multiply from being fused with anything.
template <int PREC>
__device__ __forceinline__ void kdb_decode16(const uint4 w, float q_absmax, float (&x)[KdbDecode<PREC>::E]) {
    if constexpr (PREC == KDB_PREC_F32) {
        x[0] = __uint_as_float(w.x);
        x[1] = __uint_as_float(w.y);
        x[2] = __uint_as_float(w.z);
        x[3] = __uint_as_float(w.w);
    } else if constexpr (PREC == KDB_PREC_F16) {
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            _Float16 lo, hi;
            const uint16_t l16 = (uint16_t)(ws[j] & 0xffffu), h16 = (uint16_t)(ws[j] >> 16);
            __builtin_memcpy(&lo, &l16, 2);
            __builtin_memcpy(&hi, &h16, 2);
            x[2 * j] = (float)lo;
            x[2 * j + 1] = (float)hi;
        }
    } else {
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            const int8_t q = (int8_t)((ws[j >> 2] >> (8u * (j & 3u))) & 0xffu);
            float y = 0.f;
            if (q_absmax != 0.f) { // an untrained quantizer dequantizes to zeros
                const float d = (float)q / 127.0f;
                y = d * q_absmax;
            }
            x[j] = y;
        }
    }
}

// The id names a stored, live row: 1 <= id <= count and not marked deleted (:2921-2931).  Checked before a row address is formed.
__device__ __forceinline__ bool kdb_row_found(const KdbView &v, uint32_t id) {
    bool ok = id - 1u < v.count;
    if (ok) ok = ((v.deleted[id >> 5] >> (id & 31u)) & 1u) == 0u;
    return ok;
}

template <int PREC>
__device__ __forceinline__ const uint4 *kdb_row_ptr16(const KdbView &v, uint32_t id) {
    return reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(v.rows) + (size_t)id * v.ld * (16u / KdbDecode<PREC>::E));
}
