// consensus.hip -- CalculateConsensus (pkg/engine/epistemic_types.go:126-178) for B id lists: the arithmetic half of
// Engine.VBeliefState (pkg/engine/epistemic.go:22-182), which reads the k vectors of a search back with VGet and then computes a
// float32 centroid, the float64 CosineDistance (:299-320) of every vector to it, of every pair of vectors, and one similarity per
// vector against the query.  Here the rows stay in HBM and about 40 bytes per list leave the device.
//
//   consensus_kernel   one workgroup of four waves per list.  The list's vectors -- up to 64 nodes, then the centroid, then the query:
//                      nv = count + 2 "slots" -- are walked in chunks of 64 columns staged in LDS; every dot product and squared norm
//                      the reference forms is one float64 accumulator that lives in a register across the chunks and takes its
//                      columns in ascending order, so it equals the reference's sum bit for bit (the product of two widened float32
//                      values is exact in float64: fused and unfused multiply-add agree, only the order matters).  The epilogue
//                      (sqrt, divide, clamp, sum of squares, maximum, score) runs in the same kernel.
//
// Pair tiling: the slots are cut into groups of three, and lane t owns one 3 x 3 tile (gi <= gj) of the symmetric slot x slot matrix:
// at most 22 * 23 / 2 = 253 tiles for 66 slots, nine accumulators (18 VGPRs) per lane, and per four columns six 16-byte LDS reads
// feed 36 multiply-adds.  A list of 10 uses 4 groups = 10 lanes: short lists cost what they need.
// LDS: rows[66][68] floats -- 64 columns + 4 of padding: slot r, column c sits in the 16-byte LDS slot (r + c / 4) % 16, so the 16
// lanes that ds_read_b128 serves together, which read rows 3 apart, hit 16 different slots -- 17.9 KB, reused after the last chunk
// for the 253 x 9 accumulators (18.2 KB) the epilogue picks from; with the small arrays 19.8 KB: room for eight workgroups per CU
// (82-84 VGPRs, no scratch, allow five).
#include "kdb_internal.h"
#include "kdb_decode.cuh"

namespace {

constexpr uint32_t CS_CH = 64u;                       // columns per chunk
constexpr uint32_t CS_LDW = CS_CH + 4u;               // floats per staged row
constexpr uint32_t CS_MAXV = KDB_CONSENSUS_MAX_K + 2u; // nodes + centroid + query
constexpr uint32_t CS_MAXG = CS_MAXV / 3u;            // 22 groups of three slots
constexpr uint32_t CS_TILES = CS_MAXG * (CS_MAXG + 1u) / 2u;
static_assert(CS_MAXV % 3u == 0u && CS_TILES <= 256u, "one lane per tile");

struct alignas(16) ConsensusLds {
    union {
        float rows[CS_MAXV][CS_LDW];
        double acc[CS_TILES][9];
    } u;
    double sq[CS_MAXV];  // sqrt of every slot's squared norm
    double dsq[KDB_CONSENSUS_MAX_K]; // squared distance to the centroid, per active node
    double wmax[4];
    uint32_t id[KDB_CONSENSUS_MAX_K];
    uint32_t flag[KDB_CONSENSUS_MAX_K]; // bit 0 found, bit 1 active
    uint32_t act_lo, act_hi;            // the active nodes as a bitset over list positions
};

// CosineDistance (:299-320) from its three sums; sa, sb = sqrt(na), sqrt(nb).  math.Min(1, x) / math.Max(0, x): a NaN stays a NaN,
// -0 becomes +0.
__device__ __forceinline__ double cs_cosine_distance(double dot, double na, double nb, double sa, double sb) {
    if (na == 0.0 || nb == 0.0) return 1.0;
    double sim = dot / (sa * sb);
    if (sim > 1.0) sim = 1.0;
    if (sim <= 0.0) sim = 0.0;
    return 1.0 - sim;
}

template <int PREC>
__global__ void __launch_bounds__(256)
consensus_kernel(KdbView v, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ counts, uint32_t stride,
                 const float *__restrict__ queries, const uint32_t *__restrict__ active, kdb_consensus *__restrict__ out,
                 double *__restrict__ out_sim, float *__restrict__ out_centroid, double *__restrict__ out_gram) {
    constexpr uint32_t E = KdbDecode<PREC>::E;
    constexpr uint32_t LPR = CS_CH / E; // 16-byte loads per row and chunk
    __shared__ ConsensusLds s;
    const uint32_t t = threadIdx.x;
    const size_t b = blockIdx.x;
    uint32_t cnt = stride;
    if (counts) {
        cnt = counts[b] & KDB_COUNT_MASK;
        if (cnt > stride) cnt = stride;
    }
    const uint32_t sc = cnt, sqy = cnt + 1u, nv = cnt + 2u; // slots of the centroid and the query
    const uint32_t G = (nv + 2u) / 3u, ntile = G * (G + 1u) / 2u;

    if (t < 64u) { // wave 0: which entries are nodes, which of them active
        uint32_t id = 0u, f = 0u;
        if (t < cnt) {
            id = ids[b * stride + t];
            if (kdb_row_found(v, id)) { // range-checked before the active bit or a row is addressed
                f = 1u;
                if (!active || ((active[id >> 5] >> (id & 31u)) & 1u)) f = 3u;
            }
        }
        s.id[t] = id;
        s.flag[t] = f;
        const unsigned long long ma = __ballot(f == 3u);
        if (t == 0u) {
            s.act_lo = (uint32_t)ma;
            s.act_hi = (uint32_t)(ma >> 32);
        }
    }
    for (uint32_t i = t; i < (3u * G - nv) * CS_LDW; i += 256u) s.u.rows[nv + i / CS_LDW][i % CS_LDW] = 0.f; // the last group's spare slots
    __syncthreads();
    const uint32_t act_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.act_lo), act_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.act_hi);
    const unsigned long long mact = ((unsigned long long)act_hi << 32) | act_lo;
    const uint32_t na = (uint32_t)__popcll(mact);

    // lane t's tile (gi <= gj), tiles numbered row after row of the upper triangle
    const bool mine = t < ntile;
    uint32_t gi = 0u, gj = 0u;
    if (mine) {
        uint32_t rem = t;
        while (rem >= G - gi) {
            rem -= G - gi;
            gi++;
        }
        gj = gi + rem;
    }
    double acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[a][c] = 0.0;

    for (uint32_t c0 = 0u; c0 < v.ld; c0 += CS_CH) {
        const uint32_t ncol = v.ld - c0 < CS_CH ? v.ld - c0 : CS_CH; // ld is a multiple of 16
        // the nodes' columns c0 .. c0 + 63: one 16-byte gather per lane and trip, zeros for an entry that is no node
        for (uint32_t it = t; it < cnt * LPR; it += 256u) {
            const uint32_t slot = it / LPR, part = it % LPR, c = c0 + part * E;
            float x[E];
#pragma unroll
            for (uint32_t j = 0; j < E; j++) x[j] = 0.f;
            if ((s.flag[slot] & 1u) && c < v.ld) kdb_decode16<PREC>(kdb_row_ptr16<PREC>(v, s.id[slot])[c / E], v.q_absmax, x);
#pragma unroll
            for (uint32_t j = 0; j < E; j += 4)
                *reinterpret_cast<float4 *>(&s.u.rows[slot][part * E + j]) = make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]);
        }
        if (t < CS_CH) { // the raw query (no alignment assumed), zeros behind dim
            const uint32_t c = c0 + t;
            s.u.rows[sqy][t] = (queries && c < v.dim) ? queries[b * v.dim + c] : 0.f;
        }
        __syncthreads();
        if (t < CS_CH) { // the centroid's columns: float32, node after node from 0, one correctly rounded divide (:139-146)
            float sum = 0.f;
            if (na == 1u) {
                sum = s.u.rows[__builtin_ctzll(mact)][t]; // "return 1.0, 0.0, nodes[0].Vector": the vector itself
            } else if (na > 1u) {
                for (unsigned long long m = mact; m; m &= m - 1ull) sum += s.u.rows[__builtin_ctzll(m)][t];
                sum = sum / (float)na;
            }
            s.u.rows[sc][t] = sum;
            if (out_centroid && c0 + t < v.dim) out_centroid[b * v.dim + c0 + t] = sum;
        }
        __syncthreads();
        if (mine) {
            for (uint32_t c = 0u; c < ncol; c += 4u) {
                float4 A[3], Bv[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    A[a] = *reinterpret_cast<const float4 *>(&s.u.rows[3u * gi + a][c]);
                    Bv[a] = *reinterpret_cast<const float4 *>(&s.u.rows[3u * gj + a][c]);
                }
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int d = 0; d < 3; d++) { // ascending columns into one accumulator; the product is exact, so fma rounds as mul + add
                        acc[a][d] = __builtin_fma((double)A[a].x, (double)Bv[d].x, acc[a][d]);
                        acc[a][d] = __builtin_fma((double)A[a].y, (double)Bv[d].y, acc[a][d]);
                        acc[a][d] = __builtin_fma((double)A[a].z, (double)Bv[d].z, acc[a][d]);
                        acc[a][d] = __builtin_fma((double)A[a].w, (double)Bv[d].w, acc[a][d]);
                    }
            }
        }
        __syncthreads(); // the next chunk overwrites the rows
    }

    // ---- epilogue: the accumulators go to LDS (over the rows), every lane picks what it needs
    if (mine) {
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int d = 0; d < 3; d++) s.u.acc[t][a * 3 + d] = acc[a][d];
    }
    __syncthreads();
    auto dot = [&](uint32_t x, uint32_t y) -> double { // slots x, y
        const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
        const uint32_t ti = lo / 3u, tj = hi / 3u;
        return s.u.acc[ti * G - ti * (ti - 1u) / 2u + (tj - ti)][(lo % 3u) * 3u + hi % 3u];
    };
    if (t < nv) s.sq[t] = sqrt(dot(t, t));
    __syncthreads();
    if (t < 64u) {
        double simv = -1.0;
        const uint32_t f = s.flag[t];
        if (f & 1u) simv = 1.0 - cs_cosine_distance(dot(t, sqy), dot(t, t), dot(sqy, sqy), s.sq[t], s.sq[sqy]); // epistemic.go:81
        if (out_sim && t < stride) out_sim[b * stride + t] = simv;
        if (f == 3u && na > 1u) {
            const double d = cs_cosine_distance(dot(t, sc), dot(t, t), dot(sc, sc), s.sq[t], s.sq[sc]);
            s.dsq[t] = d * d;
        }
    }
    double mx = 0.0; // maxVar (:158-166): `d > maxVar` from 0, so the order of the pairs does not matter and a NaN never wins
    if (na > 1u) {
        for (uint32_t p = t; p < cnt * 64u; p += 256u) {
            const uint32_t i = p >> 6, j = p & 63u;
            if (i < j && j < cnt && s.flag[i] == 3u && s.flag[j] == 3u) {
                const double d = cs_cosine_distance(dot(i, j), dot(i, i), dot(j, j), s.sq[i], s.sq[j]);
                if (d > mx) mx = d;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double other = __shfl_xor(mx, o, 64);
        if (other > mx) mx = other;
    }
    if ((t & 63u) == 0u) s.wmax[t >> 6] = mx;
    __syncthreads();
    if (t == 0u) {
        kdb_consensus r;
        r.score = 0.0;
        r.variance = 0.0;
        r.max_pair = 0.0;
        uint32_t nf = 0u;
        for (uint32_t i = 0; i < cnt; i++) nf += s.flag[i] & 1u;
        r.n_found = nf;
        r.n_active = na;
        if (na == 1u) r.score = 1.0;
        else if (na > 1u) {
            double sum = 0.0; // in list order (:149-153)
            for (unsigned long long m = mact; m; m &= m - 1ull) sum += s.dsq[__builtin_ctzll(m)];
            r.variance = sum / (double)na;
            double mv = 0.0;
            for (int w = 0; w < 4; w++)
                if (s.wmax[w] > mv) mv = s.wmax[w];
            r.max_pair = mv;
            if (mv < 1e-10) r.score = 1.0;
            else {
                double q = r.variance / (mv * mv);
                if (q > 1.0) q = 1.0; // math.Min(q, 1): a NaN stays
                r.score = 1.0 - q;
            }
        }
        out[b] = r;
    }
    if (out_gram) { // index `stride` is the centroid; whatever is not active is zero
        const uint32_t gw = stride + 1u;
        double *const g = out_gram + b * gw * gw;
        for (uint32_t p = t; p < gw * gw; p += 256u) {
            const uint32_t r = p / gw, c = p % gw;
            const bool okr = r == stride || (r < cnt && s.flag[r] == 3u), okc = c == stride || (c < cnt && s.flag[c] == 3u);
            g[p] = (okr && okc) ? dot(r == stride ? sc : r, c == stride ? sc : c) : 0.0;
        }
    }
}

} // namespace

int kdb_launch_consensus(const KdbView &v, const uint32_t *d_ids, const uint32_t *d_counts, uint32_t B, uint32_t stride, const float *d_queries,
                         const uint32_t *d_active, kdb_consensus *d_out, double *d_sim, float *d_centroid, double *d_gram, hipStream_t s) {
    if (B == 0) return KDB_OK;
    if (stride > KDB_CONSENSUS_MAX_K) {
        kdb_set_error("consensus: stride %u above KDB_CONSENSUS_MAX_K (%u)", stride, KDB_CONSENSUS_MAX_K);
        return KDB_ERR_INVALID;
    }
    const dim3 grid(B), block(256);
    if (v.precision == KDB_PREC_F32) hipLaunchKernelGGL(consensus_kernel<KDB_PREC_F32>, grid, block, 0, s, v, d_ids, d_counts, stride, d_queries, d_active, d_out, d_sim, d_centroid, d_gram);
    else if (v.precision == KDB_PREC_F16) hipLaunchKernelGGL(consensus_kernel<KDB_PREC_F16>, grid, block, 0, s, v, d_ids, d_counts, stride, d_queries, d_active, d_out, d_sim, d_centroid, d_gram);
    else if (v.precision == KDB_PREC_I8) hipLaunchKernelGGL(consensus_kernel<KDB_PREC_I8>, grid, block, 0, s, v, d_ids, d_counts, stride, d_queries, d_active, d_out, d_sim, d_centroid, d_gram);
    else {
        kdb_set_error("consensus: unsupported precision %u", v.precision);
        return KDB_ERR_UNSUPPORTED;
    }
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}
