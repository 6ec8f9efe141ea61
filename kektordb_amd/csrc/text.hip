// text.hip -- BM25 text search and hybrid fusion on the device (gfx950): bm25_topk_kernel restates DB.FindIDsByTextSearch
// (pkg/core/core.go:2069-2190) and the allow list of searchWithFusion (pkg/engine/ops.go:1013-1024), cut at k -- one workgroup per
// query, or one per part of its id space with bm25_merge_kernel behind them (kdb_text_split_plan); hybrid_fuse_kernel restates the
// fusion (ops.go:1072-1098, :1189-1207).  Geometry, LDS layout and the term arithmetic: kdb_text_plan.h.
#include "kdb_internal.h"
#include "kdb_text_plan.h"

namespace {

constexpr uint32_t NT = KDB_TEXT_BLOCK;
constexpr uint32_t NO_ID = 0xffffffffu; // the id of an empty entry (key 0): sorts behind every score

// (key, id) pairs in LDS into (score descending, id ascending) order: a bitonic network over n = 2^m entries, THREADS lanes
template <uint32_t THREADS>
__device__ __forceinline__ void text_sort(uint64_t *keys, uint32_t *ids, uint32_t n, uint32_t tid) {
    for (uint32_t size = 2; size <= n; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t p = tid; p < n / 2; p += THREADS) {
                const uint32_t i = 2u * p - (p & (stride - 1u)), j = i + stride;
                const uint64_t ka = keys[i], kb = keys[j];
                const uint32_t ia = ids[i], ib = ids[j];
                const bool a_first = kdb_text_before(ka, ia, kb, ib);
                if (((i & size) == 0u) != a_first) { // equal pairs (two empty entries) swap both ways: harmless
                    keys[i] = kb;
                    keys[j] = ka;
                    ids[i] = ib;
                    ids[j] = ia;
                }
            }
        }
    __syncthreads();
}

__device__ __forceinline__ uint32_t text_doc_len(const KdbTextDev &tx, uint32_t d) { return d <= tx.n_ids ? tx.doc_len[d] : 0u; }

// The running top-k of the sweep and of the merge (kdb_text_plan.h, GEOMETRY), the only copy: an array of N = kdb_text_sort_n(k)
// (key, id) pairs in LDS, its first k the sorted list, the rest the buffer of offers that beat the k-th entry.  room() is the
// buf_bound rule: the workgroup states how many offers the next pass can make at most, and when they might not fit the array is
// settled first -- sorted, cut at k, the k-th entry the threshold of later offers.  Every member but offer() is called by all lanes.
struct TextTopk {
    uint64_t *keys, *thr_key;
    uint32_t *ids, *words; // words: the 16 of the plan header (KDB_TEXT_W_BUF, KDB_TEXT_W_THR_ID, KDB_TEXT_W_NCAND ...)
    uint32_t k, N;
    uint32_t buf_bound;    // no more than this many offers sit in the buffer (uniform)

    __device__ __forceinline__ void init(uint32_t tid) { // the caller's barrier follows
        for (uint32_t i = tid; i < N; i += NT) {
            keys[i] = 0ull;
            ids[i] = NO_ID;
        }
        if (tid < 16u) words[tid] = tid == KDB_TEXT_W_THR_ID ? NO_ID : 0u;
        if (tid == 0u) *thr_key = 0ull;
        buf_bound = 0;
    }
    __device__ __forceinline__ void settle(uint32_t tid) {
        text_sort<NT>(keys, ids, N, tid);
        for (uint32_t i = k + tid; i < N; i += NT) {
            keys[i] = 0ull;
            ids[i] = NO_ID;
        }
        if (tid == 0u) {
            words[KDB_TEXT_W_BUF] = 0u;
            *thr_key = keys[k - 1u];
            words[KDB_TEXT_W_THR_ID] = ids[k - 1u];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void room(uint32_t n_pass, uint32_t tid) { // n_pass <= NT <= N - k
        if (buf_bound + n_pass > N - k) {
            settle(tid);
            buf_bound = 0;
        }
        buf_bound += n_pass;
    }
    __device__ __forceinline__ void offer(uint64_t key, uint32_t d) {
        if (kdb_text_before(key, d, *thr_key, words[KDB_TEXT_W_THR_ID])) {
            const uint32_t at = k + atomicAdd(&words[KDB_TEXT_W_BUF], 1u); // < k + buf_bound <= N
            keys[at] = key;
            ids[at] = d;
        }
    }
    // behind the last settle: the answer of query b, ncand candidates in all
    __device__ __forceinline__ void answer(uint32_t b, uint32_t ncand, uint32_t tid, uint32_t *__restrict__ out_ids, double *__restrict__ out_score,
                                           uint32_t *__restrict__ out_count, double *__restrict__ out_max, uint32_t *__restrict__ out_ncand) const {
        const uint32_t cnt = ncand < k ? ncand : k;
        for (uint32_t j = tid; j < k; j += NT) {
            out_ids[(size_t)b * k + j] = j < cnt ? ids[j] : 0u;
            out_score[(size_t)b * k + j] = j < cnt ? __longlong_as_double((long long)kdb_text_unkey(keys[j])) : 0.0;
        }
        if (tid == 0u) {
            out_count[b] = cnt;
            if (out_max) out_max[b] = cnt ? __longlong_as_double((long long)kdb_text_unkey(keys[0])) : 0.0;
            if (out_ncand) out_ncand[b] = ncand;
        }
    }
};

// SPLIT = false: one workgroup per query, grid (B).  SPLIT = true: grid (parts, B), workgroup (s, b) sweeps the ids of
// [bnd(s), bnd(s + 1)) (kdb_text_split_bound) and leaves its list in record b * parts + s of `part_out` (kdb_text_parts) instead of
// the answer.  Cursors only move forward; terms are applied one after another with a barrier between them, so inside a term every
// document of the tile is touched by one lane only and a plain LDS read-add-write has no conflicts -- and the additions come in
// query order, the reference's (core.go:2142-2146).
template <bool SPLIT>
__global__ __launch_bounds__(KDB_TEXT_BLOCK) void bm25_topk_kernel(KdbTextDev tx, const uint32_t *__restrict__ tokens, const uint32_t *__restrict__ n_tokens,
                                                                    uint32_t t_stride, uint32_t k, const uint32_t *__restrict__ allow, uint32_t count,
                                                                    uint32_t *__restrict__ out_ids, double *__restrict__ out_score,
                                                                    uint32_t *__restrict__ out_count, double *__restrict__ out_max,
                                                                    uint32_t *__restrict__ out_ncand, unsigned char *__restrict__ part_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const KdbTextLds L = kdb_text_lds(k);
    double *const score = reinterpret_cast<double *>(lds + L.o_score);
    uint64_t *const cur = reinterpret_cast<uint64_t *>(lds + L.o_cur);
    uint64_t *const end = reinterpret_cast<uint64_t *>(lds + L.o_end);
    double *const idf = reinterpret_cast<double *>(lds + L.o_idf);
    uint32_t *const dlen = reinterpret_cast<uint32_t *>(lds + L.o_len);
    uint32_t *const touched = reinterpret_cast<uint32_t *>(lds + L.o_touched);
    uint32_t *const words = reinterpret_cast<uint32_t *>(lds + L.o_words);
    TextTopk tk{reinterpret_cast<uint64_t *>(lds + L.o_keys), reinterpret_cast<uint64_t *>(lds + L.o_thr), reinterpret_cast<uint32_t *>(lds + L.o_ids), words, k,
                kdb_text_sort_n(k), 0u};
    const uint32_t tid = threadIdx.x, b = SPLIT ? blockIdx.y : blockIdx.x;
    uint32_t T = n_tokens[b];
    if (T > t_stride) T = t_stride;
    if (T > KDB_TEXT_MAX_TOKENS) T = KDB_TEXT_MAX_TOKENS;

    for (uint32_t i = tid; i < KDB_TEXT_TILE; i += NT) score[i] = 0.0;
    tk.init(tid);
    if (tid < KDB_TEXT_TILE / 32u) touched[tid] = 0u;
    if (tid < KDB_TEXT_MAX_TOKENS) {
        uint64_t c = 0, e = 0;
        double w = 0.0;
        if (tid < T) {
            const uint32_t tok = tokens[(size_t)b * t_stride + tid];
            if (tok < tx.n_tokens) { // KDB_NO_TOKEN and every id the dictionary does not hold: no list
                c = tx.post_off[tok];
                e = tx.post_off[tok + 1u];
                w = tx.idf[tok];
            }
        }
        cur[tid] = c;
        end[tid] = e;
        idf[tid] = w;
    }
    __syncthreads();
    if constexpr (SPLIT) { // lane t narrows token t's list to the part's id range: two lower bounds by binary search
        uint64_t c = 0, e = 0;
        if (tid < KDB_TEXT_MAX_TOKENS) {
            const KdbTextSpan sp = kdb_text_longest(cur, end, T);
            const uint64_t lo = kdb_text_split_bound(tx.post_doc, sp, gridDim.x, blockIdx.x), hi = kdb_text_split_bound(tx.post_doc, sp, gridDim.x, blockIdx.x + 1u);
            c = kdb_text_lower_bound(tx.post_doc, cur[tid], end[tid], lo);
            e = kdb_text_lower_bound(tx.post_doc, c, end[tid], hi);
        }
        __syncthreads(); // every lane has read the whole lists
        if (tid < KDB_TEXT_MAX_TOKENS) {
            cur[tid] = c;
            end[tid] = e;
        }
        __syncthreads();
    }

    uint32_t run = 0;     // posting runs so far: run r counts in words[r % 3], cleared during run r - 1
    uint32_t my_cand = 0; // candidates this lane has seen
    for (;;) {
        // the next tile: the one that holds the smallest id under any cursor (an empty stretch of the id space costs nothing)
        if (tid < 64u) {
            uint32_t head = NO_ID;
            if (tid < T && cur[tid] < end[tid]) head = tx.post_doc[cur[tid]];
            for (int o = 32; o; o >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)head, o);
                head = other < head ? other : head;
            }
            if (tid == 0u) words[KDB_TEXT_W_HEAD] = head;
        }
        __syncthreads();
        const uint32_t head = words[KDB_TEXT_W_HEAD];
        if (head == NO_ID) break;
        const uint32_t base = head & ~(KDB_TEXT_TILE - 1u);
        const uint64_t tile_end = (uint64_t)base + KDB_TEXT_TILE;
        for (uint32_t t = 0; t < T; t++) {
            uint64_t c = cur[t];
            const uint64_t e = end[t];
            const double w = idf[t];
            for (;;) { // runs of NT consecutive (doc, tf) entries; the entries inside the tile are a prefix of the run
                uint32_t *const ctr = words + run % 3u;
                if (tid == 0u) words[(run + 1u) % 3u] = 0u;
                const uint64_t i = c + tid;
                bool in = false;
                if (i < e) {
                    const uint32_t d = tx.post_doc[i];
                    if ((uint64_t)d < tile_end && d >= base) { // (d >= base always: the cursors are behind every earlier tile)
                        in = true;
                        const uint32_t tf = tx.post_tf[i], slot = d - base, bit = 1u << (slot & 31u);
                        uint32_t dl;
                        if (!(atomicOr(&touched[slot >> 5], bit) & bit)) { // first touch: the length is gathered once per document
                            dl = text_doc_len(tx, d);
                            dlen[slot] = dl;
                        } else {
                            dl = dlen[slot];
                        }
                        score[slot] = score[slot] + kdb_bm25_term(w, tf, dl, tx.avg_len);
                    }
                }
                const uint32_t n_wave = (uint32_t)__popcll(__ballot(in));
                if ((tid & 63u) == 0u && n_wave) atomicAdd(ctr, n_wave);
                __syncthreads(); // ... which is also the barrier between this term's additions and the next term's
                const uint32_t n = *ctr;
                run++;
                c += n;
                if (n < NT) break;
            }
            if (tid == 0u) cur[t] = c;
        }
        // the tile is complete: its touched and allowed documents are offered to the running top-k
        for (uint32_t p = 0; p < KDB_TEXT_TILE / NT; p++) {
            uint32_t n_pass = 0;
            for (uint32_t j = 0; j < NT / 32u; j++) n_pass += (uint32_t)__popc(touched[p * (NT / 32u) + j]);
            if (!n_pass) continue;
            tk.room(n_pass, tid);
            const uint32_t slot = p * NT + tid;
            if ((touched[slot >> 5] >> (slot & 31u)) & 1u) {
                const uint32_t d = base + slot;
                const double sc = score[slot];
                score[slot] = 0.0;
                if (!allow || (d <= count && ((allow[d >> 5] >> (d & 31u)) & 1u))) {
                    my_cand++;
                    tk.offer(kdb_text_key((uint64_t)__double_as_longlong(sc)), d);
                }
            }
        }
        __syncthreads();
        if (tid < KDB_TEXT_TILE / 32u) touched[tid] = 0u;
        __syncthreads();
    }
    if (my_cand) atomicAdd(&words[KDB_TEXT_W_NCAND], my_cand);
    tk.settle(tid);
    const uint32_t ncand = words[KDB_TEXT_W_NCAND];
    if constexpr (SPLIT) { // the part's first min(k, ncand) entries, its count and its candidates
        const KdbTextParts P = kdb_text_parts(gridDim.y, gridDim.x, k);
        const uint64_t r = (uint64_t)b * gridDim.x + blockIdx.x;
        const uint32_t cnt = ncand < k ? ncand : k;
        uint64_t *const p_keys = reinterpret_cast<uint64_t *>(part_out + P.o_keys) + r * k;
        uint32_t *const p_ids = reinterpret_cast<uint32_t *>(part_out + P.o_ids) + r * k, *const p_counts = reinterpret_cast<uint32_t *>(part_out + P.o_counts) + r * 2u;
        for (uint32_t j = tid; j < cnt; j += NT) {
            p_keys[j] = tk.keys[j];
            p_ids[j] = tk.ids[j];
        }
        if (tid == 0u) {
            p_counts[0] = cnt;
            p_counts[1] = ncand;
        }
    } else {
        tk.answer(b, ncand, tid, out_ids, out_score, out_count, out_max, out_ncand);
    }
}

// One workgroup per query behind bm25_topk_kernel<true>: the `parts` lists of the query are offered to one more top-k array.  The
// records of a query lie side by side, so slot e of the query is entry e % k of part e / k: a pass takes 256 slots, and a slot
// beyond its part's count offers nothing.
__global__ __launch_bounds__(KDB_TEXT_BLOCK) void bm25_merge_kernel(const unsigned char *__restrict__ part_in, uint32_t parts, uint32_t k,
                                                                     uint32_t *__restrict__ out_ids, double *__restrict__ out_score,
                                                                     uint32_t *__restrict__ out_count, double *__restrict__ out_max,
                                                                     uint32_t *__restrict__ out_ncand) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const KdbTextMergeLds L = kdb_text_merge_lds(k);
    uint32_t *const words = reinterpret_cast<uint32_t *>(lds + L.o_words);
    TextTopk tk{reinterpret_cast<uint64_t *>(lds + L.o_keys), reinterpret_cast<uint64_t *>(lds + L.o_thr), reinterpret_cast<uint32_t *>(lds + L.o_ids), words, k,
                kdb_text_sort_n(k), 0u};
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const KdbTextParts P = kdb_text_parts(gridDim.x, parts, k);
    const uint64_t r0 = (uint64_t)b * parts;
    const uint64_t *const p_keys = reinterpret_cast<const uint64_t *>(part_in + P.o_keys) + r0 * k;
    const uint32_t *const p_ids = reinterpret_cast<const uint32_t *>(part_in + P.o_ids) + r0 * k, *const p_counts = reinterpret_cast<const uint32_t *>(part_in + P.o_counts) + r0 * 2u;
    tk.init(tid);
    __syncthreads();
    uint32_t my_cand = 0;
    for (uint32_t s = tid; s < parts; s += NT) my_cand += p_counts[2u * s + 1u]; // the parts partition the ids: the sum is below 2^30
    if (my_cand) atomicAdd(&words[KDB_TEXT_W_NCAND], my_cand);
    const uint32_t slots = parts * k; // <= 512 * 1024
    for (uint32_t e0 = 0; e0 < slots; e0 += NT) {
        tk.room(slots - e0 < NT ? slots - e0 : NT, tid);
        const uint32_t e = e0 + tid;
        if (e < slots && e % k < p_counts[2u * (e / k)]) tk.offer(p_keys[e], p_ids[e]);
    }
    tk.settle(tid);
    tk.answer(b, words[KDB_TEXT_W_NCAND], tid, out_ids, out_score, out_count, out_max, out_ncand);
}

// One wave per query: vector answers first (their raw text score found by binary search in the query's lists, summed by the routine
// the text kernel uses), then the text answers the vector list does not hold, then one sort of the union and the cut at k.
__global__ __launch_bounds__(64) void hybrid_fuse_kernel(KdbTextDev tx, const uint32_t *__restrict__ tokens, const uint32_t *__restrict__ n_tokens, uint32_t t_stride,
                                                         uint32_t k, double alpha, uint32_t one_minus_dot, const uint32_t *__restrict__ v_ids,
                                                         const float *__restrict__ v_dist, const uint32_t *__restrict__ v_cnt, const uint32_t *__restrict__ t_ids,
                                                         const double *__restrict__ t_score, const uint32_t *__restrict__ t_cnt, const double *__restrict__ t_max,
                                                         uint32_t *__restrict__ out_ids, double *__restrict__ out_score, uint32_t *__restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t N = kdb_fuse_sort_n(k);
    uint64_t *const keys = reinterpret_cast<uint64_t *>(lds);
    uint64_t *const lo = keys + N, *const hi = lo + KDB_TEXT_MAX_TOKENS;
    double *const idf = reinterpret_cast<double *>(hi + KDB_TEXT_MAX_TOKENS);
    uint32_t *const ids = reinterpret_cast<uint32_t *>(idf + KDB_TEXT_MAX_TOKENS);
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    uint32_t T = n_tokens[b];
    if (T > t_stride) T = t_stride;
    if (T > KDB_TEXT_MAX_TOKENS) T = KDB_TEXT_MAX_TOKENS;
    const bool hybrid = T != 0u; // textQuery == "" takes the vector-only rule (ops.go:1083-1086)
    uint32_t nv = v_cnt[b] & KDB_COUNT_MASK, nt = hybrid ? t_cnt[b] : 0u;
    if (nv > k) nv = k;
    if (nt > k) nt = k;
    const double tmax = hybrid ? t_max[b] : 0.0;
    if (tid < KDB_TEXT_MAX_TOKENS) {
        uint64_t c = 0, e = 0;
        double w = 0.0;
        if (tid < T) {
            const uint32_t tok = tokens[(size_t)b * t_stride + tid];
            if (tok < tx.n_tokens) {
                c = tx.post_off[tok];
                e = tx.post_off[tok + 1u];
                w = tx.idf[tok];
            }
        }
        lo[tid] = c;
        hi[tid] = e;
        idf[tid] = w;
    }
    for (uint32_t i = tid; i < N; i += 64u) {
        keys[i] = 0ull;
        ids[i] = NO_ID;
    }
    __syncthreads();
    for (uint32_t j = tid; j < nv; j += 64u) {
        const uint32_t d = v_ids[(size_t)b * k + j];
        const double dist = (double)v_dist[(size_t)b * k + j];
        const double v = 1.0 / (1.0 + (one_minus_dot ? 1.0 - dist : dist)); // normalizeVectorScores
        double fused = v;
        if (hybrid) {
            double raw = 0.0;
            bool in_text = false;
            for (uint32_t t = 0; t < T; t++) { // lower bound of d in token t's list
                uint64_t a = lo[t], z = hi[t];
                const uint64_t e = z;
                while (a < z) {
                    const uint64_t m = a + ((z - a) >> 1);
                    if (tx.post_doc[m] < d) a = m + 1u;
                    else z = m;
                }
                if (a < e && tx.post_doc[a] == d) {
                    in_text = true;
                    raw = raw + kdb_bm25_term(idf[t], tx.post_tf[a], text_doc_len(tx, d), tx.avg_len);
                }
            }
            fused = alpha * v;
            if (in_text) fused = fused + (1.0 - alpha) * (tmax > 0.0 ? raw / tmax : raw);
        }
        keys[j] = kdb_text_key((uint64_t)__double_as_longlong(fused));
        ids[j] = d;
    }
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += 64u) {
        const uint32_t d = t_ids[(size_t)b * k + j];
        bool dup = false;
        for (uint32_t i = 0; i < nv; i++) dup |= ids[i] == d;
        if (dup) continue; // scored with the vector list
        const double raw = t_score[(size_t)b * k + j];
        const double fused = (1.0 - alpha) * (tmax > 0.0 ? raw / tmax : raw);
        keys[nv + j] = kdb_text_key((uint64_t)__double_as_longlong(fused));
        ids[nv + j] = d;
    }
    text_sort<64u>(keys, ids, N, tid);
    uint32_t n_mine = 0;
    for (uint32_t i = tid; i < N; i += 64u) n_mine += ids[i] != NO_ID;
    for (int o = 32; o; o >>= 1) n_mine += (uint32_t)__shfl_xor((int)n_mine, o);
    const uint32_t cnt = n_mine < k ? n_mine : k;
    for (uint32_t j = tid; j < k; j += 64u) {
        out_ids[(size_t)b * k + j] = j < cnt ? ids[j] : 0u;
        out_score[(size_t)b * k + j] = j < cnt ? __longlong_as_double((long long)kdb_text_unkey(keys[j])) : 0.0;
    }
    if (tid == 0u) out_count[b] = cnt;
}

} // namespace

int kdb_launch_bm25_topk(const KdbTextDev &tx, const uint32_t *d_tokens, const uint32_t *d_n_tokens, uint32_t B, uint32_t t_stride, uint32_t k,
                         const uint32_t *d_allow, uint32_t count, uint32_t *d_out_ids, double *d_out_score, uint32_t *d_out_count, double *d_max,
                         uint32_t *d_ncand, const KdbTextSplitPlan &plan, void *d_parts, hipStream_t s) {
    if (B == 0) return KDB_OK;
    const uint32_t lds = kdb_text_lds(k).total;
    if (plan.parts <= 1u) {
        KDB_HIP(hipFuncSetAttribute((const void *)bm25_topk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(bm25_topk_kernel<false>, dim3(B), dim3(KDB_TEXT_BLOCK), lds, s, tx, d_tokens, d_n_tokens, t_stride, k, d_allow, count, d_out_ids,
                           d_out_score, d_out_count, d_max, d_ncand, (unsigned char *)nullptr);
        KDB_HIP(hipGetLastError());
        return KDB_OK;
    }
    if (!d_parts) {
        kdb_set_error("bm25_topk: a split launch without room for its partial lists");
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipFuncSetAttribute((const void *)bm25_topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    KDB_HIP(hipFuncSetAttribute((const void *)bm25_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.merge_lds));
    hipLaunchKernelGGL(bm25_topk_kernel<true>, dim3(plan.parts, B), dim3(KDB_TEXT_BLOCK), lds, s, tx, d_tokens, d_n_tokens, t_stride, k, d_allow, count,
                       (uint32_t *)nullptr, (double *)nullptr, (uint32_t *)nullptr, (double *)nullptr, (uint32_t *)nullptr, static_cast<unsigned char *>(d_parts));
    KDB_HIP(hipGetLastError());
    hipLaunchKernelGGL(bm25_merge_kernel, dim3(B), dim3(KDB_TEXT_BLOCK), plan.merge_lds, s, static_cast<const unsigned char *>(d_parts), plan.parts, k,
                       d_out_ids, d_out_score, d_out_count, d_max, d_ncand);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}

int kdb_launch_hybrid_fuse(const KdbTextDev &tx, const uint32_t *d_tokens, const uint32_t *d_n_tokens, uint32_t B, uint32_t t_stride, uint32_t k,
                           double alpha, uint32_t one_minus_dot, const uint32_t *d_v_ids, const float *d_v_dist, const uint32_t *d_v_cnt,
                           const uint32_t *d_t_ids, const double *d_t_score, const uint32_t *d_t_cnt, const double *d_t_max, uint32_t *d_out_ids,
                           double *d_out_score, uint32_t *d_out_count, hipStream_t s) {
    if (B == 0) return KDB_OK;
    const uint32_t lds = kdb_fuse_lds_bytes(k);
    KDB_HIP(hipFuncSetAttribute((const void *)hybrid_fuse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(hybrid_fuse_kernel, dim3(B), dim3(64), lds, s, tx, d_tokens, d_n_tokens, t_stride, k, alpha, one_minus_dot, d_v_ids, d_v_dist, d_v_cnt,
                       d_t_ids, d_t_score, d_t_cnt, d_t_max, d_out_ids, d_out_score, d_out_count);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}
