// kdb_text_plan.h -- the plan of bm25_topk_kernel and hybrid_fuse_kernel (text.hip): tile geometry, the LDS layout sized from k, the
// BM25 term both kernels add, and the validation of an uploaded snapshot and of a call's arguments.  Shared by the host
// (kdb_api_text.hip validates and sizes launches with it) and the kernels (which index with it).  Plain C++, no HIP header.
//
// GEOMETRY.  One workgroup of KDB_TEXT_BLOCK lanes per query.  The id space is swept in tiles of KDB_TEXT_TILE ids; a tile's scores
// are KDB_TEXT_TILE doubles in LDS, beside them the document lengths gathered at first touch and a touched bit per id.  The running
// top-k is ONE array of kdb_text_sort_n(k) (key, id) pairs: the first k are the sorted list, the rest the buffer of offers that beat
// the current k-th key; when the buffer cannot take another pass of offers the whole array is sorted again (bitonic, in place).
#ifndef KDB_TEXT_PLAN_H
#define KDB_TEXT_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include "../../include/kektor_hip.h"

#if defined(__HIPCC__)
#define KDB_TEXT_HD __host__ __device__
#else
#define KDB_TEXT_HD
#endif

constexpr uint32_t KDB_TEXT_TILE = 4096u;   // ids per tile
constexpr uint32_t KDB_TEXT_BLOCK = 256u;   // lanes per query
constexpr uint32_t KDB_TEXT_MAX_K = 1024u;
constexpr uint32_t KDB_TEXT_MAX_ID = 0x3fffffffu; // "Conventions": at most 2^30 - 1 ids per index
constexpr uint32_t KDB_TEXT_LDS_LIMIT = 160u * 1024u;
static_assert(KDB_TEXT_TILE % KDB_TEXT_BLOCK == 0u && KDB_TEXT_BLOCK % 32u == 0u, "whole passes per tile, whole touched words per pass");
static_assert(KDB_TEXT_MAX_TOKENS <= 32u, "the heads of a query's lists are reduced by one wave");

KDB_TEXT_HD constexpr uint32_t kdb_text_pow2(uint32_t k) {
    uint32_t p = 1;
    while (p < k) p <<= 1;
    return p;
}
// entries of the top-k array: a power of two (bitonic sort) with room for the list and at least one pass of offers behind it
KDB_TEXT_HD constexpr uint32_t kdb_text_sort_n(uint32_t k) { return 2u * kdb_text_pow2(k) < 2u * KDB_TEXT_BLOCK ? 2u * KDB_TEXT_BLOCK : 2u * kdb_text_pow2(k); }
KDB_TEXT_HD constexpr uint32_t kdb_text_buffer(uint32_t k) { return kdb_text_sort_n(k) - k; }
static_assert(kdb_text_buffer(1) >= KDB_TEXT_BLOCK && kdb_text_buffer(256) >= KDB_TEXT_BLOCK && kdb_text_buffer(257) >= KDB_TEXT_BLOCK &&
              kdb_text_buffer(KDB_TEXT_MAX_K) >= KDB_TEXT_BLOCK, "the buffer takes the offers of one pass");

// LDS of bm25_topk_kernel, byte offsets (every region 8-byte aligned):
//   scores [TILE] f64 | keys [N] u64 | cursors [32] u64 | list ends [32] u64 | idf [32] f64 | threshold key u64 |
//   doc lengths [TILE] u32 | ids [N] u32 | touched [TILE / 32] u32 | words [16] u32
struct KdbTextLds {
    uint32_t o_score, o_keys, o_cur, o_end, o_idf, o_thr, o_len, o_ids, o_touched, o_words, total;
};
enum { KDB_TEXT_W_RUN0 = 0 /* .. 2: posting-run counters, rotating */, KDB_TEXT_W_BUF = 3, KDB_TEXT_W_NCAND = 4, KDB_TEXT_W_HEAD = 5, KDB_TEXT_W_THR_ID = 6 };
KDB_TEXT_HD constexpr KdbTextLds kdb_text_lds(uint32_t k) {
    KdbTextLds L{};
    const uint32_t n = kdb_text_sort_n(k);
    L.o_score = 0;
    L.o_keys = L.o_score + KDB_TEXT_TILE * 8u;
    L.o_cur = L.o_keys + n * 8u;
    L.o_end = L.o_cur + KDB_TEXT_MAX_TOKENS * 8u;
    L.o_idf = L.o_end + KDB_TEXT_MAX_TOKENS * 8u;
    L.o_thr = L.o_idf + KDB_TEXT_MAX_TOKENS * 8u;
    L.o_len = L.o_thr + 8u;
    L.o_ids = L.o_len + KDB_TEXT_TILE * 4u;
    L.o_touched = L.o_ids + n * 4u;
    L.o_words = L.o_touched + KDB_TEXT_TILE / 32u * 4u;
    L.total = L.o_words + 16u * 4u;
    return L;
}
static_assert(kdb_text_lds(KDB_TEXT_MAX_K).total <= KDB_TEXT_LDS_LIMIT, "bm25_topk_kernel fits a CU's LDS at the largest k");
// LDS of hybrid_fuse_kernel (one wave): keys [N] u64 | cursors, ends, idf [32] each | ids [N] u32, N = 2 * pow2(k) >= 2k
KDB_TEXT_HD constexpr uint32_t kdb_fuse_sort_n(uint32_t k) { return 2u * kdb_text_pow2(k); }
KDB_TEXT_HD constexpr uint32_t kdb_fuse_lds_bytes(uint32_t k) { return kdb_fuse_sort_n(k) * 12u + 3u * KDB_TEXT_MAX_TOKENS * 8u; }
static_assert(kdb_fuse_lds_bytes(KDB_TEXT_MAX_K) <= KDB_TEXT_LDS_LIMIT, "hybrid_fuse_kernel fits a CU's LDS at the largest k");

// ---- one query on many workgroups -------------------------------------------------------------------------------------------------
// bm25_topk_kernel<true> on a grid of (parts, B): workgroup (s, b) sweeps the ids of [bnd(s), bnd(s + 1)) of query b and leaves its
// own top-k, its count and its candidates in HBM; bm25_merge_kernel, one workgroup per query behind it on the same stream, offers the
// partial lists to one more top-k array and writes the answer.  The order (key descending, id ascending) is total and every part's
// list is its own top-k, so the merged answer is the one-workgroup answer bit for bit.
constexpr uint32_t KDB_TEXT_MAX_PARTS = 512u;
constexpr uint32_t KDB_TEXT_MIN_TILES_PER_PART = 1u;   // measured: one query over 245 tiles was fastest at a part per tile
constexpr uint64_t KDB_TEXT_SPLIT_MIN_POSTINGS = 64u;  // measured: from 64 postings up the split was faster in every class; at
                                                       // 16 and 32 the prologue and the second launch cost more than the few tiles they spread
constexpr uint32_t KDB_TEXT_WG_PER_CU = 2u;                  // the LDS budget above: two workgroups per CU

struct KdbTextSplitIn {
    uint32_t B, k, n_ids, n_cus;
    uint64_t postings_bound; // no query of the call sweeps more postings than this
    int32_t forced;          // KDB_TEXT_SPLIT: < 0 unset, 0 never split, N >= 1 exactly N parts (capped by the tiles and KDB_TEXT_MAX_PARTS)
};
struct KdbTextSplitPlan {
    uint32_t parts;         // 1: bm25_topk_kernel<false>, one workgroup per query, no scratch and no merge
    uint64_t scratch_bytes; // the partial lists (0 when parts == 1)
    uint32_t merge_lds;     // LDS of bm25_merge_kernel
};
// LDS of bm25_merge_kernel, the top-k array alone: keys [N] u64 | threshold key u64 | ids [N] u32 | words [16] u32
struct KdbTextMergeLds {
    uint32_t o_keys, o_thr, o_ids, o_words, total;
};
KDB_TEXT_HD constexpr KdbTextMergeLds kdb_text_merge_lds(uint32_t k) {
    KdbTextMergeLds L{};
    const uint32_t n = kdb_text_sort_n(k);
    L.o_keys = 0;
    L.o_thr = n * 8u;
    L.o_ids = L.o_thr + 8u;
    L.o_words = L.o_ids + n * 4u;
    L.total = L.o_words + 16u * 4u;
    return L;
}
static_assert(kdb_text_merge_lds(KDB_TEXT_MAX_K).total <= KDB_TEXT_LDS_LIMIT, "bm25_merge_kernel fits a CU's LDS at the largest k");
// The partial lists, R = B * parts records, record r = b * parts + s: keys [R][k] u64 | (count, candidates) [R][2] u32 | ids [R][k] u32
// -- 12 k + 8 bytes a record, every array on an 8-byte boundary, the whole rounded up to one.
struct KdbTextParts {
    uint64_t o_keys, o_counts, o_ids, total;
};
KDB_TEXT_HD constexpr KdbTextParts kdb_text_parts(uint32_t B, uint32_t parts, uint32_t k) {
    KdbTextParts P{};
    const uint64_t R = (uint64_t)B * parts;
    P.o_keys = 0;
    P.o_counts = R * k * 8u;
    P.o_ids = P.o_counts + R * 8u;
    P.total = (P.o_ids + R * k * 4u + 7u) & ~7ull; // = R * (12 k + 8), rounded up
    return P;
}
KDB_TEXT_HD constexpr uint32_t kdb_text_tiles(uint32_t n_ids) { return (uint32_t)(((uint64_t)n_ids + 1u + KDB_TEXT_TILE - 1u) / KDB_TEXT_TILE); }
KDB_TEXT_HD constexpr KdbTextSplitPlan kdb_text_split_plan(const KdbTextSplitIn &in) {
    const uint32_t tiles = kdb_text_tiles(in.n_ids);
    uint32_t parts = 1;
    if (in.forced > 0) {
        parts = (uint32_t)in.forced < tiles ? (uint32_t)in.forced : tiles; // one tile per part at least
    } else if (in.forced < 0 && in.B && in.postings_bound >= KDB_TEXT_SPLIT_MIN_POSTINGS) {
        parts = (uint32_t)(((uint64_t)KDB_TEXT_WG_PER_CU * in.n_cus + in.B - 1u) / in.B); // about two workgroups per CU for the whole call
        if (parts > tiles / KDB_TEXT_MIN_TILES_PER_PART) parts = tiles / KDB_TEXT_MIN_TILES_PER_PART;
    }
    if (parts > KDB_TEXT_MAX_PARTS) parts = KDB_TEXT_MAX_PARTS;
    if (parts < 2u || in.B > 65535u) parts = 1; // (the queries are the grid's second dimension)
    return KdbTextSplitPlan{parts, parts > 1u ? kdb_text_parts(in.B, parts, in.k).total : 0ull, kdb_text_merge_lds(in.k).total};
}
// The boundaries balance POSTINGS, not ids (documents arrive in time order and rare words cluster: equal id ranges would leave most
// parts empty).  They are cut from the query's LONGEST list, postings [a, a + len) -- among equal lengths the earliest token --:
//   bnd(0) = 0, bnd(parts) = 2^32 (past every id), bnd(s) = post_doc[a + floor(s * len / parts)] rounded down to a tile.
// Non-decreasing; equal bounds make an empty part; the ranges partition the id space, and a tile lies inside one part.  Every part
// computes both of its bounds with this routine, so the parts of a query agree.  len == 0 (no list at all): nothing is read.
struct KdbTextSpan {
    uint64_t a, len;
};
KDB_TEXT_HD inline KdbTextSpan kdb_text_longest(const uint64_t *lo, const uint64_t *hi, uint32_t T) {
    KdbTextSpan sp{0, 0};
    for (uint32_t t = 0; t < T; t++)
        if (hi[t] - lo[t] > sp.len) sp = KdbTextSpan{lo[t], hi[t] - lo[t]};
    return sp;
}
KDB_TEXT_HD inline uint64_t kdb_text_split_bound(const uint32_t *post_doc, KdbTextSpan sp, uint32_t parts, uint32_t s) {
    if (s == 0u || sp.len == 0u) return s >= parts ? 1ull << 32 : 0ull;
    if (s >= parts) return 1ull << 32;
    return post_doc[sp.a + (uint64_t)s * sp.len / parts] & ~(KDB_TEXT_TILE - 1u); // s < 512, len < 2^40: no overflow
}
// the first posting of [lo, hi) whose document is not below `bound`
KDB_TEXT_HD inline uint64_t kdb_text_lower_bound(const uint32_t *post_doc, uint64_t lo, uint64_t hi, uint64_t bound) {
    while (lo < hi) {
        const uint64_t m = lo + ((hi - lo) >> 1);
        if ((uint64_t)post_doc[m] < bound) lo = m + 1u;
        else hi = m;
    }
    return lo;
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
// calculateBM25TermScore (pkg/core/core.go:2159-2190) for a token the document holds (tf >= 1): the operations and their order are
// the reference's, in double; the library is built with -ffp-contract=off, so no multiply-add is fused.
KDB_TEXT_HD inline double kdb_bm25_term(double idf, uint32_t tf, uint32_t doc_len, double avg_len) {
    if (!(avg_len > 0.0)) return 0.0; // :2173
    const double t = (double)tf;
    return idf * ((t * 2.2) / (t + 1.2 * (0.25 + 0.75 * ((double)doc_len / avg_len))));
}
// :2178-2179 with math.Log restated as std::log (the caller who wants Go's bits passes its own table)
inline double kdb_bm25_idf(uint64_t total_docs, uint64_t df) { return std::log(1 + ((double)total_docs - (double)df + 0.5) / ((double)df + 0.5)); }
// scores ordered as unsigned keys: a larger double is a larger key, for every double that is not a NaN; key 0 is no score at all
KDB_TEXT_HD inline uint64_t kdb_text_key(uint64_t score_bits) { return (score_bits >> 63) ? ~score_bits : score_bits | 0x8000000000000000ull; }
KDB_TEXT_HD inline uint64_t kdb_text_unkey(uint64_t key) { return (key >> 63) ? key & 0x7fffffffffffffffull : ~key; }
// (score descending, id ascending): a total order, ids being distinct
KDB_TEXT_HD inline bool kdb_text_before(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka > kb || (ka == kb && ia < ib); }

// ---- validation -------------------------------------------------------------------------------------------------------------------
enum {
    KDB_TEXT_OK = 0,
    KDB_TEXT_BAD_VIEW = 1,   // a null array, n_ids above 2^30 - 1, post_off not starting at 0 or descending
    KDB_TEXT_BAD_ORDER = 2,  // a list that is not strictly ascending
    KDB_TEXT_BAD_ID = 3,     // an id that is 0, above n_ids or above the index's capacity
    KDB_TEXT_BAD_TF = 4,     // a term frequency of 0
    KDB_TEXT_BAD_DF = 5,     // a list longer than total_docs
    KDB_TEXT_BAD_AVG = 6,    // avg_len negative or not finite
    KDB_TEXT_BAD_IDF = 7     // an idf that is not finite
};
// cap: the capacity of the index the snapshot is for.  *bad_token: the token at which the check failed.
inline int kdb_text_validate_view(const kdb_text_view *v, uint32_t cap, uint32_t *bad_token) {
    if (bad_token) *bad_token = 0;
    if (!v || !v->post_off || !v->doc_len || v->n_ids > KDB_TEXT_MAX_ID || v->n_tokens == KDB_NO_TOKEN || v->post_off[0] != 0u) return KDB_TEXT_BAD_VIEW;
    if (!(v->avg_len >= 0.0) || std::isinf(v->avg_len)) return KDB_TEXT_BAD_AVG;
    for (uint32_t t = 0; t < v->n_tokens; t++) {
        if (bad_token) *bad_token = t;
        const uint64_t a = v->post_off[t], b = v->post_off[t + 1];
        if (b < a || (b > a && (!v->post_doc || !v->post_tf))) return KDB_TEXT_BAD_VIEW;
        if (b - a > v->total_docs) return KDB_TEXT_BAD_DF;
        if (v->idf && !std::isfinite(v->idf[t])) return KDB_TEXT_BAD_IDF;
        uint32_t prev = 0;
        for (uint64_t i = a; i < b; i++) {
            const uint32_t d = v->post_doc[i];
            if (d == 0u || d > v->n_ids || d > cap) return KDB_TEXT_BAD_ID;
            if (i > a && d <= prev) return KDB_TEXT_BAD_ORDER;
            if (v->post_tf[i] == 0u) return KDB_TEXT_BAD_TF;
            prev = d;
        }
    }
    return KDB_TEXT_OK;
}
inline const char *kdb_text_strerror(int rc) {
    switch (rc) {
    case KDB_TEXT_OK: return "ok";
    case KDB_TEXT_BAD_VIEW: return "null array, n_ids above 2^30 - 1, or post_off does not start at 0 and ascend";
    case KDB_TEXT_BAD_ORDER: return "a posting list is not strictly ascending by id";
    case KDB_TEXT_BAD_ID: return "a posting names id 0, an id above n_ids or an id above the index's capacity";
    case KDB_TEXT_BAD_TF: return "a term frequency of 0";
    case KDB_TEXT_BAD_DF: return "a posting list longer than total_docs";
    case KDB_TEXT_BAD_AVG: return "avg_len is negative or not finite";
    case KDB_TEXT_BAD_IDF: return "an idf that is not finite";
    }
    return "?";
}
// the arguments of a text call that need no index: 0, or the reason as text
inline const char *kdb_text_call_check(uint32_t field, uint32_t t_stride, uint32_t k) {
    if (field >= KDB_MAX_TEXT_FIELDS) return "field outside 0..KDB_MAX_TEXT_FIELDS-1";
    if (t_stride > KDB_TEXT_MAX_TOKENS) return "t_stride above KDB_TEXT_MAX_TOKENS (32)";
    if (k == 0u || k > KDB_TEXT_MAX_K) return "k outside 1..1024";
    return nullptr;
}

#endif
