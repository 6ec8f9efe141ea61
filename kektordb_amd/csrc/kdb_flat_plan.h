// kdb_flat_plan.h -- everything the exact scan (flat_scan.hip) decides before its first launch, and what its kernels share with
// that decision: the tile constants, the stripe geometry, the seed predicate, the LDS sizes, the plan of one scan call and the
// layout of its scratch.
//
// ONE function resolves the stripe geometry and ONE states when a seed launch is valid: the host plans with them and the kernels
// run them, so the two cannot disagree.  The scratch layout is part of the plan: the launchers ask for plan.total bytes and form
// their pointers as base + offset.  Plain C++, no HIP header: host and device under hipcc, and tests/cpp/flat_plan_test.cpp builds
// it alone.
#ifndef KDB_FLAT_PLAN_H
#define KDB_FLAT_PLAN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/kektor_hip.h"
#include "kdb_stage.h"

#if defined(__HIPCC__)
#define KDB_FLAT_HD __host__ __device__
#else
#define KDB_FLAT_HD
#endif

constexpr int FS_TR = 128;          // rows per tile
constexpr int FS_TQ = 128;          // queries per tile
constexpr int FS_LDS_KL = 16;       // running top-k lists live in LDS up to this length, else in HBM scratch
constexpr uint32_t FS_MAX_MERGE = 16384; // entries one merge workgroup gathers in LDS (128 KB)
constexpr uint32_t FS_FIN = 1024;        // finalists one merge workgroup can re-score exactly (band modes)
constexpr int FS_PREC_F32R = 3; // internal: float32 rows RANKED on the f16 MFMA (converted while staging), re-scored exactly
constexpr int FSS_TQ = 16;     // small kernel: queries per workgroup
constexpr int FSS_SLACK = 64;  // small kernel: buffer = kl + one tile of rows + slack entries
constexpr uint32_t FSS_TAIL = FSS_TQ * 12; // small kernel: thresholds, counts
constexpr int FB_T = 256;        // big-tile kernel: rows per tile = queries per tile
constexpr int FB_SLAB = 128;     // big-tile kernel: bytes of every row per K slab
constexpr int FB_CSLOTS = 20;    // fs_compact_wave register slots: a list never holds more than 64 * 20 entries
constexpr uint32_t FSR_BUF = 320; // rescue kernel: entries per wave buffer (fs_compact_wave handles up to 320)
constexpr uint32_t FSR_TQ = 8;    // rescued queries that share one pass over a stripe's rows (ungrouped scans)
// Batches of at least this many queries rank with the big-tile kernel.
constexpr uint32_t FS_BIG_MIN = 33;
// Batches up to this many queries use flat_scan_small_kernel (the merge layout of the small kernel holds one 128-query tile, so
// never more than 128).
constexpr uint32_t FS_SMALL_MAX = 64;
// One launch = one round of 512 workgroups = (stripes) x (query tiles): with more than 64 query tiles the stripes
// get so long, and so many workgroups stream the same stripe out of step, that the rows fall out of L2 (32768
// queries in one launch: 3x slower per query, 150x the HBM traffic).  Larger batches run as 8192-query launches.
constexpr uint32_t FS_MAX_B = 8192;
// exact pass, first tier: up to FS_FEW unsettled queries go through the streaming kernel (16 queries per workgroup, the
// rows read at HBM speed by every CU) -- the tile kernel gives ONE query tile a handful of stripes: a single unsettled
// query of an 8192-query batch cost 78 ms behind a 12 ms ranking scan (seen once in five calls on the clustered corpus)
constexpr uint32_t FS_FEW = 64;
constexpr size_t FS_LDS_MAX = 150u * 1024u; // what a workgroup of the streaming / rescue kernels may ask for

// Stripe geometry, resolved ON THE DEVICE by every kernel of the scan and by the host's plan (same integer arithmetic everywhere):
// the number of rows that survive the filter is produced by a kernel of the same stream, so the host never waits for it.
// want: stripe count asked for; min_tiles: fewest tiles worth a stripe; tile_rows: FS_TR or FB_T.
struct FsGeom { uint32_t n_scan, n_stripes, rows_per_stripe; };
KDB_FLAT_HD static inline FsGeom fs_resolve_n(uint32_t n_scan, uint32_t want, uint32_t min_tiles, uint32_t tile_rows) {
    FsGeom g;
    g.n_scan = n_scan;
    const uint32_t TR = tile_rows;
    const uint32_t n_tiles = (g.n_scan + TR - 1) / TR;
    uint32_t ns = want;
    const uint32_t lim = (n_tiles + min_tiles - 1) / min_tiles;
    if (ns > lim) ns = lim;
    if (ns < 1) ns = 1;
    const uint32_t tiles_per = (n_tiles + ns - 1) / ns;
    g.n_stripes = tiles_per ? (n_tiles + tiles_per - 1) / tiles_per : 0u;
    g.rows_per_stripe = tiles_per * TR;
    return g;
}

// The seed launch of the big-tile kernel is valid when: it was decided (seeded) for the stripe count the geometry resolves to,
// there are at least two stripes, every stripe holds a whole first tile, and a stripe's share of the kl best is at most the 16 rows
// a tile's block maxima vouch for.  The host decides with it (and adds conditions of its own, fs_plan); both launches of the kernel
// check it again on the resolved geometry: false => the seed publishes nothing and the scan reads nothing -- open thresholds,
// slower, still exact.
KDB_FLAT_HD static inline bool fs_seed_ok(const FsGeom &geo, uint32_t kl, uint32_t seeded, uint32_t seed_nstr) {
    return seeded && seed_nstr == geo.n_stripes && geo.n_stripes >= 2u &&
           (geo.n_stripes - 1u) * geo.rows_per_stripe + FB_T <= geo.n_scan && (kl + geo.n_stripes - 1u) / geo.n_stripes <= 16u;
}

// big-tile kernel, entries allocated per (stripe, query): lists are compacted every `period` tiles when they hold more than
// kl + slack entries, and a tile appends at most FB_T entries to a list
KDB_FLAT_HD static inline uint32_t fb_cap(uint32_t kl, uint32_t slack, uint32_t period) { return kl + slack + period * (uint32_t)FB_T; }

// per-stripe list length: a stripe keeps its k+16 best by the ranking key; the merge kernel checks that no full
// list reaches into the error band of the k-th key (else the query goes to the exact / rescue pass)
KDB_FLAT_HD static inline uint32_t fs_kl(uint32_t k) { return k + 16 > 144 ? 144 : k + 16; }
KDB_FLAT_HD static inline uint32_t fs_cap_s(uint32_t kl) { return kl + FS_TR + FSS_SLACK; } // a query's buffer in the small kernel

// small kernel, 16 queries in LDS in the encoding prec (KDB_PREC_* or FS_PREC_F32R): stride of an f32 query, bytes of all 16
KDB_FLAT_HD static inline uint32_t fss_qstride(uint32_t ld) { return ld + ((40u + 64u - (ld & 63u)) & 63u); }
KDB_FLAT_HD static inline size_t fss_q_bytes(int prec, uint32_t ld) {
    return prec == KDB_PREC_I8   ? (((size_t)FSS_TQ * (ld + 16u) + 255u) & ~(size_t)255u)
           : (prec == FS_PREC_F32R || prec == KDB_PREC_F16) ? (((size_t)FSS_TQ * (ld * 2u + 16u) + 255u) & ~(size_t)255u)
                                  : (size_t)FSS_TQ * fss_qstride(ld) * 4u;
}
// LDS of the small kernel: the queries, their buffers, thresholds and counts
KDB_FLAT_HD static inline size_t fs_small_lds(int prec, uint32_t ld, uint32_t kl) {
    return fss_q_bytes(prec, ld) + (size_t)FSS_TQ * fs_cap_s(kl) * 8 + FSS_TAIL;
}
// LDS of the merge kernel: <= FS_MAX_MERGE gathered entries, the finalists, the query, the stripes' counts and thresholds
KDB_FLAT_HD static inline size_t fs_merge_lds(uint32_t ld, uint32_t want, uint32_t kl) {
    return (size_t)want * kl * 8 + FS_FIN * 8 + 48 + 1024 + (size_t)ld * 4 + (size_t)want * 12 + 16;
}
// LDS of the rescue kernel with tq queries per work item
KDB_FLAT_HD static inline size_t fsr_lds_bytes(uint32_t ld, uint32_t tq) {
    return (size_t)tq * ((size_t)ld * 4 + 4 * FSR_BUF * 8 + 4 * 4 + 4 * 8) + 64;
}

// float32 cosine / L2: rank on the f16 MFMA inside a rigorous error band, settle the rest exactly (only when the library
// normalised the queries itself and the rows are far from the f16 range limit)
static inline bool fs_rank16_ok(uint32_t precision, uint32_t metric, bool queries_normalised, float max_norm2, bool exact_only) {
    return precision == KDB_PREC_F32 && (metric == KDB_METRIC_L2 || queries_normalised) && max_norm2 > 0.f && max_norm2 <= 1.0e4f && !exact_only;
}
// eps bounds |q.x (wave order) - sum f16(q)f16(x) (MFMA order)| for rows and queries of norm <= 1: f16 rounding
// of both factors (2^-10 and its square), f32 summation in either order (dim * 2^-23); band = 2 * eps
// rows of norm R widen it by R (queries are normalised by the preparation step)
static inline float fs_band(uint32_t metric, float max_norm2, uint32_t dim) {
    const float rmax = metric == KDB_METRIC_COSINE ? (max_norm2 > 1.0f ? sqrtf(max_norm2) : 1.0f) : sqrtf(max_norm2);
    return 2.0f * (9.9e-4f + (float)dim * 2.4e-7f) * rmax * 1.001f; // cosine: the band; L2: per unit of ||q|| (x2 in the kernel)
}
// float32 indexes: the ranking copy has its own row stride (ld16: whole 128-byte slabs, zero pad).  The kernels that read it take
// a view with that stride and queries re-laid with it (fs_pad_queries); everything exact keeps the index's own.
static inline uint32_t fs_rank_ld(uint32_t precision, uint32_t ld, bool has_rows16, uint32_t ld16) {
    return precision == KDB_PREC_F32 && has_rows16 && ld16 != ld ? ld16 : ld;
}

// What fs_plan decides from.  The two environment switches are read where this is filled (flat_scan.hip), once per call.
struct FsPlanIn {
    uint32_t precision, metric; // KDB_PREC_*, KDB_METRIC_*
    uint32_t ld, ld16, dim, count;
    bool has_rows16;            // float32 index: the half-precision row copy exists (stride ld16)
    float max_norm2;
    uint32_t B, k;
    bool need_ids;              // a filter or deleted rows: the scan list is compacted on the device, its length stays there
    bool queries_normalised;
    bool exact_only;            // KDB_FLAT_EXACT_ONLY
    uint32_t seed_min_tiles;    // KDB_FB_SEED_MIN_TILES, default 32
};

// Geometry of one scan of <= FS_MAX_B queries with k <= 128: which kernels, how many stripes, how much scratch and where.
struct FsPlan {
    uint32_t kl, n_qtiles, n_q16;
    size_t lds_s;         // the small kernel's LDS with the queries in the index's own precision
    uint32_t ld_rank;     // row stride of the ranking copy (fs_rank_ld)
    bool copy_padded;     // ... which is another than the index's
    bool need_ids;        // scan list: the compacted ids of the rows that are live and allowed (else identity)
    bool rank16, small, big, few_tier;
    uint32_t want, min_tiles, cap;                   // small / 128 x 128 tile kernel
    uint32_t want_big, cap_big;                      // big-tile kernel ...
    uint32_t fb_nqt, fb_nqg, fb_nqx, fb_spx;         // ... its blockIdx -> (query tile, stripe) map (FsParams)
    uint32_t fb_slack, fb_period;
    uint32_t fb_seeded, fb_seed_nstr;                // a seed launch goes first; the stripe count that decision assumed
    uint32_t want_few;                               // first tier of the exact pass
    size_t n_part, n_part_big, n_part_few, n_qpad;   // (stripe, query) lists; query rows the ranking kernels may touch
    size_t ids_bytes, fbq_bytes, fbl_bytes, rsl_bytes, part_bytes, qp_bytes;
    // scratch layout, byte offsets in this order: [scan_ids: count u32][header: n_scan word, counts (256 B)][unsettled queries /
    // query halfs][their list][rescue list][per-stripe lists][padded queries]
    size_t o_ids, o_hdr, o_fbq, o_fblist, o_rslist, o_part, o_qpad, total;
};

// bytes of n_part per-stripe lists of cap entries: keys, ids, counts (+ words more per list: the big-tile kernel's thresholds)
static inline size_t fs_lists_bytes(size_t n_part, uint32_t cap, uint32_t words) { return n_part * cap * 8 + n_part * 4 * words; }

static inline FsPlan fs_plan(const FsPlanIn &in) {
    FsPlan g{};
    const uint32_t B = in.B;
    g.n_qtiles = (B + FS_TQ - 1) / FS_TQ;
    g.kl = fs_kl(in.k);
    // small batches take the HBM-bound streaming kernel (16 queries per workgroup, whole queries in LDS)
    g.n_q16 = (B + FSS_TQ - 1) / FSS_TQ;
    g.lds_s = fs_small_lds((int)in.precision, in.ld, g.kl);
    // which kernel (measured at 1M x 768, scripts/flat_probe.py): the streaming kernel re-reads the rows once per 16 queries
    // and wins up to 32 queries (0.47 ms at 32); the big-tile kernel (flat_scan_big.cuh: 256 queries x 256 rows per
    // workgroup; rows must be whole 128-byte slabs -- any number: 64-d halfs are ONE slab, 8192 queries 11.4 -> 2.9 ms against the
    // 128 x 128 tile kernel -- in a 1- or 2-byte encoding: int8 rows, float16 rows, or the
    // half-precision ranking copy of float32 rows) wins from 65 queries on (128 queries 0.92 vs 1.20 ms for the 128 x 128
    // tile kernel, 256 queries 1.10 vs 1.81 ms; k=100: 1.30 vs 3.66 ms) and between 33 and 64 queries when the lists are
    // short (k=10, 48 queries: 0.69 vs 1.04 ms; k=100, 64 queries: 1.12 vs 0.94 ms)
    g.ld_rank = fs_rank_ld(in.precision, in.ld, in.has_rows16, in.ld16);
    g.copy_padded = g.ld_rank != in.ld;
    const uint32_t rowb = in.precision == KDB_PREC_I8 ? in.ld : g.ld_rank * 2u;
    const bool rank16_ok = fs_rank16_ok(in.precision, in.metric, in.queries_normalised, in.max_norm2, in.exact_only);
    const bool big_ok = B >= FS_BIG_MIN && rowb % (uint32_t)FB_SLAB == 0u &&
                        (in.precision == KDB_PREC_I8 || in.precision == KDB_PREC_F16 || (rank16_ok && in.has_rows16));
    g.small = B <= FS_SMALL_MAX && g.lds_s <= FS_LDS_MAX && !(big_ok && B > 32u && g.kl <= 48u);
    // float32, large batches: rank on the f16 MFMA inside a rigorous error band, settle the rest exactly
    // (small batches rank on the half-precision copy of the rows, when the index keeps one: half the HBM bytes)
    g.rank16 = (!g.small || in.has_rows16) && rank16_ok;
    g.big = !g.small && big_ok;

    g.ids_bytes = ((size_t)in.count * 4 + 255) / 256 * 256;
    g.need_ids = in.need_ids;
    uint32_t stripes_max = FS_MAX_MERGE / g.kl;
    if (stripes_max < 1) stripes_max = 1;
    // stripes: ONE round of resident workgroups (two fit a CU: 512 in all).  Every stripe pays a start-up phase
    // (threshold still open, everything is a survivor), so more, shorter stripes only cost: measured at 1M x 768,
    // 512 workgroups beat 1024 and 2048 for every batch from 1 to 8192 queries.
    g.want = 512 / (g.small ? g.n_q16 : g.n_qtiles);
    if (g.want < 1) g.want = 1;
    if (g.want > stripes_max) g.want = stripes_max;
    g.min_tiles = g.small ? 4u : 8u;
    {   // never more stripes than the index could fill
        const uint32_t max_tiles = (in.count + FS_TR - 1) / FS_TR;
        const uint32_t lim = (max_tiles + g.min_tiles - 1) / g.min_tiles;
        if (g.want > lim) g.want = lim;
        if (g.want < 1) g.want = 1;
    }
    g.n_part = (size_t)g.want * g.n_qtiles * FS_TQ;
    // buffered mode: kl entries + room for max(kl, 64) appends between two compactions (<= 320 in all)
    g.cap = (g.small || g.kl <= (uint32_t)FS_LDS_KL) ? g.kl : g.kl + (g.kl > 64u ? g.kl : 64u);
    g.fb_nqg = g.fb_nqx = g.fb_spx = g.want_big = 1;
    if (g.big) {
        g.fb_nqt = (B + FB_T - 1) / FB_T;                 // <= 32 (batches above 8192 queries are split)
        const uint32_t per_xcd = 8u;
        while (g.fb_nqg * per_xcd < g.fb_nqt && g.fb_nqg < 8u) g.fb_nqg *= 2u; // groups of <= 8 query tiles; 1, 2 or 4 groups
        g.fb_nqx = (g.fb_nqt + g.fb_nqg - 1u) / g.fb_nqg; // query tiles an XCD serves
        g.fb_spx = 32u / g.fb_nqx;                        // stripes an XCD walks (32 CUs, one workgroup each)
        g.want_big = (8u / g.fb_nqg) * g.fb_spx;
        if (g.want_big > stripes_max) g.want_big = stripes_max;
        const uint32_t max_tiles = (in.count + FB_T - 1) / FB_T;
        const uint32_t lim = (max_tiles + 3u) / 4u;
        if (g.want_big > lim) g.want_big = lim;
        if (g.want_big < 1) g.want_big = 1;
    }
    g.fb_slack = 64u;
    g.fb_period = 4u; // measured at 8192 queries over 1M x 768: period 1 / 2 / 4 = 14.8 / 14.0 / 13.9 ms
    while (g.fb_period > 1u && fb_cap(g.kl, g.fb_slack, g.fb_period) > 64u * (uint32_t)FB_CSLOTS) g.fb_period--;
    if (fb_cap(g.kl, g.fb_slack, g.fb_period) > 64u * (uint32_t)FB_CSLOTS) g.fb_slack = 64u * (uint32_t)FB_CSLOTS - g.kl - g.fb_period * (uint32_t)FB_T;
    g.cap_big = fb_cap(g.kl, g.fb_slack, g.fb_period);
    g.n_part_big = g.big ? (size_t)g.want_big * g.fb_nqt * FB_T : 0;
    // Seed launch: only when the stripe geometry is known here (no filter, no deleted rows: the row count never leaves the
    // device otherwise), the kernel's own predicate holds on it, and a stripe is long enough to gain
    // (a stripe of fewer than 32 tiles pays more for the extra tile than the open thresholds cost it: 128 queries over
    //  1M x 768 = 256 stripes of 15 tiles 0.92 vs 0.89 ms; 8192 queries = 8 stripes of 488 tiles 11.80 vs 11.94 ms;
    //  tests lower seed_min_tiles: the seed path on small cases)
    if (g.big && !in.need_ids) {
        const FsGeom geo = fs_resolve_n(in.count, g.want_big, 4u, (uint32_t)FB_T);
        g.fb_seed_nstr = geo.n_stripes;
        if (fs_seed_ok(geo, g.kl, 1u, g.fb_seed_nstr) && geo.rows_per_stripe / (uint32_t)FB_T >= in.seed_min_tiles) g.fb_seeded = 1u;
    }

    g.part_bytes = fs_lists_bytes(g.n_part, g.cap, 1) + 1024;
    // big-tile kernel: lists + counts + the thresholds the stripes publish / end with (two floats per (stripe, query))
    if (g.big && fs_lists_bytes(g.n_part_big, g.cap_big, 3) + 1024 > g.part_bytes) g.part_bytes = fs_lists_bytes(g.n_part_big, g.cap_big, 3) + 1024;
    g.fbq_bytes = g.rank16 ? (((size_t)g.n_qtiles * FS_TQ * in.ld * 4 + 255) & ~(size_t)255) : 0; // vectors of the unsettled queries
    if (g.big && in.precision == KDB_PREC_F16) g.fbq_bytes = ((size_t)g.fb_nqt * FB_T * in.ld * 2 + 255) & ~(size_t)255; // the queries as halfs
    g.n_qpad = (size_t)(g.big ? g.fb_nqt * FB_T : g.n_qtiles * FS_TQ); // query rows the ranking kernels may touch (d_q holds >= as many)
    if (g.rank16 && g.copy_padded) { // ... the ranking scan's query halfs live there first, with the copy's stride
        const size_t h = ((g.n_qpad * g.ld_rank * 2 + 255) & ~(size_t)255);
        if (h > g.fbq_bytes) g.fbq_bytes = h;
    }
    g.qp_bytes = (g.rank16 && g.copy_padded) ? ((g.n_qpad * g.ld_rank * 4 + 255) & ~(size_t)255) : 0;
    g.few_tier = g.rank16 && !g.small && g.lds_s <= FS_LDS_MAX;
    g.want_few = 512u / (FS_FEW / (uint32_t)FSS_TQ);
    if (g.want_few > stripes_max) g.want_few = stripes_max;
    {
        const uint32_t max_tiles = (in.count + FS_TR - 1) / FS_TR;
        const uint32_t lim = (max_tiles + 3u) / 4u;
        if (g.want_few > lim) g.want_few = lim;
        if (g.want_few < 1u) g.want_few = 1u;
    }
    g.n_part_few = (size_t)g.want_few * FS_TQ; // one 128-query block of lists per stripe
    if (g.few_tier && fs_lists_bytes(g.n_part_few, g.kl, 1) + 1024 > g.part_bytes) g.part_bytes = fs_lists_bytes(g.n_part_few, g.kl, 1) + 1024;
    g.fbl_bytes = g.rank16 ? (((size_t)g.n_qtiles * FS_TQ * 4 + 255) & ~(size_t)255) : 0; // their indices
    g.rsl_bytes = ((size_t)g.n_qtiles * FS_TQ * 4 + 255) & ~(size_t)255;                  // queries handed to the rescue pass

    KdbCarver scratch;
    g.o_ids = scratch.take(g.ids_bytes);
    g.o_hdr = scratch.take(256);
    g.o_fbq = scratch.take(g.fbq_bytes);
    g.o_fblist = scratch.take(g.fbl_bytes);
    g.o_rslist = scratch.take(g.rsl_bytes);
    g.o_part = scratch.take(g.part_bytes);
    g.o_qpad = scratch.take(g.qp_bytes);
    g.total = scratch.total();
    return g;
}

// ---- grouped scan (one allow list per group of queries): always the small kernel, over the T 16-query tiles of the groups

constexpr uint32_t FG_NB = 64; // chunks a group's bitset is counted and filled in

// Stripes per group.  Workgroup b runs on XCD b % 8 (the dispatcher deals workgroups round-robin) and serves stripe
// (b/8/T)*8 + b%8, so that the tiles of one stripe share an L2: XCD x owns the stripes s = x (mod 8) and therefore
// T * ceil-ish(want/8) workgroups for its n_cu/8 CUs.  Round 2 sized `want` as if the chip were one pool of slots: with
// 105 tiles it picked 9 stripes, which gave XCD 0 twice the work of the others (config 5 ran at 2.85 TB/s).  Now the
// estimated time -- rounds of the BUSIEST XCD x (rows of a stripe + a start-up allowance for the open threshold of a
// stripe's first tiles) -- is minimised over the stripe counts the merge can take.
static inline uint32_t fs_group_stripes(uint32_t n_cu, uint32_t T, uint32_t G, uint64_t total, uint32_t stripes_max, size_t lds_s) {
    const uint32_t per_cu = (uint32_t)(160u * 1024u / lds_s) > 0 ? (uint32_t)(160u * 1024u / lds_s) : 1u;
    const uint32_t slots_x = (n_cu / 8u > 0 ? n_cu / 8u : 1u) * (per_cu > 2 ? 2u : per_cu);
    uint32_t want = 1;
    const double rows_g = (double)total / (double)G; // rows per group (the caller's bound, or counted)
    const double startup = 3.0 * FS_TR;
    double best = 1e300;
    const uint32_t lim = stripes_max < 64u ? stripes_max : 64u;
    for (uint32_t w = 1; w <= lim; w++) {
        if ((double)w * 4.0 * FS_TR > rows_g && w > 1) break; // a stripe is at least min_tiles tiles
        const uint64_t on_x = (uint64_t)T * ((w + 7u) / 8u);  // workgroups of the busiest XCD
        const uint64_t rounds = (on_x + slots_x - 1) / slots_x;
        const double t = (double)rounds * (rows_g / (double)w + startup);
        if (t < best * 0.98) { best = t; want = w; } // the fewest stripes within 2 % of the best
    }
    return want;
}

// scratch of the group-size count that runs first when the caller gave no bound on the allowed rows: [G][FG_NB] counts
static inline size_t fs_group_count_bytes(uint32_t G) {
    KdbCarver scratch;
    scratch.take((size_t)G * FG_NB * 4);
    return scratch.total();
}

// in: as for fs_plan (need_ids and seed_min_tiles unused); T 16-query tiles in G groups, total = allowed rows of all groups
struct FsGroupPlan {
    uint32_t kl, n_qtiles, want, ld_rank;
    size_t lds_s;    // the small kernel's LDS with the queries in the index's own precision
    bool rank16;     // float32 indexes with a half-precision row copy rank on it inside the error band (see fs_plan)
    size_t n_part;
    // scratch layout, byte offsets in this order.  q_flag, tile_flag and the header are cleared in one go (o_rsl - o_qflag bytes).
    size_t o_ids, o_gn, o_gbase, o_ccnt, o_cbase, o_tiles, o_qgrp, o_qtile, o_qflag, o_tflag, o_hdr, o_rsl, o_part, o_qpad, total;
};
static inline FsGroupPlan fs_group_plan(const FsPlanIn &in, uint32_t n_cu, uint32_t T, uint32_t G, uint64_t total) {
    FsGroupPlan g{};
    g.kl = fs_kl(in.k); // finalists are re-scored in the order of the graph search
    g.lds_s = fs_small_lds((int)in.precision, in.ld, g.kl);
    g.ld_rank = fs_rank_ld(in.precision, in.ld, in.has_rows16, in.ld16);
    g.rank16 = in.has_rows16 && fs_rank16_ok(in.precision, in.metric, in.queries_normalised, in.max_norm2, in.exact_only);
    g.want = fs_group_stripes(n_cu, T, G, total, FS_MAX_MERGE / g.kl, g.lds_s);
    g.n_qtiles = (in.B + FS_TQ - 1) / FS_TQ;
    g.n_part = (size_t)g.want * g.n_qtiles * FS_TQ;
    const size_t chunk_bytes = (size_t)G * FG_NB * 4, tile_bytes = (size_t)T * 3 * 4, q_bytes = (size_t)in.B * 4;
    KdbCarver scratch;
    g.o_ids = scratch.take((size_t)total * 4 + 1024);
    g.o_gn = scratch.take((size_t)G * 4);
    g.o_gbase = scratch.take((size_t)G * 4);
    g.o_ccnt = scratch.take(chunk_bytes);  // [G][FG_NB] rows per chunk
    g.o_cbase = scratch.take(chunk_bytes); // where each chunk writes
    g.o_tiles = scratch.take(tile_bytes);
    g.o_qgrp = scratch.take(q_bytes);
    g.o_qtile = scratch.take(q_bytes);
    g.o_qflag = scratch.take(q_bytes);
    g.o_tflag = scratch.take(tile_bytes);
    g.o_hdr = scratch.take(256);           // counts: unsettled queries, queries handed to the rescue pass
    g.o_rsl = scratch.take(q_bytes);
    g.o_part = scratch.take(fs_lists_bytes(g.n_part, g.kl, 1) + 1024);
    g.o_qpad = scratch.take(g.ld_rank != in.ld ? (size_t)in.B * g.ld_rank * 4 : 0);
    g.total = scratch.total();
    return g;
}
#endif
