// The plan of the exact scan (kektordb_amd/csrc/kdb_flat_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/flat_plan_test.cpp
// The kernels resolve their stripes with fs_resolve_n and check the seed launch with fs_seed_ok; the host plans with the same two
// functions and takes every scratch pointer from the plan's offsets.  What is checked here: the geometry covers the rows with
// whole tiles inside 32 bits, the plan's choices respect what the kernels can take, the scratch regions are in order, aligned,
// disjoint and as large as each layout that shares them, and the figures are the ones fs_plan produced while it still lived in
// flat_scan.hip (the table: literals, printed once by that version for the shapes the benchmark and the GPU tests run).
#include "kdb_flat_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static void check_geometry(uint32_t n_scan, uint32_t want, uint32_t min_tiles, uint32_t tile_rows) {
    const FsGeom g = fs_resolve_n(n_scan, want, min_tiles, tile_rows);
    CHECK(g.n_scan == n_scan);
    CHECK(g.n_stripes <= want);
    CHECK((g.n_stripes == 0) == (n_scan == 0));
    CHECK(g.rows_per_stripe % tile_rows == 0);
    if (n_scan == 0) return;
    // the stripes cover the rows and the last one is not empty
    CHECK((uint64_t)g.n_stripes * g.rows_per_stripe >= n_scan);
    CHECK((uint64_t)(g.n_stripes - 1) * g.rows_per_stripe < n_scan);
    // the kernels form stripe * rows_per_stripe in 32 bits: the first row of every stripe fits
    for (uint32_t s = 0; s < g.n_stripes; s++) CHECK((uint64_t)s * g.rows_per_stripe <= 0xffffffffull);
}

// bytes of the three list layouts that share `part`, and of the three uses of `fbq`
static size_t lists_tile(const FsPlan &g) { return g.n_part * g.cap * 8 + g.n_part * 4; }
static size_t lists_big(const FsPlan &g) { return g.n_part_big * g.cap_big * 8 + g.n_part_big * 4 + 2 * g.n_part_big * 4; } // + g_pub, part_thr
static size_t lists_few(const FsPlan &g) { return g.n_part_few * g.kl * 8 + g.n_part_few * 4; }

static void check_plan(const FsPlanIn &in) {
    const FsPlan g = fs_plan(in);
    CHECK(g.kl == fs_kl(in.k) && g.kl >= in.k && g.kl <= 144);
    // exactly one ranking kernel: the small one, the big-tile one, or (neither flag) the 128 x 128 tile kernel
    const bool tile = !g.small && !g.big;
    CHECK((int)g.small + (int)g.big + (int)tile == 1);
    if (g.small) CHECK(g.lds_s <= FS_LDS_MAX && in.B <= FS_SMALL_MAX);
    if (g.big) {
        const uint32_t rowb = in.precision == KDB_PREC_I8 ? in.ld : g.ld_rank * 2u;
        CHECK(in.B >= FS_BIG_MIN && rowb % (uint32_t)FB_SLAB == 0);
        CHECK(in.precision == KDB_PREC_I8 || in.precision == KDB_PREC_F16 || (g.rank16 && in.has_rows16)); // a 1- or 2-byte ranking encoding
        CHECK(g.fb_nqt * (uint32_t)FB_T >= in.B && g.fb_nqg * g.fb_nqx >= g.fb_nqt && g.fb_nqg <= 8 && g.fb_spx >= 1);
        CHECK((8u / g.fb_nqg) * g.fb_spx * g.fb_nqx <= 256); // the launch is 256 workgroups: 32 per XCD
    }
    if (g.rank16) CHECK(in.precision == KDB_PREC_F32 && !in.exact_only);
    if (g.few_tier) CHECK(g.rank16 && !g.small && g.lds_s <= FS_LDS_MAX);
    CHECK(g.want >= 1 && g.want_big >= 1 && g.want_few >= 1);
    CHECK(g.want * g.kl <= FS_MAX_MERGE && g.want_big * g.kl <= FS_MAX_MERGE && g.want_few * g.kl <= FS_MAX_MERGE);
    CHECK(g.cap_big <= 64u * (uint32_t)FB_CSLOTS && g.fb_period >= 1 && g.cap_big == fb_cap(g.kl, g.fb_slack, g.fb_period));
    CHECK(g.cap >= g.kl);
    // the seed launch: decided by the predicate the kernel checks, on the geometry the kernel resolves -- the same two functions,
    // so the two cannot disagree; stated here all the same
    if (g.fb_seeded) {
        CHECK(g.big && !in.need_ids);
        const FsGeom geo = fs_resolve_n(in.count, g.want_big, 4u, (uint32_t)FB_T);
        CHECK(fs_seed_ok(geo, g.kl, g.fb_seeded, g.fb_seed_nstr));
        CHECK(geo.rows_per_stripe / (uint32_t)FB_T >= in.seed_min_tiles);
    }
    // scratch: in order, 256-byte aligned, disjoint, ending at total
    const size_t off[7] = {g.o_ids, g.o_hdr, g.o_fbq, g.o_fblist, g.o_rslist, g.o_part, g.o_qpad};
    const size_t need[7] = {g.ids_bytes, 256, g.fbq_bytes, g.fbl_bytes, g.rsl_bytes, g.part_bytes, g.qp_bytes};
    CHECK(off[0] == 0);
    size_t end = 0;
    for (int i = 0; i < 7; i++) {
        CHECK(off[i] >= end && off[i] % 256 == 0);
        end = off[i] + need[i];
    }
    CHECK(g.total >= end && g.total - end < 256 && g.total % 256 == 0);
    CHECK(g.ids_bytes >= (size_t)in.count * 4);
    // `part` holds each of the list layouts that alias it
    CHECK(g.part_bytes >= lists_tile(g));
    if (g.big) CHECK(g.part_bytes >= lists_big(g));
    if (g.few_tier) CHECK(g.part_bytes >= lists_few(g));
    // `fbq` holds each of its uses: the vectors of the unsettled queries, the queries as halfs, and those with the copy's stride
    if (g.rank16) CHECK(g.fbq_bytes >= (size_t)g.n_qtiles * FS_TQ * in.ld * 4);
    if ((g.rank16 && !g.small) || (g.big && in.precision == KDB_PREC_F16)) {
        const bool rk = g.rank16 && g.copy_padded;
        CHECK(g.fbq_bytes >= g.n_qpad * (rk ? g.ld_rank : in.ld) * 2);
    }
    if (g.qp_bytes) CHECK(g.rank16 && g.copy_padded && g.qp_bytes >= g.n_qpad * g.ld_rank * 4);
    CHECK(g.fbl_bytes >= (g.rank16 ? (size_t)in.B * 4 : 0) && g.rsl_bytes >= (size_t)in.B * 4);
}

struct PlanRow {
    FsPlanIn in; // exact_only false, seed_min_tiles as given
    int small, big, rank16, few_tier;
    uint32_t want, want_big, cap, cap_big, fb_nqg, fb_nqx, fb_spx, fb_period, fb_seeded;
    size_t ids_bytes, fbq_bytes, fbl_bytes, rsl_bytes, part_bytes, qp_bytes;
};
static FsPlanIn plan_in(uint32_t prec, uint32_t metric, uint32_t ld, uint32_t ld16, uint32_t count, bool has16, float max_norm2, uint32_t B, uint32_t k,
                        bool need_ids, uint32_t seed_min_tiles) {
    FsPlanIn in{};
    in.precision = prec, in.metric = metric, in.ld = ld, in.ld16 = ld16, in.dim = ld, in.count = count;
    in.has_rows16 = has16, in.max_norm2 = max_norm2, in.B = B, in.k = k, in.need_ids = need_ids;
    in.queries_normalised = true, in.exact_only = false, in.seed_min_tiles = seed_min_tiles;
    return in;
}

struct StripesRow {
    uint32_t n_cu, T, G;
    uint64_t total;
    uint32_t stripes_max;
    size_t lds_s;
    uint32_t want;
};

int main() {
    for (uint32_t n_scan : {0u, 1u, 127u, 128u, 129u, 255u, 256u, 257u, 1000u, 65535u, 1000000u, 10000000u, 0xffffff00u})
        for (uint32_t want : {1u, 2u, 7u, 8u, 9u, 113u, 512u})
            for (uint32_t min_tiles : {1u, 4u, 8u})
                for (uint32_t tile_rows : {128u, 256u}) check_geometry(n_scan, want, min_tiles, tile_rows);

    const uint32_t F32 = KDB_PREC_F32, F16 = KDB_PREC_F16, I8 = KDB_PREC_I8, L2 = KDB_METRIC_L2, COS = KDB_METRIC_COSINE;
    // fs_plan as flat_scan.hip had it before this header existed (precision, metric, ld, ld16, count, row copy, max_norm2, B, k, filter,
    // seed_min_tiles): 1M x 768 cosine float32 with the row copy at 16 / 48 / 128 / 8192 queries, 10M x 768 L2 k = 100, int8, float16,
    // filtered, no row copy, a padded row copy over a short index, and two seed launches on small cases (seed_min_tiles 1)
    const PlanRow table[] = {
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 16, 10, false, 32),
         1, 0, 1, 0, 512, 1, 26, 1114, 1, 1, 1, 4, 0, 4000000, 393216, 512, 512, 13894656, 0},
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 48, 10, false, 32),
         0, 1, 1, 1, 512, 256, 90, 1114, 1, 1, 32, 4, 0, 4000000, 393216, 512, 512, 584844288, 0},
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 128, 10, false, 32),
         0, 1, 1, 1, 512, 256, 90, 1114, 1, 1, 32, 4, 0, 4000000, 393216, 512, 512, 584844288, 0},
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 8192, 10, false, 32),
         0, 1, 1, 1, 8, 8, 90, 1114, 4, 8, 4, 4, 1, 4000000, 25165824, 32768, 32768, 584844288, 0},
        {plan_in(F32, L2, 768, 768, 10000000, true, 900.0f, 1024, 100, false, 32),
         0, 1, 1, 1, 64, 64, 232, 1204, 1, 4, 8, 4, 1, 40000000, 3145728, 4096, 4096, 632030208, 0},
        {plan_in(I8, COS, 768, 0, 1000000, false, 1.0f, 256, 10, false, 32),
         0, 1, 0, 0, 256, 256, 90, 1114, 1, 1, 32, 4, 0, 4000000, 0, 0, 1024, 584844288, 0},
        {plan_in(F16, L2, 768, 0, 1000000, false, 1.0f, 256, 10, false, 32),
         0, 1, 0, 0, 256, 256, 90, 1114, 1, 1, 32, 4, 0, 4000000, 393216, 0, 1024, 584844288, 0},
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 128, 10, true, 32),
         0, 1, 1, 1, 512, 256, 90, 1114, 1, 1, 32, 4, 0, 4000000, 393216, 512, 512, 584844288, 0},
        {plan_in(F32, COS, 768, 0, 1000000, false, 1.0f, 128, 10, false, 32),
         0, 0, 1, 1, 512, 1, 90, 1114, 1, 1, 1, 4, 0, 4000000, 393216, 512, 512, 47449088, 0},
        {plan_in(F32, COS, 112, 128, 5000, true, 1.0f, 300, 32, false, 32),
         0, 1, 1, 1, 5, 5, 112, 1136, 1, 2, 16, 4, 0, 20224, 172032, 1536, 1536, 23297024, 262144},
        {plan_in(F32, COS, 768, 768, 1000000, true, 1.0f, 128, 10, false, 1),
         0, 1, 1, 1, 512, 256, 90, 1114, 1, 1, 32, 4, 1, 4000000, 393216, 512, 512, 584844288, 0},
        {plan_in(F32, COS, 112, 128, 5000, true, 1.0f, 300, 32, false, 1),
         0, 1, 1, 1, 5, 5, 112, 1136, 1, 2, 16, 4, 1, 20224, 172032, 1536, 1536, 23297024, 262144},
    };
    for (const PlanRow &r : table) {
        const FsPlan g = fs_plan(r.in);
        CHECK(g.small == (r.small != 0) && g.big == (r.big != 0) && g.rank16 == (r.rank16 != 0) && g.few_tier == (r.few_tier != 0));
        CHECK(g.want == r.want && g.want_big == r.want_big && g.cap == r.cap && g.cap_big == r.cap_big);
        CHECK(g.fb_nqg == r.fb_nqg && g.fb_nqx == r.fb_nqx && g.fb_spx == r.fb_spx && g.fb_period == r.fb_period && g.fb_seeded == r.fb_seeded);
        CHECK(g.ids_bytes == r.ids_bytes && g.fbq_bytes == r.fbq_bytes && g.fbl_bytes == r.fbl_bytes && g.rsl_bytes == r.rsl_bytes);
        CHECK(g.part_bytes == r.part_bytes && g.qp_bytes == r.qp_bytes);
        check_plan(r.in);
    }

    for (uint32_t prec : {F32, F16, I8})
        for (uint32_t metric : {L2, COS}) {
            if ((prec == F16 && metric != L2) || (prec == I8 && metric != COS)) continue; // float16 is L2 only, int8 cosine only
            for (uint32_t ld : {16u, 48u, 64u, 100u, 128u, 768u, 1536u, 4096u})
                for (uint32_t count : {1u, 300u, 5000u, 1000000u, 10000000u})
                    for (uint32_t B : {1u, 16u, 32u, 33u, 48u, 64u, 65u, 128u, 256u, 1024u, 8192u})
                        for (uint32_t k : {1u, 10u, 32u, 33u, 100u, 128u})
                            for (int has16 = 0; has16 < (prec == F32 ? 2 : 1); has16++)
                                for (int need_ids = 0; need_ids < 2; need_ids++)
                                    for (uint32_t smt : {1u, 32u})
                                        check_plan(plan_in(prec, metric, ld, has16 ? (ld + 63u) / 64u * 64u : 0u, count, has16 != 0, 1.0f, B, k,
                                                           need_ids != 0, smt));
        }

    // the grouped scan's stripes (n_cu, T tiles, G groups, allowed rows in all, stripes the merge can take, the small kernel's LDS):
    // 105 tiles of 100 groups take 24 stripes -- three per XCD -- where a count of free slots over the whole chip picked 9
    const StripesRow stripes[] = {
        {256, 105, 100, 10000000ull, 630, 78016, 24},
        {256, 105, 100, 10000000ull, 630, 40000, 24},
        {256, 1, 1, 1000ull, 630, 78016, 1},
        {256, 16, 4, 4000000ull, 141, 78016, 32},
        {256, 8, 8, 40000ull, 630, 20000, 9},
    };
    for (const StripesRow &r : stripes) CHECK(fs_group_stripes(r.n_cu, r.T, r.G, r.total, r.stripes_max, r.lds_s) == r.want);
    // ... and its scratch: in order, aligned, the flags and the header contiguous (they are cleared in one go)
    for (uint32_t B : {1u, 100u, 1000u})
        for (uint32_t G : {1u, 7u, 100u}) {
            const uint32_t T = (B + 15) / 16 + G;
            const FsPlanIn in = plan_in(F32, COS, 112, 128, 100000, true, 1.0f, B, 10, true, 32);
            const FsGroupPlan g = fs_group_plan(in, 256, T, G, (uint64_t)G * 1000);
            CHECK(g.kl == fs_kl(in.k) && g.lds_s == fs_small_lds((int)in.precision, in.ld, g.kl) && g.rank16 && g.ld_rank == 128);
            CHECK(g.want >= 1 && g.want * g.kl <= FS_MAX_MERGE && g.n_part == (size_t)g.want * g.n_qtiles * FS_TQ);
            const size_t off[14] = {g.o_ids, g.o_gn, g.o_gbase, g.o_ccnt, g.o_cbase, g.o_tiles, g.o_qgrp, g.o_qtile, g.o_qflag, g.o_tflag, g.o_hdr, g.o_rsl, g.o_part, g.o_qpad};
            const size_t need[14] = {(size_t)G * 1000 * 4, (size_t)G * 4, (size_t)G * 4, (size_t)G * FG_NB * 4, (size_t)G * FG_NB * 4, (size_t)T * 12, (size_t)B * 4, (size_t)B * 4,
                                     (size_t)B * 4, (size_t)T * 12, 256, (size_t)B * 4, g.n_part * g.kl * 8 + g.n_part * 4, (size_t)B * g.ld_rank * 4};
            size_t end = 0;
            for (int i = 0; i < 14; i++) {
                CHECK(off[i] >= end && off[i] % 256 == 0);
                end = off[i] + need[i];
            }
            CHECK(g.total >= end && g.total % 256 == 0);
            CHECK(g.o_tflag - g.o_qflag < 256 + (size_t)B * 4 && g.o_hdr - g.o_tflag < 256 + (size_t)T * 12 && g.o_rsl - g.o_hdr == 256);
            CHECK(fs_group_count_bytes(G) >= (size_t)G * FG_NB * 4);
        }
    printf("ok\n");
    return 0;
}
