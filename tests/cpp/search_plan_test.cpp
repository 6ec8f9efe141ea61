// The launch plan of hnsw_search_kernel (kektordb_amd/csrc/kdb_search_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/search_plan_test.cpp
// The host sizes the launch with kdb_search_lds_bytes; the kernel cuts its dynamic LDS itself, region after region
// (search_kernel.cuh).  kernel_carve below restates that cut from the kernel's text, and the plan's byte count must be exactly where
// the cut ends: a plan that is a word short lets the hash table's last words run into the next workgroup's memory, one that is too
// large only costs occupancy, and neither shows in an answer.  Beside that: the class boundaries, the ladders of the beams the GPU
// parity module walks (tests/test_gpu_walk_instantiations.py), and what is left of a ladder at the 160 KiB limit.
//
//   search_plan_test ladder (<int8> <ld> <effective ef> <deleted nodes>)...: the ladder of each 4-tuple, one line per rung --
//   "<tuple> <hash> <waves> <visited words> <LDS bytes> <bounded> <planes>" -- for the GPU module to hold the launch-shape hook against
#include "kdb_search_plan.h"
#include "kdb_walk_lds.h" // kdb_nr_cap

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(cond)                                                                                                                          \
    do {                                                                                                                                     \
        if (!(cond)) {                                                                                                                       \
            printf("FAILED %s:%d: %s  (wk %d ld %u bs %d waves %u vis %u nr_cap %u ef %u)\n", __FILE__, __LINE__, #cond, (int)g_wk, g_ld, g_bs, \
                   g_waves, g_vis, g_nr, g_ef);                                                                                              \
            exit(1);                                                                                                                         \
        }                                                                                                                                    \
    } while (0)

static bool g_wk;
static int g_bs;
static uint32_t g_ld, g_waves, g_vis, g_nr, g_ef;

// hnsw_search_kernel's `off` when it has set s.marks, plus the region s.marks points at: PREC == KDB_PREC_I8 is wk, WIDE is waves,
// VIS == 1 is vis_size != 0 (the hash table; else the un-mark list of KDB_UP_MARK_CAP = 256 words).  hop3: the three-wave planes
// kernel, which cuts the hash table ahead of the pending list.
static size_t kernel_carve(bool wk, uint32_t ld, int BS, uint32_t WIDE, uint32_t beam_cap, uint32_t nr_cap, uint32_t vis_size, bool hop3) {
    size_t off = 0;
    off += wk ? ((size_t)ld + 15) / 16 * 16 : (size_t)ld * 4; // s.q (q_lds_bytes)
    if (BS == 0) off += (size_t)beam_cap * 4;                 // s.beam_d
    if (BS == 0) off += (size_t)beam_cap * 4;                 // s.beam_id
    if (BS == 0 && wk) off += (size_t)beam_cap * 4;           // s.beam_lo
    off += 64 * 4;                                            // s.nb_id
    off += 64 * 4;                                            // s.nb_d
    if (wk) off += 64 * 4;                                    // s.nb_lo
    if (WIDE > 1) off += 64;                                  // s.ctl
    if (WIDE > 1 || BS >= 2) {
        const uint32_t ins_n = 64u * (BS >= 2 ? (uint32_t)BS : 1u);
        off += ins_n * 4;                                     // s.ins_d
        off += ins_n * 4;                                     // s.ins_id
    }
    const size_t marks = (vis_size ? (size_t)vis_size : (size_t)256) * 4;
    if (hop3) off += marks;                                   // s.marks (the hash table: VIS == 1 there)
    off += (size_t)nr_cap * 4;                                // s.nr_d
    off += (size_t)nr_cap * 4;                                // s.nr_id
    if (wk) off += (size_t)nr_cap * 4;                        // s.nr_lo
    if (!hop3) off += marks;                                  // s.marks
    return off;
}

struct Want {
    uint32_t hash, waves, vis_words, lds;
    bool bounded, planes;
};
static void check_ladder(const KdbSearchLadder &l, std::initializer_list<Want> want) {
    CHECK(l.n == want.size() && l.n <= KDB_SEARCH_RUNGS_MAX);
    uint32_t i = 0;
    for (const Want &w : want) {
        const KdbSearchRung &r = l.rung[i++];
        g_waves = w.waves, g_vis = w.vis_words;
        CHECK(r.hash == w.hash && r.waves == w.waves && r.vis_words == w.vis_words && r.lds == w.lds && r.bounded == w.bounded && r.planes == w.planes);
    }
}

// the ladder rebuilt from the carve: every rung of the class in its order, a bounded one only where carve + 16 <= 160 KiB
static void check_ladder_against_carve(bool wk, uint32_t ld, uint32_t ef, uint32_t nr_cap) {
    g_wk = wk, g_ld = ld, g_ef = ef, g_nr = nr_cap;
    const KdbSearchLadder l = kdb_search_ladder(wk, ld, ef, nr_cap);
    const int bs = ef <= 64 ? 1 : ef <= 128 ? 2 : ef <= 256 ? 4 : 0;
    g_bs = bs;
    const uint32_t cap = (ef + 2 + 63) / 64 * 64;
    CHECK(l.bs == bs && l.beam_cap == cap);
    const uint32_t h1 = bs == 0 ? 0u : ef <= 100 ? 2048u : 4096u, hbig = ef <= 260 || ef > 1040 ? 0u : ef <= 520 ? 8192u : 16384u; // (257 .. 260: the LDS beam over the bitset)
    const uint32_t hw = bs == 4 ? h1 : h1 * 4;
    const size_t limit = 160u * 1024u;
    CHECK(l.lds1 == kernel_carve(wk, ld, bs, 1, cap, nr_cap, h1, false));
    if (l.lds1 + 16 > limit) {
        CHECK(l.n == 0);
        return;
    }
    uint32_t n = 0;
    auto expect = [&](uint32_t hash, uint32_t waves, uint32_t vis, bool last) {
        g_waves = waves, g_vis = vis;
        // (the latency modes of the two- and four-slot beams are launched with 512 bytes more than they cut: KDB_SEARCH_WIDE_SLACK)
        const size_t bytes = kernel_carve(wk, ld, bs, waves, cap, nr_cap, vis, false) + (bs >= 2 && waves > 1 ? 512u : 0u);
        if (!last && bytes + 16 > limit) return;
        CHECK(n < l.n);
        const KdbSearchRung &r = l.rung[n++];
        CHECK(r.hash == hash && r.waves == waves && r.vis_words == vis && r.lds == bytes && r.bounded == !last);
        CHECK(r.planes == (bs != 0 && waves == 1));
        CHECK(last || r.lds + 16 <= limit);
    };
    if (bs) {
        expect(1, 4, hw, false), expect(1, 2, hw, false), expect(1, 1, h1, true);
    } else {
        if (hbig) expect(1, 4, hbig, false), expect(1, 2, hbig, false), expect(1, 1, hbig, false);
        expect(0, 4, 0, false), expect(0, 2, 0, false), expect(0, 1, 0, true);
    }
    CHECK(n == l.n);
}

int main(int argc, char **argv) {
    if (argc > 1) {
        for (int i = 2, t = 0; i + 3 < argc; i += 4, t++) {
            const KdbSearchLadder l = kdb_search_ladder(atoi(argv[i]) != 0, (uint32_t)strtoul(argv[i + 1], nullptr, 10), (uint32_t)strtoul(argv[i + 2], nullptr, 10),
                                                        kdb_nr_cap((uint32_t)strtoul(argv[i + 3], nullptr, 10)));
            for (uint32_t r = 0; r < l.n; r++)
                printf("%d %u %u %u %u %d %d\n", t, l.rung[r].hash, l.rung[r].waves, l.rung[r].vis_words, l.rung[r].lds, (int)l.rung[r].bounded, (int)l.rung[r].planes);
        }
        return 0;
    }
    // class boundaries
    static_assert(kdb_beam_slots(1) == 1 && kdb_beam_slots(64) == 1 && kdb_beam_slots(65) == 2 && kdb_beam_slots(128) == 2 && kdb_beam_slots(129) == 4 &&
                      kdb_beam_slots(256) == 4 && kdb_beam_slots(257) == 0, "beam slots");
    static_assert(kdb_vis_hash_size(1) == 2048 && kdb_vis_hash_size(100) == 2048 && kdb_vis_hash_size(101) == 4096 && kdb_vis_hash_size(260) == 4096 &&
                      kdb_vis_hash_size(261) == 0, "visited hash");
    static_assert(kdb_vis_hash_size_large(260) == 0 && kdb_vis_hash_size_large(261) == 8192 && kdb_vis_hash_size_large(520) == 8192 &&
                      kdb_vis_hash_size_large(521) == 16384 && kdb_vis_hash_size_large(1040) == 16384 && kdb_vis_hash_size_large(1041) == 0, "large visited hash");
    static_assert(KDB_UP_MARK_CAP == 256u, "un-mark list");
    CHECK(kdb_walk_bs(64) == 2 && kdb_walk_bs(128) == 2 && kdb_walk_bs(129) == 4 && kdb_walk_bs(256) == 4 && kdb_walk_bs(257) == 0);

    // the footprint against the carve: the full cross
    for (bool wk : {false, true})
        for (uint32_t ld : {96u, 768u, 1536u})
            for (int bs : {0, 1, 2, 4})
                for (uint32_t waves : {1u, 2u, 4u})
                    for (uint32_t vis : {2048u, 4096u, 8192u, 16384u, 0u}) // hash, large hash, marks
                        for (uint32_t nr_cap : {4u, 2048u})
                            for (uint32_t beam_cap : {320u, 1216u}) {
                                g_wk = wk, g_ld = ld, g_bs = bs, g_waves = waves, g_vis = vis, g_nr = nr_cap, g_ef = beam_cap;
                                const size_t got = kdb_search_lds_bytes(wk, ld, bs, beam_cap, nr_cap, vis, waves);
                                CHECK(got == kernel_carve(wk, ld, bs, waves, beam_cap, nr_cap, vis, false));
                                if (bs == 1 && waves == 1 && vis) CHECK(got == kernel_carve(wk, ld, bs, waves, beam_cap, nr_cap, vis, true));
                                CHECK(got % 4 == 0);
                            }
    CHECK(kdb_search_lds_fits(160u * 1024u - 16u) && !kdb_search_lds_fits(160u * 1024u - 15u));

    // The ladders of the GPU parity module's beams: float32, 768 columns, 153 deleted nodes (156 pending entries).  (hash, waves,
    // visited words, LDS bytes, bounded, planes); the words of (one wave, latency mode) are that module's BEAMS table: (2048, 8192),
    // (2048, 8192), (4096, 4096), (8192, 8192), (16384, 16384), (0, 0).  The bytes are the launcher's as it was, summed by hand.
    g_wk = false, g_ld = 768, g_nr = 156;
    CHECK(kdb_nr_cap(153) == 156);
    g_ef = 16;
    check_ladder(kdb_search_ladder(false, 768, 16, 156), {{1, 4, 8192, 38176, true, false}, {1, 2, 8192, 38176, true, false}, {1, 1, 2048, 13024, false, true}});
    g_ef = 100;
    check_ladder(kdb_search_ladder(false, 768, 100, 156), {{1, 4, 8192, 39200, true, false}, {1, 2, 8192, 39200, true, false}, {1, 1, 2048, 14048, false, true}});
    g_ef = 200;
    check_ladder(kdb_search_ladder(false, 768, 200, 156), {{1, 4, 4096, 23840, true, false}, {1, 2, 4096, 23840, true, false}, {1, 1, 4096, 23264, false, true}});
    g_ef = 300;
    check_ladder(kdb_search_ladder(false, 768, 300, 156), {{1, 4, 8192, 40736, true, false}, {1, 2, 8192, 40736, true, false}, {1, 1, 8192, 40160, true, false},
                                                            {0, 4, 0, 8992, true, false}, {0, 2, 0, 8992, true, false}, {0, 1, 0, 8416, false, false}});
    g_ef = 700;
    check_ladder(kdb_search_ladder(false, 768, 700, 156), {{1, 4, 16384, 76576, true, false}, {1, 2, 16384, 76576, true, false}, {1, 1, 16384, 76000, true, false},
                                                            {0, 4, 0, 12064, true, false}, {0, 2, 0, 12064, true, false}, {0, 1, 0, 11488, false, false}});
    g_ef = 1200;
    check_ladder(kdb_search_ladder(false, 768, 1200, 156), {{0, 4, 0, 16160, true, false}, {0, 2, 0, 16160, true, false}, {0, 1, 0, 15584, false, false}});

    // every class, both key widths, short and long rows, few and many pending entries: the ladder is the carve's
    for (bool wk : {false, true})
        for (uint32_t ld : {96u, 768u, 1536u})
            for (uint32_t nr_cap : {4u, 156u, 2048u})
                for (uint32_t ef = 1; ef <= 1300; ef++) check_ladder_against_carve(wk, ld, ef, nr_cap);

    // limits.  1536 columns of float32, 4 pending entries: the one-wave bitset footprint is 7712 + 8 bytes per beam entry, so a beam
    // of 19456 entries (ef 19454) is the last that fits and ef 19455 (19520 entries) the first that is refused
    {
        uint32_t ef = 1;
        while (kdb_search_ladder(false, 1536, ef, 4).n) ef++;
        g_wk = false, g_ld = 1536, g_nr = 4, g_ef = ef;
        CHECK(ef == 19455);
        const KdbSearchLadder refused = kdb_search_ladder(false, 1536, ef, 4);
        CHECK(refused.n == 0 && refused.lds1 == 7712u + 19520u * 8u && refused.lds1 + 16 > 160u * 1024u);
        // just under: the latency modes (576 bytes more) no longer fit; the one-wave kernel is what is left
        check_ladder(kdb_search_ladder(false, 1536, 19454, 4), {{0, 1, 0, 7712u + 19456u * 8u, false, false}});
        // one step of the beam (64 entries, 512 bytes) further down all three rungs are back, in their order
        check_ladder(kdb_search_ladder(false, 1536, 19454 - 64, 4), {{0, 4, 0, 7712u + 19392u * 8u + 576u, true, false}, {0, 2, 0, 7712u + 19392u * 8u + 576u, true, false},
                                                                      {0, 1, 0, 7712u + 19392u * 8u, false, false}});
        // the large hash at the limit (ef 1040: 65536 bytes of hash, 1088 beam entries; rows of 22128 columns): one wave with the hash
        // fits (163296 + 16), its latency modes (163872) do not -- the bitset rungs follow as ever
        check_ladder(kdb_search_ladder(false, 22128, 1040, 4), {{1, 1, 16384, 163296, true, false}, {0, 4, 0, 99360, true, false}, {0, 2, 0, 99360, true, false},
                                                                 {0, 1, 0, 98784, false, false}});
        // ... and 160 columns more take the hash out altogether
        check_ladder(kdb_search_ladder(false, 22128 + 160, 1040, 4), {{0, 4, 0, 100000, true, false}, {0, 2, 0, 100000, true, false}, {0, 1, 0, 99424, false, false}});
        for (uint32_t ld = 16; ld <= 40960; ld += 16)
            for (uint32_t e : {64u, 128u, 256u, 520u, 1040u, 1200u}) {
                check_ladder_against_carve(false, ld, e, 4);
                check_ladder_against_carve(true, ld, e, 2048);
            }
    }
    printf("ok\n");
    return 0;
}
