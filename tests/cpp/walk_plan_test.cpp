// The LDS plan of a walking wave of graph construction (kektordb_amd/csrc/kdb_walk_lds.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/walk_plan_test.cpp
// The kernels take their pointers from this plan and the host sizes the launch from it; what is checked here is that the regions
// hold what a walk writes into them without touching each other, and that the numbers are the ones the four host sites computed
// by hand before the plan existed (the table: literals, the first row is the 4640 bytes the profiles show for
// build_search_kernel<1, 4, 0>).
#include "kdb_walk_lds.h"

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

struct Row {
    bool i8;
    uint32_t ld, efc, n_deleted, bs, beam_cap, nr_cap, bytes;
};

static void check_plan(bool i8, uint32_t ld, uint32_t efc, uint32_t n_deleted) {
    const KdbWalkLds w = kdb_walk_lds(i8, ld, efc, n_deleted);
    CHECK(w.bs == 0 || w.bs == 2 || w.bs == 4);
    CHECK(w.bs == 0 ? w.beam_cap >= efc + 2 : 64 * w.bs >= efc); // the beam holds ef entries (+ the LDS beam's two of slack)
    CHECK(w.nr_cap >= 1 && w.nr_cap % 4 == 0);
    // the regions in their order, with the bytes a walk needs in each
    const uint32_t beam = w.bs == 0 ? w.beam_cap * 4 : 0, nr = w.nr_cap * 4, lo = i8 ? 1 : 0;
    const uint32_t off[11] = {w.q, w.beam_d, w.beam_id, w.beam_lo, w.nr_d, w.nr_id, w.nr_lo, w.nb_id, w.nb_d, w.nb_lo, w.marks};
    const uint32_t need[11] = {i8 ? ld : ld * 4, beam, beam, beam * lo, nr, nr, nr * lo, 256, 256, 256 * lo, KDB_WALK_MARKS * 4};
    CHECK(off[0] == 0); // the query row: 16-byte aligned with the LDS itself
    uint32_t end = 0;
    for (int i = 0; i < 11; i++) {
        CHECK(off[i] >= end);    // in order, no overlap
        CHECK(off[i] % 4 == 0);
        end = off[i] + need[i];
    }
    CHECK(end == w.bytes);       // the end of marks is what the host asks for
}

int main(int argc, char **argv) {
    // walk_plan_test bs <efConstruction>...: the beam storage KDB_WALK_KERNEL dispatches on (wl.bs), one figure per argument -- the GPU
    // parity cases of the construction walks assert from it that each runs the <BS> instantiation it was written for
    if (argc > 1) {
        for (int i = 2; i < argc; i++) printf("%u\n", kdb_walk_lds(false, 48, (uint32_t)strtoul(argv[i], nullptr, 10), 0).bs);
        return 0;
    }
    const Row table[] = {
        {false, 768, 200, 0, 4, 320, 4, 4640},
        {false, 48, 400, 0, 0, 512, 4, 5856},
        {true, 768, 512, 5000, 0, 640, 2048, 34816},
        {false, 64, 64, 3, 2, 192, 4, 1824}, // (float16: the query in LDS is f32 as well)
        {false, 16, 256, 0, 4, 384, 4, 1632},
        {false, 16, 257, 0, 0, 384, 4, 4704},
    };
    for (const Row &r : table) {
        const KdbWalkLds w = kdb_walk_lds(r.i8, r.ld, r.efc, r.n_deleted);
        CHECK(w.bs == r.bs && w.beam_cap == r.beam_cap && w.nr_cap == r.nr_cap && w.bytes == r.bytes);
        check_plan(r.i8, r.ld, r.efc, r.n_deleted);
    }
    for (int i8 = 0; i8 < 2; i8++)
        for (uint32_t ld : {16u, 48u, 768u, 1536u, 4096u})
            for (uint32_t efc : {1u, 63u, 64u, 65u, 128u, 129u, 256u, 257u, 400u, 512u})
                for (uint32_t nd : {0u, 1u, 3u, 4u, 2046u, 2047u, 2048u, 1000000u, 0xffffffffu}) check_plan(i8 != 0, ld, efc, nd);
    // the side list: one entry more than the deleted nodes, in fours, 2048 at the most
    CHECK(kdb_nr_cap(0) == 4 && kdb_nr_cap(3) == 4 && kdb_nr_cap(4) == 8 && kdb_nr_cap(2046) == 2048 && kdb_nr_cap(2047) == 2048);
    CHECK(kdb_nr_cap(2048) == 2048 && kdb_nr_cap(0xffffffffu) == 2048);
    // the scoring tail: four waves' chunks of 64 distances and low words, then the row
    for (int i8 = 0; i8 < 2; i8++)
        for (uint32_t ld : {16u, 768u, 4096u}) {
            const KdbScoreTail t = kdb_score_tail(i8 != 0, ld);
            CHECK(t.w_d == 0 && t.w_lo == t.w_d + 4 * 64 * 4 && t.tq == t.w_lo + 4 * 64 * 4 && t.tq % 16 == 0);
            CHECK(t.bytes == 2048 + (i8 ? ld : ld * 4) + 64);
        }
    printf("ok\n");
    return 0;
}
