// The plan of the heap-order walk (kektordb_amd/csrc/kdb_heap_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/heap_plan_test.cpp
// The host sizes heap_walk_kernel's launch with kdb_heap_plan_lds; the kernel cuts its dynamic LDS itself, region after region
// (search_heap.hip).  kernel_carve below restates that cut from the kernel's text -- the query, the neighbour arrays of one hop, the
// visited hash or the un-mark list, the result heap unless it is in registers, the drain arrays, the candidate heap's LDS part --
// and the plan's byte count must be exactly where the cut ends: a plan that is a word short lets the candidate heap's last LDS
// entries run into the next workgroup's memory, one that is too large only costs occupancy, and neither shows in an answer.
// Beside that: the bounds every plan keeps, for every ef from 1 to 2000.
#include "kdb_heap_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            printf("FAILED %s:%d: %s  (wk %d ld %u count %u ef %u)\n", __FILE__, __LINE__, #cond, (int)g_wk, g_ld, g_count, g_ef); \
            exit(1);                                                                                        \
        }                                                                                                   \
    } while (0)

static bool g_wk;
static uint32_t g_ld, g_count, g_ef;

// heap_walk_kernel's `off` after its last take(): VIS = the plan's hsize != 0, RES = the plan's reg_results, WK = int8
static size_t kernel_carve(bool wk, uint32_t ld, uint32_t ef, uint32_t hsize, bool reg_results, uint32_t nl_c) {
    size_t off = 0;
    off += wk ? ((size_t)ld + 15) / 16 * 16 : (size_t)ld * 4; // s.q: the packed int8 row, else float32 values
    off += 64 * 4;                                            // s.nb_id
    off += 64 * 4;                                            // s.nb_d
    if (wk) off += 64 * 4;                                    // s.nb_lo
    off += (hsize ? (size_t)hsize : (size_t)256) * 4;         // s.marks: the hash table, or the un-mark list (KDB_UP_MARK_CAP)
    const size_t nres = (size_t)ef + 2;
    const size_t arrays = wk ? 3 : 2;                         // id, key (, lo)
    if (!reg_results) off += arrays * nres * 4;               // results.st.l_id, l_key (, l_lo)
    off += arrays * nres * 4;                                 // res_id, res_key (, res_lo): the drain
    off += arrays * (size_t)nl_c * 4;                         // cands.st.l_id, l_key (, l_lo)
    return off;
}

int main() {
    static_assert(kdb_heap_hash_words(100) == 2048 && kdb_heap_hash_words(101) == 4096 && kdb_heap_hash_words(260) == 4096 &&
                      kdb_heap_hash_words(261) == 0, "the visited hash's boundaries");
    unsigned long refused = 0, planned = 0;
    for (bool wk : {false, true})
        for (uint32_t ld : {32u, 128u, 768u, 1536u})
            for (uint32_t count : {100u, 3000u, 1000000u})
                for (uint32_t ef = 1; ef <= 2000; ef++) {
                    g_wk = wk, g_ld = ld, g_count = count, g_ef = ef;
                    KdbHeapPlan p{};
                    const bool ok = kdb_heap_plan_lds(wk, ld, count, ef, &p);
                    // the footprint is the kernel's own, whether or not it fits
                    CHECK(p.lds == kernel_carve(wk, ld, ef, p.hsize, p.reg_results != 0, p.nl_c));
                    CHECK(ok == (p.lds + 16 <= 160u * 1024u)); // ... and it fits a CU's LDS, or the plan refuses
                    if (!ok) {
                        refused++;
                        continue;
                    }
                    planned++;
                    CHECK(p.hsize == (ef <= 100 ? 2048u : ef <= 260 ? 4096u : 0u));
                    CHECK((p.reg_results != 0) == (ef <= 62));                      // entry i in lane i: ef + 2 <= 64 (and a hash there)
                    CHECK(p.cap_c <= count + 2u);                                   // a heap never holds more entries than there are nodes
                    CHECK(p.cap_c == count + 2u || (p.cap_c >= 2048u && p.cap_c >= 16u * ef));
                    CHECK(p.nl_c <= p.cap_c);
                    CHECK(p.nl_c <= 4095u);                                         // twelve levels of the heap on chip
                    CHECK(p.nl_c >= 64u || p.nl_c == p.cap_c);                      // (a small index clips it to the capacity)
                    CHECK(p.grid == 0 && p.tail_bytes == 0);                        // the launch's, not this header's
                    CHECK(kdb_heap_tail_bytes(7, p.cap_c, p.nl_c) == (size_t)7 * (p.cap_c - p.nl_c) * 12u);
                }
    CHECK(planned > 0);
    // the figures the GPU tests of the tail were sized with (ld = dim there)
    {
        g_wk = false, g_ld = 32, g_count = 3000, g_ef = 60;
        KdbHeapPlan p{};
        CHECK(kdb_heap_plan_lds(false, 32, 3000, 60, &p));
        CHECK(p.hsize == 2048 && p.reg_results == 1 && p.nl_c == 1330 && p.cap_c == 2048);
        CHECK(kdb_heap_plan_lds(false, 768, 3000, 60, &p) && p.nl_c == 962);
        CHECK(kdb_heap_plan_lds(false, 32, 100000, 1200, &p) && p.nl_c == 4095 && p.cap_c == 19200 && p.hsize == 0 && p.reg_results == 0);
        CHECK(kdb_heap_plan_lds(false, 32, 2000, 60, &p) && p.cap_c == 2002); // clipped: overflow impossible
    }
    printf("ok\n");
    (void)refused;
    return 0;
}
