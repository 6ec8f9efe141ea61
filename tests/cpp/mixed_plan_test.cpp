// The rules of a mixed search launch (kektordb_amd/csrc/kdb_mixed_plan.h) on their own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/mixed_plan_test.cpp
// The host sizes a launch with these functions and the kernels apply them to every query; what is checked here are the figures
// themselves (literals taken from hnsw_index.go:387-399 and :2377-2380 and from the beam classes 64 | 128 | 256 | LDS), the edges
// of the validity and admission predicates, and that the stride of an open launch keeps its buffer inside the pin limit.
#include "kdb_mixed_plan.h"

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

// (usable in constant expressions: the kernels' launchers and static_asserts rely on it)
static_assert(kdb_mixed_effective_ef(10, 20, false) == 20, "ef = max(efSearch, k)");
static_assert(kdb_mixed_ef_cap(65) == 128, "the top of the class");

int main() {
    // effective ef: ef < k, ef == 0, ef == k, ef > k
    CHECK(kdb_mixed_effective_ef(5, 10, false) == 10);
    CHECK(kdb_mixed_effective_ef(0, 10, false) == 10);
    CHECK(kdb_mixed_effective_ef(0, 1, false) == 1);
    CHECK(kdb_mixed_effective_ef(10, 10, false) == 10);
    CHECK(kdb_mixed_effective_ef(64, 10, false) == 64);
    CHECK(kdb_mixed_effective_ef(0, 0, false) == 0);
    // the refine boost: 2 ef inside [80, 200], never below the ef asked for -- and it comes BEFORE max(ef, k)
    CHECK(kdb_mixed_boosted_ef(10, true) == 80);
    CHECK(kdb_mixed_boosted_ef(40, true) == 80);
    CHECK(kdb_mixed_boosted_ef(100, true) == 200);
    CHECK(kdb_mixed_boosted_ef(150, true) == 200);
    CHECK(kdb_mixed_boosted_ef(0, true) == 80);
    CHECK(kdb_mixed_boosted_ef(41, true) == 82);
    CHECK(kdb_mixed_boosted_ef(200, true) == 200);
    CHECK(kdb_mixed_boosted_ef(201, true) == 201);
    CHECK(kdb_mixed_boosted_ef(0xffffffffu, true) == 0xffffffffu);
    CHECK(kdb_mixed_boosted_ef(0x80000001u, true) == 0x80000001u);
    CHECK(kdb_mixed_boosted_ef(150, false) == 150);
    CHECK(kdb_mixed_effective_ef(10, 5, true) == 80);
    CHECK(kdb_mixed_effective_ef(40, 100, true) == 100);
    CHECK(kdb_mixed_effective_ef(100, 100, true) == 200);
    CHECK(kdb_mixed_effective_ef(150, 256, true) == 256);
    // class and capacity on both sides of every boundary
    CHECK(kdb_mixed_beam_class(1) == 1 && kdb_mixed_ef_cap(1) == 64);
    CHECK(kdb_mixed_beam_class(64) == 1 && kdb_mixed_ef_cap(64) == 64);
    CHECK(kdb_mixed_beam_class(65) == 2 && kdb_mixed_ef_cap(65) == 128);
    CHECK(kdb_mixed_beam_class(128) == 2 && kdb_mixed_ef_cap(128) == 128);
    CHECK(kdb_mixed_beam_class(129) == 4 && kdb_mixed_ef_cap(129) == 256);
    CHECK(kdb_mixed_beam_class(256) == 4 && kdb_mixed_ef_cap(256) == 256);
    CHECK(kdb_mixed_beam_class(257) == 0 && kdb_mixed_ef_cap(257) == 257);
    CHECK(kdb_mixed_beam_class(1200) == 0 && kdb_mixed_ef_cap(1200) == 1200);
    for (uint32_t e = 1; e <= 2000; e++) { // the capacity holds the ef it was made for, and asking again changes nothing
        CHECK(kdb_mixed_ef_cap(e) >= e);
        CHECK(kdb_mixed_ef_cap(kdb_mixed_ef_cap(e)) == kdb_mixed_ef_cap(e));
        CHECK(kdb_mixed_beam_class(kdb_mixed_ef_cap(e)) == kdb_mixed_beam_class(e));
    }
    // validity against (stride, ef_cap)
    CHECK(kdb_mixed_query_valid(10, 64, 10, 64));   // k == stride, ef == cap
    CHECK(!kdb_mixed_query_valid(11, 64, 10, 64));  // k == stride + 1
    CHECK(!kdb_mixed_query_valid(0, 64, 10, 64));   // k == 0
    CHECK(!kdb_mixed_query_valid(10, 65, 10, 64));  // ef one above the cap
    CHECK(kdb_mixed_query_valid(1, 1, 100, 1200));
    CHECK(!kdb_mixed_query_valid(10, 1201, 100, 1200));
    // admission of a late caller: the same predicate, plus equal flags and bytes per distance
    CHECK(kdb_mixed_admit(16, 128, 0x30u, 4, 16, 128, 0x30u, 4));
    CHECK(!kdb_mixed_admit(17, 128, 0x30u, 4, 16, 128, 0x30u, 4));
    CHECK(!kdb_mixed_admit(16, 129, 0x30u, 4, 16, 128, 0x30u, 4));
    CHECK(!kdb_mixed_admit(0, 10, 0x30u, 4, 16, 128, 0x30u, 4));
    CHECK(!kdb_mixed_admit(16, 128, 0x20u, 4, 16, 128, 0x30u, 4));
    CHECK(!kdb_mixed_admit(16, 128, 0x30u, 8, 16, 128, 0x30u, 4));
    CHECK(kdb_mixed_admit(3, 64, 0u, 8, 16, 128, 0u, 8));
    // stride of an open launch: whole steps of 16, capped by the capacity, 0 when nothing fits
    const size_t pin = KDB_MIXED_PIN_DEFAULT;
    CHECK(kdb_mixed_open_stride(5, 64, 768, 4, pin) == 16);
    CHECK(kdb_mixed_open_stride(16, 64, 768, 4, pin) == 16);
    CHECK(kdb_mixed_open_stride(17, 64, 768, 4, pin) == 32);
    CHECK(kdb_mixed_open_stride(60, 64, 768, 4, pin) == 64);
    CHECK(kdb_mixed_open_stride(100, 100, 768, 4, pin) == 100);  // (an LDS-beam capacity need not be a multiple of 16)
    CHECK(kdb_mixed_open_stride(300, 300, 96, 4, pin) == 300);
    CHECK(kdb_mixed_open_stride(0, 64, 768, 4, pin) == 0);
    CHECK(kdb_mixed_open_stride(65, 64, 768, 4, pin) == 0);      // no valid query has k > ef_cap
    // ... and the buffer of KDB_MIXED_GROUP_CAP queries stays inside the pin limit, at 1536 columns and k 256 too
    CHECK(KDB_MIXED_GROUP_CAP == 256u);
    for (uint32_t dim : {96u, 768u, 1536u, 4096u})
        for (uint32_t db : {4u, 8u})
            for (uint32_t cap : {64u, 128u, 256u, 300u, 1200u})
                for (uint32_t k = 1; k <= cap; k++) {
                    const uint32_t st = kdb_mixed_open_stride(k, cap, dim, db, pin);
                    if (st == 0u) {
                        CHECK(kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, dim, k, db) > pin);
                        continue;
                    }
                    CHECK(st >= k && st <= cap && st < k + KDB_MIXED_STRIDE_STEP);
                    CHECK(kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, dim, st, db) <= pin);
                    CHECK(kdb_mixed_query_valid(k, k, st, cap));
                }
    CHECK(kdb_mixed_open_stride(256, 256, 1536, 8, pin) == 256);
    CHECK(kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, 1536, 256, 8) <= pin);
    // a pin limit the rounded stride passes but the founders' own does not: no headroom rather than no launch
    {
        const size_t tight = kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, 768, 20, 4);
        CHECK(kdb_mixed_open_stride(20, 64, 768, 4, tight) == 20);
        CHECK(kdb_mixed_open_stride(20, 64, 768, 4, tight - 1) == 0);
    }
    printf("ok\n");
    return 0;
}
