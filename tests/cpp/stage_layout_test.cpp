// The carver of the staging buffers (kektordb_amd/csrc/kdb_stage.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/stage_layout_test.cpp
#include "kdb_stage.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

struct Region {
    size_t off, bytes;
};

// the properties every layout must have, whatever the sizes
static void check_layout(const std::vector<size_t> &sizes) {
    KdbCarver cv;
    std::vector<Region> r;
    for (size_t b : sizes) r.push_back({cv.take(b), b});
    CHECK(r.empty() || r[0].off == 0);
    size_t end = 0;
    for (size_t i = 0; i < r.size(); i++) {
        CHECK(r[i].off % 256 == 0);
        if (i) CHECK(r[i].off >= r[i - 1].off);
        if (r[i].bytes) {
            CHECK(r[i].off >= end); // no overlap with any non-empty region before it (offsets never decrease: `end` is the largest end)
            end = r[i].off + r[i].bytes;
        } else {                    // an empty region shares its offset with whatever comes next
            CHECK(i + 1 == r.size() ? cv.total() == r[i].off : r[i + 1].off == r[i].off);
        }
    }
    CHECK(cv.total() >= end);
    CHECK(cv.total() % 256 == 0);
}

int main() {
    check_layout({});
    check_layout({0});
    check_layout({1});
    check_layout({255, 256, 257});
    check_layout({0, 0, 7, 0, 513, 0});
    check_layout({1000003, 0, 17, 4096, 0, 1, 1, 0});
    unsigned long long x = 88172645463325252ull; // xorshift64: sizes of every magnitude, many of them empty
    for (int round = 0; round < 2000; round++) {
        std::vector<size_t> sizes;
        for (int i = 0; i < 9; i++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            sizes.push_back(x % 3 == 0 ? 0 : (size_t)(x >> (20 + x % 40)));
        }
        check_layout(sizes);
    }
    {   // take(0) takes nothing
        KdbCarver cv;
        const size_t a = cv.take(300), e = cv.take(0), b = cv.take(1);
        CHECK(a == 0 && e == 512 && b == 512 && cv.total() == 768);
    }
    {   // a million queries, k = 1024, 8-byte distances: exact 64-bit offsets (B * k * 8 = 2^33: nothing may pass through 32 bits)
        const uint32_t B = 1u << 20, k = 1024, dim = 768;
        KdbCarver cv;
        const size_t o_q = cv.take((size_t)B * dim * 4), o_allow = cv.take(0), o_ids = cv.take((size_t)B * k * 4), o_dist = cv.take((size_t)B * k * 8),
                     o_cnt = cv.take((size_t)B * 4);
        CHECK(o_q == 0ull);
        CHECK(o_allow == 3221225472ull && o_ids == 3221225472ull); // 2^20 * 768 * 4
        CHECK(o_dist == 3221225472ull + 4294967296ull);            // + 2^32
        CHECK(o_cnt == 3221225472ull + 4294967296ull + 8589934592ull); // + 2^33
        CHECK(cv.total() == 3221225472ull + 4294967296ull + 8589934592ull + 4194304ull);
        KdbCarver odd; // sizes that are no multiple of 256, above 2^32
        CHECK(odd.take(((size_t)1 << 32) + 1) == 0 && odd.take(3) == ((size_t)1 << 32) + 256 && odd.total() == ((size_t)1 << 32) + 512);
    }
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 0xffffffffu}) // the expression the carver's users wrote out before
        CHECK(kdb_bits_bytes(n) == ((size_t)(n >> 6) + 1) * 8);
    CHECK(kdb_bits_bytes(0) == 8 && kdb_bits_bytes(63) == 8 && kdb_bits_bytes(64) == 16 && kdb_bits_bytes(0xffffffffu) == 536870912ull);
    printf("ok\n");
    return 0;
}
