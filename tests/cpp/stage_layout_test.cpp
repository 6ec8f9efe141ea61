// The carver and the region list of the staging buffers (kektordb_amd/csrc/kdb_stage.h) on their own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/stage_layout_test.cpp
#include "kdb_stage.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

// ---- the region list (KdbStage) over a heap "device" buffer, memcpy as the copy functor -----------------------------------
struct Decl { // one declaration: 0 = in, 1 = out, 2 = device only; `present`: the host pointer is given
    int kind;
    size_t bytes;
    bool present;
};

static void check_stage(const std::vector<Decl> &decls) {
    const size_t n = decls.size();
    std::vector<std::vector<unsigned char>> host(n); // sources of the inputs, destinations of the outputs
    KdbStage st;
    KdbCarver cv; // the same sequence of take() calls
    std::vector<KdbRegion> r(n);
    std::vector<size_t> want_off(n);
    size_t present_in = 0, present_out = 0;
    for (size_t i = 0; i < n; i++) {
        const Decl &d = decls[i];
        host[i].assign(d.bytes ? d.bytes : 1, 0);
        for (size_t j = 0; j < host[i].size(); j++) host[i][j] = d.kind == 0 ? (unsigned char)(31 * i + 7 * j + 1) : 0xee;
        void *p = d.present ? host[i].data() : nullptr;
        r[i] = d.kind == 0 ? st.in(p, d.bytes) : d.kind == 1 ? st.out(p, d.bytes) : st.dev(d.bytes);
        const bool there = d.kind == 2 ? d.bytes != 0 : d.present && d.bytes != 0;
        want_off[i] = cv.take(there ? d.bytes : 0);
        CHECK(r[i].off == want_off[i] && r[i].bytes == (there ? d.bytes : 0)); // an absent region takes nothing
        present_in += there && d.kind == 0;
        present_out += there && d.kind == 1;
    }
    CHECK(st.total() == cv.total() && !st.overflow);
    std::vector<unsigned char> dev(st.total() + 1, 0xcd);
    unsigned char *const base = dev.data();
    size_t end = 0;
    for (size_t i = 0; i < n; i++) { // null exactly when absent; regions never overlap
        if (!r[i].bytes) {
            CHECK(r[i].at<unsigned char>(base) == nullptr);
            continue;
        }
        CHECK(r[i].at<unsigned char>(base) == base + r[i].off && r[i].off % 256 == 0);
        CHECK(r[i].off >= end && r[i].off + r[i].bytes <= st.total());
        end = r[i].off + r[i].bytes;
    }
    size_t calls = 0;
    auto copy = [&](void *dst, const void *src, size_t bytes) {
        calls++;
        memcpy(dst, src, bytes);
        return 0;
    };
    CHECK(st.copy_in(base, copy) == 0 && calls == present_in); // one copy per present input, none for anything else
    for (size_t i = 0; i < n; i++)
        if (decls[i].kind == 0 && r[i].bytes) CHECK(memcmp(r[i].at<unsigned char>(base), host[i].data(), r[i].bytes) == 0); // byte for byte where the typed pointer points
    CHECK(dev[st.total()] == 0xcd);
    for (size_t i = 0; i < n; i++) // what the "kernel" leaves in every output region
        if (decls[i].kind == 1 && r[i].bytes)
            for (size_t j = 0; j < r[i].bytes; j++) r[i].at<unsigned char>(base)[j] = (unsigned char)(17 * i + 3 * j + 5);
    calls = 0;
    CHECK(st.copy_out(base, copy) == 0 && calls == present_out);
    for (size_t i = 0; i < n; i++) {
        if (decls[i].kind != 1) continue;
        for (size_t j = 0; j < host[i].size(); j++) // a present output arrived; an absent one's buffer was never touched
            CHECK(host[i][j] == (r[i].bytes ? (unsigned char)(17 * i + 3 * j + 5) : 0xee));
    }
    // the first error of the functor ends the walk and is what the call returns
    calls = 0;
    const int rc = st.copy_in(base, [&](void *, const void *, size_t) { return ++calls == 2 ? 42 : 0; });
    CHECK(present_in < 2 ? (rc == 0 && calls == present_in) : (rc == 42 && calls == 2));
}

int main() {
    // ---- KdbStage: the consensus call's eight regions (ids, counts, queries, active | out, similarity, centroid, gram), every
    // optional one absent in turn, all of them absent, stride == 0 (the id lists and the similarities are empty)
    {
        const size_t B = 5, stride = 4, dim = 48, gw = stride + 1, bits = kdb_bits_bytes(300);
        const std::vector<Decl> all = {{0, B * stride * 4, true}, {0, B * 4, true},          {0, B * dim * 4, true}, {0, bits, true},
                                       {1, B * 40, true},         {1, B * stride * 8, true}, {1, B * dim * 4, true}, {1, B * gw * gw * 8, true}};
        check_stage(all);
        for (size_t skip : {1u, 2u, 3u, 5u, 6u, 7u}) {
            std::vector<Decl> d = all;
            d[skip].present = false;
            check_stage(d);
        }
        std::vector<Decl> none = all, empty = all;
        for (size_t skip : {1u, 2u, 3u, 5u, 6u, 7u}) none[skip].present = false;
        check_stage(none);
        empty[0].bytes = empty[5].bytes = 0;
        check_stage(empty);
        // a search on a turn (queries, k, ef, allow | ids, distances, counts), plain / mixed / filtered; device-only regions in between
        check_stage({{0, 5 * 48 * 4, true}, {0, 20, false}, {0, 20, false}, {0, bits, false}, {1, 80, true}, {1, 80, true}, {1, 20, true}});
        check_stage({{0, 5 * 48 * 4, true}, {0, 20, true}, {0, 20, true}, {0, bits, true}, {1, 80, true}, {1, 160, true}, {1, 20, true}});
        check_stage({{2, 1000}, {0, bits, true}, {2, 0}, {2, 77}, {1, 3, false}, {1, 3, true}});
        check_stage({});
    }
    {   // 64-bit sizes pass through exactly (the 2^33 case below, as regions; nothing is allocated: offsets and totals only)
        const uint32_t B = 1u << 20, k = 1024, dim = 768;
        int q_host, out_host; // (never dereferenced)
        KdbStage st;
        const KdbRegion q = st.in(&q_host, (size_t)B * dim * 4), allow = st.in(nullptr, kdb_bits_bytes(B)), ids = st.out(&out_host, (size_t)B * k * 4),
                        dist = st.out(&out_host, (size_t)B * k * 8), cnt = st.out(&out_host, (size_t)B * 4);
        CHECK(q.off == 0 && allow.bytes == 0 && allow.off == 3221225472ull && ids.off == 3221225472ull);
        CHECK(dist.off == 3221225472ull + 4294967296ull && dist.bytes == 8589934592ull);
        CHECK(cnt.off == 3221225472ull + 4294967296ull + 8589934592ull);
        CHECK(st.total() == 3221225472ull + 4294967296ull + 8589934592ull + 4194304ull);
        CHECK(q.bytes == 3221225472ull && ids.bytes == 4294967296ull && cnt.bytes == 4194304ull);
    }
    {   // more declarations than the list holds: the layout is still right, the copies refuse
        KdbStage st;
        int h;
        for (int i = 0; i < KdbStage::CAP + 1; i++) (void)st.in(&h, 4);
        CHECK(st.overflow && st.total() == (size_t)(KdbStage::CAP + 1) * 256);
        CHECK(st.copy_in(nullptr, [](void *, const void *, size_t) { return 0; }) != 0);
    }
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
