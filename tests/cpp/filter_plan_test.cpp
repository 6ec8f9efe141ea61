// The plan of filter_eval_kernel (kektordb_amd/csrc/kdb_filter_plan.h) on its own: no HIP, no library.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I kektordb_amd/csrc tests/cpp/filter_plan_test.cpp
// The host plans and validates with these functions and the kernel indexes with them; checked here: tiles cover every word of a
// list exactly once (walked word by word the way the kernel walks them, except at 2^30 - 1 ids where the tiles are summed), program
// chunks cover every program exactly once, the validation refuses what the header says it refuses, the staged layout's offsets
// are exact in 64 bits, the passes' LDS cells are disjoint and fit, and kdb_filter_run[_words] -- the ONE statement of a program's
// value -- against a few hand-evaluated programs, W ids at once against one id at a time.  And the routing plan of a filtered request
// (kdb_filter_route_of, kdb_filter_route): the rule at its edges, the plan against a brute-force restatement.
#include "kdb_filter_plan.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static_assert(kdb_filter_tiles(1) == 1 && kdb_filter_tiles(KDB_FILTER_TILE_WORDS + 1) == 2, "usable in constant expressions");
static_assert(KDB_FILTER_TILE_IDS == 1024 && KDB_FILTER_CHUNK == 32, "the figures the tests and the documents quote");

static kdb_filter_term term(uint8_t op, uint8_t flags, uint16_t col, uint32_t code, double value) {
    kdb_filter_term t;
    memset(&t, 0, sizeof t);
    t.op = op, t.flags = flags, t.col = col, t.code = code, t.value = value;
    return t;
}

static void tiles_cover(uint32_t count, uint64_t extra_words) {
    const uint64_t words = kdb_filter_min_words(count) + extra_words;
    CHECK(words == ((uint64_t)count >> 6) + 1 + extra_words);
    const uint64_t tiles = kdb_filter_tiles(words);
    if (words <= (1u << 22)) { // word by word, as the kernel's loops go
        std::vector<uint8_t> seen((size_t)words, 0);
        for (uint64_t t = 0; t < tiles; t++) {
            const uint64_t w0 = kdb_filter_tile_first_word(t);
            const uint32_t nw = kdb_filter_tile_words(t, words);
            CHECK(nw >= 1 && nw <= KDB_FILTER_TILE_WORDS);
            for (uint32_t w = 0; w < nw; w++) {
                CHECK(w0 + w < words);
                CHECK(seen[(size_t)(w0 + w)]++ == 0);
            }
        }
        for (uint64_t w = 0; w < words; w++) CHECK(seen[(size_t)w] == 1);
    } else { // consecutive, gap-free, summing to the list
        uint64_t next = 0;
        for (uint64_t t = 0; t < tiles; t++) {
            CHECK(kdb_filter_tile_first_word(t) == next);
            next += kdb_filter_tile_words(t, words);
        }
        CHECK(next == words);
    }
    CHECK(kdb_filter_tile_words(tiles, words) == 0); // nothing behind the last tile
    // the last id of the list's last needed word is count's word: id count lies inside the cover
    CHECK(((uint64_t)count >> 6) < words);
}

static void chunks_cover(uint32_t P) {
    std::vector<uint8_t> seen(P, 0);
    const uint32_t n = kdb_filter_chunks(P);
    for (uint32_t c = 0; c < n; c++) {
        const uint32_t p0 = kdb_filter_chunk_first(c), np = kdb_filter_chunk_programs(c, P);
        CHECK(np >= 1 && np <= KDB_FILTER_CHUNK);
        for (uint32_t j = 0; j < np; j++) {
            CHECK(p0 + j < P);
            CHECK(seen[p0 + j]++ == 0);
        }
    }
    for (uint32_t p = 0; p < P; p++) CHECK(seen[p] == 1);
    CHECK(kdb_filter_chunk_programs(n, P) == 0);
}

int main() {
    // ---- tiles
    const uint32_t T = KDB_FILTER_TILE_IDS;
    for (uint32_t count : {1u, 63u, 64u, 65u, T - 1, T, T + 1, 10000u, (1u << 30) - 1u})
        for (uint64_t extra : {0ull, 3ull}) tiles_cover(count, extra);
    CHECK(kdb_filter_tiles(kdb_filter_min_words(T - 1)) == 1 && kdb_filter_tiles(kdb_filter_min_words(T)) == 2);
    CHECK(kdb_filter_min_words((1u << 30) - 1u) == (1ull << 24));
    CHECK(kdb_filter_tiles(KDB_FILTER_MAX_WORDS) == (KDB_FILTER_MAX_WORDS / KDB_FILTER_TILE_WORDS) && kdb_filter_tiles(KDB_FILTER_MAX_WORDS) < (1ull << 31));
    // ---- chunks
    const uint32_t Cn = KDB_FILTER_CHUNK;
    for (uint32_t P : {1u, 2u, Cn - 1, Cn, Cn + 1, 130u, (uint32_t)KDB_FILTER_MAX_PROGRAMS}) chunks_cover(P);
    CHECK(kdb_filter_chunks(KDB_FILTER_MAX_PROGRAMS) == KDB_FILTER_MAX_PROGRAMS / Cn);
    // ---- the staged layout: 64-bit exact, aligned, disjoint, at the limits
    {
        const uint64_t nt = (uint64_t)KDB_FILTER_MAX_PROGRAMS * KDB_FILTER_MAX_TERMS;
        const KdbFilterStage L = kdb_filter_stage(nt, KDB_FILTER_MAX_PROGRAMS);
        CHECK(L.o_terms == 0 && L.o_offsets == nt * 16u);
        CHECK(L.o_masks == L.o_offsets + kdb_filter_align(4097ull * 4u));
        CHECK(L.o_cols == L.o_masks + kdb_filter_align(128ull * 4u));
        CHECK(L.total == L.o_cols + kdb_filter_align(KDB_MAX_COLUMNS * 12ull));
        CHECK(L.o_offsets % 256 == 0 && L.o_masks % 256 == 0 && L.o_cols % 256 == 0 && L.total % 256 == 0);
        const KdbFilterStage S = kdb_filter_stage(1, 1);
        CHECK(S.o_offsets == 256 && S.o_masks == 512 && S.o_cols == 768 && S.total == 1024);
        // a list offset beyond 32 bits
        CHECK(kdb_filter_list_word(4095, 1ull << 24) == 4095ull << 24);
        CHECK(kdb_filter_list_word(4095, KDB_FILTER_MAX_WORDS) == 4095ull << 30);
    }
    // ---- validation
    uint32_t kinds[KDB_MAX_COLUMNS] = {};
    kinds[0] = KDB_COL_F64, kinds[1] = KDB_COL_CODE;
    {
        const kdb_filter_term ok[] = {term(KDB_FOP_F64_EQ, KDB_FT_OR_NEXT | KDB_FT_NOT, 0, 0, 10.0), term(KDB_FOP_CODE_EQ, 0, 1, 7, 0),
                                      term(KDB_FOP_F64_GE, KDB_FT_END_BLOCK, 0, 0, -0.0), term(KDB_FOP_NEVER, KDB_FT_END_BLOCK, 99, 0, NAN)};
        uint32_t used = 0;
        CHECK(kdb_filter_validate_program(ok, 4, kinds, &used) == KDB_FILTER_OK && used == 3u);
        CHECK(kdb_filter_validate_program(ok, 2, kinds, nullptr) == KDB_FILTER_NO_END);   // the final END_BLOCK is missing
        CHECK(kdb_filter_validate_program(ok, 1, kinds, nullptr) == KDB_FILTER_NO_END);
        CHECK(kdb_filter_validate_program(ok, 0, kinds, nullptr) == KDB_FILTER_BAD_LENGTH);
        kdb_filter_term t = term(KDB_FOP_F64_LT, KDB_FT_END_BLOCK, 0, 0, 1.0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_OK);
        t.col = 1; // a code column under a numeric op
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_SLOT);
        t.col = 2; // an empty slot
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_SLOT);
        t.col = KDB_MAX_COLUMNS; // no such slot
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_SLOT);
        t.col = 65535;
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_SLOT);
        t = term(KDB_FOP_CODE_EQ, KDB_FT_END_BLOCK, 0, 3, 0); // a numeric column under CODE_EQ
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_SLOT);
        t = term(KDB_FOP_CODE_EQ + 1, KDB_FT_END_BLOCK, 0, 0, 0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_OP);
        t = term(255, KDB_FT_END_BLOCK, 0, 0, 0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_OP);
        t = term(KDB_FOP_F64_EQ, KDB_FT_END_BLOCK, 0, 0, NAN);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_VALUE);
        t = term(KDB_FOP_CODE_EQ, KDB_FT_END_BLOCK, 1, 0, 0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_VALUE);
        t = term(KDB_FOP_NEVER, KDB_FT_END_BLOCK | 8, 0, 0, 0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_FLAGS);
        t = term(KDB_FOP_NEVER, KDB_FT_END_BLOCK | KDB_FT_OR_NEXT, 0, 0, 0);
        CHECK(kdb_filter_validate_program(&t, 1, kinds, nullptr) == KDB_FILTER_BAD_FLAGS);
        const kdb_filter_term inner_not[] = {term(KDB_FOP_NEVER, KDB_FT_OR_NEXT, 0, 0, 0), term(KDB_FOP_NEVER, KDB_FT_NOT | KDB_FT_END_BLOCK, 0, 0, 0)};
        CHECK(kdb_filter_validate_program(inner_not, 2, kinds, nullptr) == KDB_FILTER_BAD_FLAGS);
        // 64 terms pass, 65 do not
        std::vector<kdb_filter_term> many(65, term(KDB_FOP_NEVER, 0, 0, 0, 0));
        many[63].flags = KDB_FT_END_BLOCK;
        many[64].flags = KDB_FT_END_BLOCK;
        CHECK(kdb_filter_validate_program(many.data(), 64, kinds, nullptr) == KDB_FILTER_OK);
        CHECK(kdb_filter_validate_program(many.data(), 65, kinds, nullptr) == KDB_FILTER_BAD_LENGTH);
        // whole calls: offsets, counts, the masks of the chunks, where it failed
        std::vector<kdb_filter_term> ts;
        std::vector<uint32_t> off(1, 0);
        for (uint32_t p = 0; p < Cn + 1; p++) {
            ts.push_back(p == Cn ? term(KDB_FOP_CODE_EQ, KDB_FT_END_BLOCK, 1, 1, 0) : term(KDB_FOP_F64_LT, KDB_FT_END_BLOCK, 0, 0, 1.0));
            off.push_back((uint32_t)ts.size());
        }
        uint32_t masks[2] = {77, 77}, bad = 99;
        CHECK(kdb_filter_validate(ts.data(), off.data(), Cn + 1, kinds, masks, &bad) == KDB_FILTER_OK);
        CHECK(masks[0] == 1u && masks[1] == 2u);
        CHECK(kdb_filter_validate(ts.data(), off.data(), 0, kinds, nullptr, &bad) == KDB_FILTER_BAD_COUNTS);
        CHECK(kdb_filter_validate(ts.data(), off.data(), KDB_FILTER_MAX_PROGRAMS + 1, kinds, nullptr, &bad) == KDB_FILTER_BAD_COUNTS);
        ts[5].flags = 0;
        CHECK(kdb_filter_validate(ts.data(), off.data(), Cn + 1, kinds, nullptr, &bad) == KDB_FILTER_NO_END && bad == 5);
        ts[5].flags = KDB_FT_END_BLOCK;
        off[3] = off[2]; // an empty program
        CHECK(kdb_filter_validate(ts.data(), off.data(), Cn + 1, kinds, nullptr, &bad) == KDB_FILTER_BAD_LENGTH && bad == 2);
        off[3] = 1; // descending
        CHECK(kdb_filter_validate(ts.data(), off.data(), Cn + 1, kinds, nullptr, &bad) == KDB_FILTER_BAD_OFFSETS && bad == 2);
        off[3] = 3;
        off[0] = 1;
        CHECK(kdb_filter_validate(ts.data(), off.data(), Cn + 1, kinds, nullptr, &bad) == KDB_FILTER_BAD_OFFSETS);
        for (int rc = 0; rc <= KDB_FILTER_NO_END; rc++) CHECK(strcmp(kdb_filter_strerror(rc), "?") != 0);
    }
    // ---- the value of a program: cells of one id (slot 0 numeric, slot 1 code)
    {
        auto run = [](const std::vector<kdb_filter_term> &p, double x, uint32_t code) {
            return kdb_filter_run(p.data(), (uint32_t)p.size(), [&](uint32_t c) -> uint64_t {
                uint64_t b = code;
                if (c == 0) memcpy(&b, &x, 8);
                return b;
            });
        };
        const uint8_t E = KDB_FT_END_BLOCK, O = KDB_FT_OR_NEXT, N = KDB_FT_NOT;
        // every op against 1.0, NaN (absent) never matches, -0.0 == 0.0
        const uint8_t ops[] = {KDB_FOP_F64_EQ, KDB_FOP_F64_LT, KDB_FOP_F64_LE, KDB_FOP_F64_GT, KDB_FOP_F64_GE};
        const bool at_half[] = {false, true, true, false, false}, at_one[] = {true, false, true, false, true}, at_two[] = {false, false, false, true, true};
        for (int i = 0; i < 5; i++) {
            const std::vector<kdb_filter_term> p = {term(ops[i], E, 0, 0, 1.0)};
            CHECK(run(p, 0.5, 0) == at_half[i] && run(p, 1.0, 0) == at_one[i] && run(p, 2.0, 0) == at_two[i] && !run(p, NAN, 0));
        }
        CHECK(run({term(KDB_FOP_F64_EQ, E, 0, 0, 0.0)}, -0.0, 0) && run({term(KDB_FOP_F64_EQ, E, 0, 0, -0.0)}, 0.0, 0));
        CHECK(!run({term(KDB_FOP_F64_EQ, E, 0, 0, 16777217.0)}, 16777216.0, 0) && !run({term(KDB_FOP_F64_EQ, E, 0, 0, 0.1)}, (double)0.1f, 0));
        CHECK(run({term(KDB_FOP_CODE_EQ, E, 1, 7, 0)}, NAN, 7) && !run({term(KDB_FOP_CODE_EQ, E, 1, 7, 0)}, NAN, 0));
        CHECK(!run({term(KDB_FOP_NEVER, E, 0, 0, 0)}, 1.0, 1) && run({term(KDB_FOP_NEVER, E | N, 0, 0, 0)}, 1.0, 1));
        // k != v with both alternatives: NOT (x == 10 OR code == 7); an absent node passes
        const std::vector<kdb_filter_term> ne = {term(KDB_FOP_F64_EQ, O | N, 0, 0, 10.0), term(KDB_FOP_CODE_EQ, E, 1, 7, 0)};
        CHECK(!run(ne, 10.0, 0) && !run(ne, NAN, 7) && run(ne, NAN, 0) && run(ne, 11.0, 3));
        // (x < 5 AND code == 2) OR (x >= 100)
        const std::vector<kdb_filter_term> ao = {term(KDB_FOP_F64_LT, 0, 0, 0, 5.0), term(KDB_FOP_CODE_EQ, E, 1, 2, 0), term(KDB_FOP_F64_GE, E, 0, 0, 100.0)};
        CHECK(run(ao, 1.0, 2) && !run(ao, 1.0, 3) && !run(ao, 7.0, 2) && run(ao, 100.0, 0) && !run(ao, NAN, 2));
        // NOT applies to its own clause only: (NOT code == 1) AND x > 0
        const std::vector<kdb_filter_term> na = {term(KDB_FOP_CODE_EQ, N, 1, 1, 0), term(KDB_FOP_F64_GT, E, 0, 0, 0.0)};
        CHECK(run(na, 1.0, 2) && !run(na, 1.0, 1) && !run(na, -1.0, 2) && !run(na, NAN, 0));
    }
    // ---- passes: the words a wave evaluates per fetch of the terms, the cells they need, the slot of a column inside a chunk
    {
        for (uint32_t nc = 0; nc <= KDB_MAX_COLUMNS; nc++) {
            const uint32_t wp = kdb_filter_pass_words(nc);
            CHECK(wp >= 4 && wp <= KDB_FILTER_TILE_WORDS && KDB_FILTER_TILE_WORDS % wp == 0);
            CHECK(kdb_filter_cell_bytes(nc) == nc * wp * 512u && kdb_filter_cell_bytes(nc) <= KDB_FILTER_LDS_CELL_BYTES_MAX);
            CHECK(kdb_filter_lds_bytes(nc) == 4096u + nc * wp * 512u && kdb_filter_lds_bytes(nc) <= 36u * 1024u);
        }
        CHECK(kdb_filter_pass_words(0) == 16 && kdb_filter_pass_words(4) == 16 && kdb_filter_pass_words(5) == 8 && kdb_filter_pass_words(8) == 8 &&
              kdb_filter_pass_words(9) == 4 && kdb_filter_pass_words(16) == 4);
        const uint32_t mask = 0x8109u; // slots 0, 3, 8, 15
        CHECK(kdb_filter_popcount(mask) == 4 && kdb_filter_popcount(0) == 0 && kdb_filter_popcount(0xffffu) == 16);
        CHECK(kdb_filter_dense_slot(mask, 0) == 0 && kdb_filter_dense_slot(mask, 3) == 1 && kdb_filter_dense_slot(mask, 8) == 2 && kdb_filter_dense_slot(mask, 15) == 3);
        // every (slot, word, lane) of a pass has a cell of its own inside the cells' bytes
        for (uint32_t nc : {1u, 4u, 5u, 8u, 9u, 16u}) {
            const uint32_t wp = kdb_filter_pass_words(nc);
            std::vector<uint8_t> seen((size_t)nc * wp * KDB_FILTER_WAVE, 0);
            for (uint32_t sl = 0; sl < nc; sl++)
                for (uint32_t w = 0; w < wp; w++)
                    for (uint32_t lane = 0; lane < KDB_FILTER_WAVE; lane++) {
                        const size_t at = (size_t)(sl * wp + w) * KDB_FILTER_WAVE + lane;
                        CHECK(at * 8 < kdb_filter_cell_bytes(nc) && seen[at]++ == 0);
                    }
        }
    }
    // ---- W ids at once == one id at a time, for every W the kernel uses and a program with every construct
    {
        const uint8_t E = KDB_FT_END_BLOCK, O = KDB_FT_OR_NEXT, N = KDB_FT_NOT;
        const std::vector<kdb_filter_term> p = {term(KDB_FOP_F64_EQ, O | N, 0, 0, 1.0), term(KDB_FOP_CODE_EQ, 0, 1, 2, 0), term(KDB_FOP_F64_LE, E, 0, 0, 0.1),
                                                term(KDB_FOP_NEVER, O, 0, 0, 0),        term(KDB_FOP_F64_GT, 0, 0, 0, 16777216.0), term(KDB_FOP_CODE_EQ, N | E, 1, 5, 0),
                                                term(KDB_FOP_F64_GE, 0, 0, 0, -0.0),    term(KDB_FOP_F64_LT, E, 0, 0, 0.5)};
        const double xs[] = {-1.0, -0.0, 0.0, 1.0, 0.1, (double)0.1f, 16777216.0, 16777217.0, NAN};
        for (uint32_t W : {1u, 3u, 4u, 8u, 11u, 16u, 32u}) {
            std::vector<double> x(W);
            std::vector<uint32_t> code(W);
            for (uint32_t round = 0; round < 54; round++) {
                for (uint32_t w = 0; w < W; w++) x[w] = xs[(round + 5 * w) % 9], code[w] = (round / 9 + w) % 6;
                auto cells = [&](uint32_t c, uint32_t w) -> uint64_t {
                    uint64_t b = code[w];
                    if (c == 0) memcpy(&b, &x[w], 8);
                    return b;
                };
                const uint32_t m = kdb_filter_run_words(p.data(), (uint32_t)p.size(), W, cells);
                CHECK(W == 32 || (m >> W) == 0);
                for (uint32_t w = 0; w < W; w++)
                    CHECK(((m >> w) & 1u) == (uint32_t)kdb_filter_run(p.data(), (uint32_t)p.size(), [&](uint32_t c) { return cells(c, w); }));
            }
        }
    }
    // ---- the route of one program (the rule of takes_flat_scan, kektor_hip.hpp): 2 = empty, 1 = exact scan, 0 = walk
    {
        const uint32_t MAXK = 1024u; // KDB_FLAT_MAX_K
        CHECK(kdb_filter_route_of(0, 1000, 10, 0.5, MAXK) == 2 && kdb_filter_route_of(0, 0, 10, 1.0, MAXK) == 2 && kdb_filter_route_of(0, 1000, 2000, 0.0, MAXK) == 2);
        // the comparison is strict: card == ceil(f * count) walks, one below it scans -- with f * count whole and not whole
        for (const auto &fc : {std::pair<double, uint32_t>{0.25, 1000u}, {0.1, 1003u}, {0.5, 7u}, {1.0 / 3.0, 100u}, {0.999, 123457u}}) {
            const uint32_t edge = (uint32_t)ceil(fc.first * (double)fc.second);
            CHECK(edge >= 2);
            CHECK(kdb_filter_route_of(edge, fc.second, 10, fc.first, MAXK) == 0);
            CHECK(kdb_filter_route_of(edge - 1, fc.second, 10, fc.first, MAXK) == 1);
        }
        CHECK(kdb_filter_route_of(5, 1000, 1024, 0.5, MAXK) == 1 && kdb_filter_route_of(5, 1000, 1025, 0.5, MAXK) == 0); // k at and above the scan's limit
        for (uint32_t card : {1u, 2u, 999u, 1000u}) CHECK(kdb_filter_route_of(card, 1000, 10, 0.0, MAXK) == 0);          // f == 0: nothing scans
        CHECK(kdb_filter_route_of(999, 1000, 10, 1.0, MAXK) == 1 && kdb_filter_route_of(1000, 1000, 10, 1.0, MAXK) == 0); // f == 1: all but the full list
        CHECK(kdb_filter_route_of(1, 0, 10, 1.0, MAXK) == 0 && kdb_filter_route_of(0, 0, 10, 1.0, MAXK) == 2);            // count == 0
    }
    // ---- the plan of a request against a brute-force restatement, a few thousand small random cases
    {
        unsigned long long x = 0x9e3779b97f4a7c15ull;
        auto rnd = [&](uint32_t n) { x ^= x << 13, x ^= x >> 7, x ^= x << 17; return (uint32_t)((x >> 33) % n); };
        uint32_t n_nothing = 0, n_both = 0;
        for (int round = 0; round < 4000; round++) {
            const uint32_t P = 1 + rnd(6), B = 1 + rnd(40), count = rnd(8) ? 1 + rnd(50) : 0, k = rnd(10) ? 1 + rnd(20) : 1020 + rnd(10);
            const double f = rnd(6) == 0 ? 0.0 : rnd(6) == 0 ? 1.0 : (double)rnd(1000) / 1000.0;
            std::vector<uint32_t> card(P), prog(B);
            for (uint32_t &c : card) c = rnd(3) == 0 ? 0 : rnd(count + 1);
            const uint32_t mode = rnd(8); // now and then: no query filtered, or every query on one program
            for (uint32_t &p : prog) p = mode == 0 ? KDB_NO_FILTER : mode == 1 ? 0 : rnd(4) == 0 ? KDB_NO_FILTER : rnd(P);
            const KdbFilterRoute R = kdb_filter_route(card.data(), P, prog.data(), B, count, k, f, 1024u);
            // the restatement: every query's route, straight from the rule
            CHECK(R.route_p.size() == P);
            std::vector<uint8_t> rq(B);
            for (uint32_t b = 0; b < B; b++) {
                rq[b] = prog[b] == KDB_NO_FILTER ? 0 : card[prog[b]] == 0 ? 2 : (count > 0 && k <= 1024u && (double)card[prog[b]] < f * (double)count) ? 1 : 0;
                CHECK(R.route_of_query(prog[b]) == rq[b]);
                if (prog[b] != KDB_NO_FILTER) CHECK(R.route_p[prog[b]] == rq[b]);
            }
            // order: a permutation of exactly the queries whose route is not 2
            std::vector<uint8_t> seen(B, 0);
            for (uint32_t b : R.order) {
                CHECK(b < B && rq[b] != 2 && seen[b]++ == 0);
            }
            uint32_t n_run = 0;
            for (uint32_t b = 0; b < B; b++) n_run += rq[b] != 2;
            CHECK(R.order.size() == n_run && R.n_walk + R.n_scan == n_run);
            // the first n_walk: the walked queries in caller order, with their program
            std::vector<uint32_t> walked;
            for (uint32_t b = 0; b < B; b++)
                if (rq[b] == 0) walked.push_back(b);
            CHECK(R.n_walk == walked.size() && R.of_query.size() == walked.size());
            for (uint32_t i = 0; i < R.n_walk; i++) CHECK(R.order[i] == walked[i] && R.of_query[i] == prog[walked[i]]);
            // the rest: grouped by ascending program, caller order inside a group, one entry of group_offsets per non-empty scanned program
            std::vector<uint32_t> progs;
            for (uint32_t p = 0; p < P; p++) {
                bool any = false;
                for (uint32_t b = 0; b < B; b++) any = any || (rq[b] == 1 && prog[b] == p);
                if (any) progs.push_back(p);
            }
            CHECK(R.scan_progs == progs);
            CHECK(R.group_offsets.size() == progs.size() + 1 && R.group_offsets.front() == 0 && R.group_offsets.back() == R.n_scan);
            for (size_t g = 0; g < progs.size(); g++) {
                CHECK(R.group_offsets[g] < R.group_offsets[g + 1]);
                std::vector<uint32_t> members;
                for (uint32_t b = 0; b < B; b++)
                    if (rq[b] == 1 && prog[b] == progs[g]) members.push_back(b);
                CHECK(R.group_offsets[g + 1] - R.group_offsets[g] == members.size());
                for (size_t j = 0; j < members.size(); j++) CHECK(R.order[R.n_walk + R.group_offsets[g] + j] == members[j]);
            }
            if (n_run == 0) { // a plan with nothing to run
                CHECK(R.n_walk + R.n_scan == 0 && R.order.empty() && R.scan_progs.empty() && R.group_offsets.size() == 1);
                n_nothing++;
            }
            n_both += R.n_walk && R.n_scan;
        }
        CHECK(n_nothing >= 20 && n_both >= 200); // the cases the assertions above are about did occur
    }
    printf("ok\n");
    return 0;
}
