// kdb_filter_plan.h -- the plan of filter_eval_kernel (filter.hip): tile geometry, program chunking, term validation and the layout
// of the staged programs.  Shared by the host (kdb_api_filter.hip plans and validates with it) and the kernel (which indexes with it), so
// the two cannot disagree.  Plain C++, no HIP header: host and device under hipcc, and tests/cpp/filter_plan_test.cpp builds it alone.
//
// GEOMETRY.  One lane per id, one wave per workgroup.  A wave's ballot of a program's verdict over 64 consecutive ids is one word of
// that program's list.  A wave takes a TILE of KDB_FILTER_TILE_WORDS consecutive words (x 64 ids) and a CHUNK of up to
// KDB_FILTER_CHUNK consecutive programs.  It goes through the tile in PASSES of `wp` words: the columns the chunk reads are fetched
// ONCE per word into LDS cells (8 bytes per lane, word and column), then every program of the chunk runs over the whole pass -- its
// terms fetched once per pass, each term compared against the wp cells of a lane into one bit per word (kdb_filter_run_words) --
// and its ballots are parked in LDS; after the tile's last word sixteen lanes per program store its KDB_FILTER_TILE_WORDS words as
// one contiguous run of 128 bytes.  wp is the whole tile while the chunk reads at most 4 columns, 8 words up to 8, 4 words up to
// 16 (kdb_filter_pass_words): the cells never take more than 32 KB.  The grid is (tiles, chunks).  Tiles cover words_per_list, not
// (count >> 6) + 1: ids above count are not live, so padding words are written as zeros by the same code.
#ifndef KDB_FILTER_PLAN_H
#define KDB_FILTER_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/kektor_hip.h"

#if defined(__HIPCC__)
#define KDB_FILTER_HD __host__ __device__
#else
#define KDB_FILTER_HD
#endif

constexpr uint32_t KDB_FILTER_WAVE = 64u;
constexpr uint32_t KDB_FILTER_TILE_WORDS = 16u;                                      // words of a list one wave writes: one 128-byte run
constexpr uint32_t KDB_FILTER_TILE_IDS = KDB_FILTER_TILE_WORDS * KDB_FILTER_WAVE;    // 1024 ids
constexpr uint32_t KDB_FILTER_CHUNK = 32u;                                           // programs that share one fetch of the columns
constexpr uint32_t KDB_FILTER_MAX_ID = 0x3fffffffu;                                  // "Conventions": at most 2^30 - 1 ids per index
static_assert(KDB_FILTER_TILE_WORDS * 8u >= 128u, "a wave's stores are runs of at least 128 bytes per list");
static_assert(KDB_FILTER_WAVE % KDB_FILTER_TILE_WORDS == 0u, "the write-out gives each program a group of TILE_WORDS lanes");
static_assert(KDB_FILTER_CHUNK % (KDB_FILTER_WAVE / KDB_FILTER_TILE_WORDS) == 0u, "whole rounds of the write-out");
static_assert(sizeof(kdb_filter_term) == 16u, "kdb_filter_term is 16 bytes");
// LDS of one workgroup (= one wave): the ballots of the chunk | the column cells of one pass.  A chunk that reads nc columns goes
// through its tile wp = kdb_filter_pass_words(nc) words at a time; cell (column slot s, word w of the pass, lane) is 8 bytes at
// index (s * wp + w) * 64 + lane, where s counts the chunk's columns in ascending slot order (kdb_filter_dense_slot).
constexpr uint32_t KDB_FILTER_LDS_BALLOT_BYTES = KDB_FILTER_CHUNK * KDB_FILTER_TILE_WORDS * 8u;
constexpr uint32_t KDB_FILTER_LDS_CELL_BYTES_MAX = 32u * 1024u;
KDB_FILTER_HD constexpr uint32_t kdb_filter_pass_words(uint32_t nc) { return nc <= 4u ? 16u : nc <= 8u ? 8u : 4u; }
KDB_FILTER_HD constexpr uint32_t kdb_filter_cell_bytes(uint32_t nc) { return nc * kdb_filter_pass_words(nc) * KDB_FILTER_WAVE * 8u; }
KDB_FILTER_HD constexpr uint32_t kdb_filter_lds_bytes(uint32_t nc) { return KDB_FILTER_LDS_BALLOT_BYTES + kdb_filter_cell_bytes(nc); }
KDB_FILTER_HD constexpr uint32_t kdb_filter_popcount(uint32_t m) {
    uint32_t n = 0;
    for (; m; m &= m - 1u) n++;
    return n;
}
// the cell slot of column `col` in a chunk whose columns are `mask`
KDB_FILTER_HD constexpr uint32_t kdb_filter_dense_slot(uint32_t mask, uint32_t col) { return kdb_filter_popcount(mask & ((1u << col) - 1u)); }
static_assert(kdb_filter_pass_words(4) == KDB_FILTER_TILE_WORDS && KDB_FILTER_TILE_WORDS % kdb_filter_pass_words(5) == 0u &&
              KDB_FILTER_TILE_WORDS % kdb_filter_pass_words(16) == 0u, "whole passes per tile");
static_assert(kdb_filter_cell_bytes(4) <= KDB_FILTER_LDS_CELL_BYTES_MAX && kdb_filter_cell_bytes(8) <= KDB_FILTER_LDS_CELL_BYTES_MAX &&
              kdb_filter_cell_bytes(KDB_MAX_COLUMNS) <= KDB_FILTER_LDS_CELL_BYTES_MAX, "four waves per CU and more, whatever the programs read");

// words of a list that covers ids 0..count
KDB_FILTER_HD constexpr uint64_t kdb_filter_min_words(uint32_t count) { return ((uint64_t)count >> 6) + 1u; }
// tiles of a list of words_per_list words; tile t covers words [first, first + n)
KDB_FILTER_HD constexpr uint64_t kdb_filter_tiles(uint64_t words_per_list) { return (words_per_list + KDB_FILTER_TILE_WORDS - 1u) / KDB_FILTER_TILE_WORDS; }
KDB_FILTER_HD constexpr uint64_t kdb_filter_tile_first_word(uint64_t tile) { return tile * KDB_FILTER_TILE_WORDS; }
KDB_FILTER_HD constexpr uint32_t kdb_filter_tile_words(uint64_t tile, uint64_t words_per_list) {
    const uint64_t first = kdb_filter_tile_first_word(tile);
    if (first >= words_per_list) return 0u;
    const uint64_t left = words_per_list - first;
    return left < KDB_FILTER_TILE_WORDS ? (uint32_t)left : KDB_FILTER_TILE_WORDS;
}
// chunks of P programs; chunk c covers programs [first, first + n)
KDB_FILTER_HD constexpr uint32_t kdb_filter_chunks(uint32_t P) { return (P + KDB_FILTER_CHUNK - 1u) / KDB_FILTER_CHUNK; }
KDB_FILTER_HD constexpr uint32_t kdb_filter_chunk_first(uint32_t chunk) { return chunk * KDB_FILTER_CHUNK; }
KDB_FILTER_HD constexpr uint32_t kdb_filter_chunk_programs(uint32_t chunk, uint32_t P) {
    const uint32_t first = kdb_filter_chunk_first(chunk);
    if (first >= P) return 0u;
    return P - first < KDB_FILTER_CHUNK ? P - first : KDB_FILTER_CHUNK;
}
// the largest words_per_list a call accepts: lists are addressed with 64-bit offsets; this bounds the grid (2^26 tiles)
constexpr uint64_t KDB_FILTER_MAX_WORDS = (uint64_t)1 << 30;

// What the call stages for the kernel, in one buffer: the terms of all programs | prog_offsets [P + 1] | the columns every chunk
// reads, one 32-bit mask per chunk (bit c = slot c) | the column table: KDB_MAX_COLUMNS device addresses (64-bit) and behind them
// KDB_MAX_COLUMNS kinds (32-bit).  Offsets in bytes, 64-bit exact, every region on a 256-byte boundary.
struct KdbFilterStage {
    uint64_t o_terms, o_offsets, o_masks, o_cols, total;
};
constexpr uint64_t KDB_FILTER_COLTAB_BYTES = (uint64_t)KDB_MAX_COLUMNS * (8u + 4u);
KDB_FILTER_HD constexpr uint64_t kdb_filter_align(uint64_t b) { return (b + 255u) & ~(uint64_t)255u; }
KDB_FILTER_HD constexpr KdbFilterStage kdb_filter_stage(uint64_t n_terms, uint32_t P) {
    KdbFilterStage L{};
    L.o_terms = 0;
    L.o_offsets = kdb_filter_align(n_terms * sizeof(kdb_filter_term));
    L.o_masks = L.o_offsets + kdb_filter_align(((uint64_t)P + 1u) * 4u);
    L.o_cols = L.o_masks + kdb_filter_align((uint64_t)kdb_filter_chunks(P) * 4u);
    L.total = L.o_cols + kdb_filter_align(KDB_FILTER_COLTAB_BYTES);
    return L;
}
// where list p starts, in words
KDB_FILTER_HD constexpr uint64_t kdb_filter_list_word(uint32_t p, uint64_t words_per_list) { return (uint64_t)p * words_per_list; }

// ---- validation -------------------------------------------------------------------------------------------------------------
enum {
    KDB_FILTER_OK = 0,
    KDB_FILTER_BAD_COUNTS = 1,   // P outside 1..KDB_FILTER_MAX_PROGRAMS
    KDB_FILTER_BAD_OFFSETS = 2,  // prog_offsets[0] != 0 or not ascending
    KDB_FILTER_BAD_LENGTH = 3,   // a program of 0 or more than KDB_FILTER_MAX_TERMS terms
    KDB_FILTER_BAD_OP = 4,
    KDB_FILTER_BAD_FLAGS = 5,    // unknown bits, OR_NEXT together with END_BLOCK, NOT inside a clause
    KDB_FILTER_BAD_SLOT = 6,     // column >= KDB_MAX_COLUMNS, an empty slot, or a slot of the other kind
    KDB_FILTER_BAD_VALUE = 7,    // NaN operand, CODE_EQ against code 0
    KDB_FILTER_NO_END = 8        // the program's last term lacks END_BLOCK
};
KDB_FILTER_HD constexpr uint32_t kdb_filter_op_kind(uint32_t op) { // the column kind an op reads; 0: none
    return op >= KDB_FOP_F64_EQ && op <= KDB_FOP_F64_GE ? (uint32_t)KDB_COL_F64 : op == KDB_FOP_CODE_EQ ? (uint32_t)KDB_COL_CODE : 0u;
}
// one program: terms[0..n); col_kind[KDB_MAX_COLUMNS] = the kind of every slot of the index, 0 = empty.  *cols_used gains the slots read.
inline int kdb_filter_validate_program(const kdb_filter_term *terms, uint64_t n, const uint32_t *col_kind, uint32_t *cols_used) {
    if (n == 0 || n > KDB_FILTER_MAX_TERMS) return KDB_FILTER_BAD_LENGTH;
    bool clause_open = false;
    for (uint64_t i = 0; i < n; i++) {
        const kdb_filter_term &t = terms[i];
        if (t.op > KDB_FOP_CODE_EQ) return KDB_FILTER_BAD_OP;
        if (t.flags & ~(uint32_t)(KDB_FT_OR_NEXT | KDB_FT_NOT | KDB_FT_END_BLOCK)) return KDB_FILTER_BAD_FLAGS;
        if ((t.flags & KDB_FT_OR_NEXT) && (t.flags & KDB_FT_END_BLOCK)) return KDB_FILTER_BAD_FLAGS;
        if ((t.flags & KDB_FT_NOT) && clause_open) return KDB_FILTER_BAD_FLAGS;
        const uint32_t kind = kdb_filter_op_kind(t.op);
        if (kind) {
            if (t.col >= KDB_MAX_COLUMNS || col_kind[t.col] != kind) return KDB_FILTER_BAD_SLOT;
            if (kind == KDB_COL_F64 && t.value != t.value) return KDB_FILTER_BAD_VALUE;
            if (kind == KDB_COL_CODE && t.code == 0u) return KDB_FILTER_BAD_VALUE;
            if (cols_used) *cols_used |= 1u << t.col;
        }
        clause_open = (t.flags & KDB_FT_OR_NEXT) != 0;
    }
    return (terms[n - 1].flags & KDB_FT_END_BLOCK) ? KDB_FILTER_OK : KDB_FILTER_NO_END;
}
// a whole call; chunk_masks: NULL or kdb_filter_chunks(P) words that receive the slots each chunk reads.  *bad_program: where it failed.
inline int kdb_filter_validate(const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P, const uint32_t *col_kind,
                               uint32_t *chunk_masks, uint32_t *bad_program) {
    if (bad_program) *bad_program = 0;
    if (P == 0 || P > KDB_FILTER_MAX_PROGRAMS) return KDB_FILTER_BAD_COUNTS;
    if (prog_offsets[0] != 0u) return KDB_FILTER_BAD_OFFSETS;
    if (chunk_masks)
        for (uint32_t c = 0; c < kdb_filter_chunks(P); c++) chunk_masks[c] = 0u;
    for (uint32_t p = 0; p < P; p++) {
        if (bad_program) *bad_program = p;
        if (prog_offsets[p + 1] < prog_offsets[p]) return KDB_FILTER_BAD_OFFSETS;
        uint32_t used = 0;
        const int rc = kdb_filter_validate_program(terms + prog_offsets[p], (uint64_t)prog_offsets[p + 1] - prog_offsets[p], col_kind, &used);
        if (rc) return rc;
        if (chunk_masks) chunk_masks[p / KDB_FILTER_CHUNK] |= used;
    }
    return KDB_FILTER_OK;
}
inline const char *kdb_filter_strerror(int rc) {
    switch (rc) {
    case KDB_FILTER_OK: return "ok";
    case KDB_FILTER_BAD_COUNTS: return "P must be 1..4096";
    case KDB_FILTER_BAD_OFFSETS: return "prog_offsets must start at 0 and ascend";
    case KDB_FILTER_BAD_LENGTH: return "a program has 1..64 terms";
    case KDB_FILTER_BAD_OP: return "unknown op";
    case KDB_FILTER_BAD_FLAGS: return "bad flags (unknown bit, OR_NEXT with END_BLOCK, or NOT inside a clause)";
    case KDB_FILTER_BAD_SLOT: return "the term's column is not a live slot of the kind its op reads";
    case KDB_FILTER_BAD_VALUE: return "NaN operand or code 0";
    case KDB_FILTER_NO_END: return "the last term of a program must carry KDB_FT_END_BLOCK";
    }
    return "?";
}

// The verdict of one program on W <= 32 ids at once -- one id of each of W consecutive words -- from their column cells:
// cell(col, w) returns the 8 bytes staged for column `col` of the id in word w (a double's bits for KDB_COL_F64; the code in the low
// word for KDB_COL_CODE).  Bit w of the result is the program's value for that id, without live: the caller ANDs.  ONE statement of
// the semantics: the kernel calls it with LDS cells and the words of a pass, filter_plan_test with arrays; every boolean of the
// definition (term, clause, NOT, block, program) is a W-bit mask here.
template <typename Cell>
KDB_FILTER_HD inline uint32_t kdb_filter_run_words(const kdb_filter_term *terms, uint32_t n, uint32_t W, Cell cell) {
    const uint32_t all = W >= 32u ? 0xffffffffu : (1u << W) - 1u;
    uint32_t prog = 0u, block = all, clause = 0u;
    bool inv = false, first = true;
    for (uint32_t i = 0; i < n; i++) {
        // the term as two 64-bit words (little endian: op | flags << 8 | col << 16 | code << 32, then the double's bits): on the device
        // ONE 16-byte load through the scalar cache -- field by field the byte- and half-sized members would be vector loads
        uint64_t raw[2];
        __builtin_memcpy(raw, terms + i, 16);
        const uint32_t op = (uint32_t)(raw[0] & 0xffu), flags = (uint32_t)((raw[0] >> 8) & 0xffu), col = (uint32_t)((raw[0] >> 16) & 0xffffu);
        const uint32_t code = (uint32_t)(raw[0] >> 32);
        double value;
        __builtin_memcpy(&value, &raw[1], 8);
        uint32_t v = 0u;
        if (op == KDB_FOP_CODE_EQ) {
            for (uint32_t w = 0; w < W; w++) v |= (uint32_t)((uint32_t)cell(col, w) == code) << w;
        } else if (op != KDB_FOP_NEVER) {
            for (uint32_t w = 0; w < W; w++) {
                const uint64_t bits = cell(col, w);
                double x;
                __builtin_memcpy(&x, &bits, 8);
                const bool t = op == KDB_FOP_F64_EQ ? x == value : op == KDB_FOP_F64_LT ? x < value : op == KDB_FOP_F64_LE ? x <= value
                               : op == KDB_FOP_F64_GT ? x > value : x >= value;
                v |= (uint32_t)t << w;
            }
        }
        if (first) {
            clause = v;
            inv = (flags & KDB_FT_NOT) != 0u;
        } else {
            clause |= v;
        }
        first = false;
        if (!(flags & KDB_FT_OR_NEXT)) {
            block &= inv ? ~clause : clause;
            first = true;
            if (flags & KDB_FT_END_BLOCK) {
                prog |= block;
                block = all;
            }
        }
    }
    return prog & all;
}
// ... and on one id
template <typename Cell>
KDB_FILTER_HD inline bool kdb_filter_run(const kdb_filter_term *terms, uint32_t n, Cell cell) {
    return kdb_filter_run_words(terms, n, 1u, [&](uint32_t col, uint32_t) { return cell(col); }) != 0u;
}

// ---- routing of a filtered request (kdb_search_filtered, kdb_api_filter.hip) -- host only ------------------------------------------------
// The route of one program from its cardinality: 2 = it matches nothing (answered by the host), 1 = the exact scan, 0 = the walk.
// The rule of the micro-batcher's takes_flat_scan (kektor_hip.hpp), per program; flat_max_k is the exact scan's limit (KDB_FLAT_MAX_K).
inline uint8_t kdb_filter_route_of(uint32_t card, uint32_t count, uint32_t k, double flat_selectivity, uint32_t flat_max_k) {
    return card == 0 ? 2 : (count > 0 && k <= flat_max_k && (double)card < flat_selectivity * (double)count) ? 1 : 0;
}
// The plan of one request: the order the queries are staged and run in -- the walked ones (no filter, or a program on route 0) in
// caller order, then the scanned ones program by program, in caller order inside a program -- and what the launches need beside it.
struct KdbFilterRoute {
    std::vector<uint8_t> route_p;        // [P] the route of every program
    std::vector<uint32_t> order;         // [n_walk + n_scan] caller index of the i-th staged query
    std::vector<uint32_t> of_query;      // [n_walk] the program (or KDB_NO_FILTER) of every walked query
    std::vector<uint32_t> scan_progs;    // the programs that have scanned queries, ascending
    std::vector<uint32_t> group_offsets; // [scan_progs.size() + 1] where each one's queries start among the scanned
    uint32_t n_walk = 0, n_scan = 0;
    uint8_t route_of_query(uint32_t prog) const { return prog == KDB_NO_FILTER ? 0 : route_p[prog]; }
};
inline KdbFilterRoute kdb_filter_route(const uint32_t *card, uint32_t P, const uint32_t *prog_of_query, uint32_t B, uint32_t count, uint32_t k,
                                       double flat_selectivity, uint32_t flat_max_k) {
    KdbFilterRoute R;
    R.route_p.resize(P);
    for (uint32_t p = 0; p < P; p++) R.route_p[p] = kdb_filter_route_of(card[p], count, k, flat_selectivity, flat_max_k);
    R.group_offsets.assign(1, 0u);
    R.order.reserve(B);
    for (uint32_t b = 0; b < B; b++)
        if (R.route_of_query(prog_of_query[b]) == 0) {
            R.order.push_back(b);
            R.of_query.push_back(prog_of_query[b]);
        }
    R.n_walk = (uint32_t)R.order.size();
    std::vector<std::vector<uint32_t>> by_prog(P);
    for (uint32_t b = 0; b < B; b++)
        if (R.route_of_query(prog_of_query[b]) == 1) by_prog[prog_of_query[b]].push_back(b);
    for (uint32_t p = 0; p < P; p++)
        if (!by_prog[p].empty()) {
            R.scan_progs.push_back(p);
            R.order.insert(R.order.end(), by_prog[p].begin(), by_prog[p].end());
            R.group_offsets.push_back((uint32_t)R.order.size() - R.n_walk);
        }
    R.n_scan = (uint32_t)R.order.size() - R.n_walk;
    return R;
}

#endif
