// filter.hip -- metadata filters on the device: the allow lists that DB.FindIDsByFilter (pkg/core/core.go:1766-1839,
// evaluateBooleanFilter :1900-2034) builds on the host as roaring bitmaps, written by ONE streaming kernel from per-id metadata
// columns in HBM, in the dense layout every filtered entry point takes.
//
//   col_fill_kernel      entries of a column set to "absent" (NaN / code 0): a slot's first upload, the tail after a reserve
//   filter_eval_kernel   (tile, chunk) per wave: P predicate programs over the columns -> P bitsets + P cardinalities
//
// Semantics, geometry, validation and the staged layout are kdb_filter_plan.h's; this file holds what needs the device.
#include "kdb_internal.h"
#include "kdb_filter_plan.h"
#include <errno.h>
#include <locale.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define KDB_GLOBAL_AS __attribute__((address_space(1)))

namespace {

__global__ void __launch_bounds__(256) col_fill_kernel(void *col, uint32_t kind, size_t first, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (kind == KDB_COL_F64) reinterpret_cast<uint64_t *>(col)[first + i] = 0x7ff8000000000000ull; // quiet NaN: no numeric value
    else reinterpret_cast<uint32_t *>(col)[first + i] = 0u;
}

// One wave per workgroup; blockIdx.x = tile (KDB_FILTER_TILE_WORDS words of every list), blockIdx.y = chunk of programs.  The tile
// is taken in passes of wp = kdb_filter_pass_words(columns the chunk reads) words (kdb_filter_plan.h):
//   stage     per word of the pass, lane = one id: live = 1 <= id <= count and the index's deleted bit clear (one bit per word in
//             a lane register); every column the chunk reads (chunk_masks) is fetched once -- coalesced, 8 or 4 bytes per lane --
//             into the lane's own LDS cell, "absent" for an id that is not live;
//   evaluate  every program of the chunk runs over the pass (kdb_filter_run_words: control flow and terms are wave-uniform, a term is
//             one 16-byte load through the scalar cache PER PASS, compared against the lane's wp cells into one bit per word); the
//             ballot of bit w is the list's word, kept by lane w and parked in LDS with one store per program;
//   write-out after the last pass: 16 lanes per program, four programs per round: each group stores the program's 16 words as one
//             128-byte run and adds the popcounts up (xor shuffles inside the group); one vector atomicAdd per (tile, program).
// A lane reads only cells it wrote itself; the ballots cross lanes and are read behind the barrier.
// No id forms an address before it is checked against count (columns hold cap + 1 >= count + 1 entries; the deleted bitset
// (cap >> 5) + 1 words); a word index is checked against words_per_list before it is stored to.
// Registers: nothing is indexed dynamically in registers (cells and ballots live in LDS; the column table is read from memory through
// the scalar cache, one slot at a time, not held in 48 SGPRs): no scratch, no spill.
__global__ void __launch_bounds__(KDB_FILTER_WAVE)
filter_eval_kernel(const uint64_t *__restrict__ col_addr, const uint32_t *__restrict__ col_kind, const uint32_t *__restrict__ deleted,
                   uint32_t count, const kdb_filter_term *__restrict__ terms, const uint32_t *__restrict__ prog_offsets,
                   const uint32_t *__restrict__ chunk_masks, uint32_t P, unsigned long long *__restrict__ lists, uint64_t words_per_list,
                   uint32_t *__restrict__ card) {
    extern __shared__ uint64_t s_filter[]; // ballots [KDB_FILTER_CHUNK][KDB_FILTER_TILE_WORDS] | cells [nc][wp][64]
    uint64_t *const s_ballot = s_filter;
    uint64_t *const s_cell = s_filter + KDB_FILTER_CHUNK * KDB_FILTER_TILE_WORDS;
    const uint32_t lane = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    const uint32_t chunk = blockIdx.y;
    const uint32_t p0 = kdb_filter_chunk_first(chunk), np = kdb_filter_chunk_programs(chunk, P);
    const uint64_t w0 = kdb_filter_tile_first_word(tile);
    const uint32_t nw = kdb_filter_tile_words(tile, words_per_list);
    const uint32_t mask = chunk_masks[chunk];
    const uint32_t wp = kdb_filter_pass_words((uint32_t)__popc(mask));
    for (uint32_t wb = 0; wb < nw; wb += wp) {
        const uint32_t npass = nw - wb < wp ? nw - wb : wp;
        uint32_t live_bits = 0u;
        for (uint32_t w = 0; w < npass; w++) {
            const uint64_t id64 = (w0 + wb + w) * KDB_FILTER_WAVE + lane;
            bool live = id64 >= 1u && id64 <= (uint64_t)count;
            const uint32_t id = live ? (uint32_t)id64 : 0u;
            if (live) live = ((deleted[id >> 5] >> (id & 31u)) & 1u) == 0u;
            live_bits |= (uint32_t)live << w;
            uint32_t slot = 0;
#pragma unroll 1
            for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++) {
                if (!((mask >> c) & 1u)) continue; // (wave-uniform)
                const bool f64 = col_kind[c] == KDB_COL_F64;
                const uint64_t base = col_addr[c]; // (a global address: hipMalloc'ed by kdb_index_set_column)
                uint64_t cell = f64 ? 0x7ff8000000000000ull : 0ull; // absent
                if (live) cell = f64 ? reinterpret_cast<const KDB_GLOBAL_AS uint64_t *>(base)[id] : (uint64_t) reinterpret_cast<const KDB_GLOBAL_AS uint32_t *>(base)[id];
                s_cell[(slot * wp + w) * KDB_FILTER_WAVE + lane] = cell;
                slot++;
            }
        }
        for (uint32_t j = 0; j < np; j++) {
            const uint32_t a = prog_offsets[p0 + j], b = prog_offsets[p0 + j + 1];
            const uint32_t hits = live_bits & kdb_filter_run_words(terms + a, b - a, npass, [&](uint32_t col, uint32_t w) {
                                      return s_cell[(kdb_filter_dense_slot(mask, col) * wp + w) * KDB_FILTER_WAVE + lane];
                                  });
            unsigned long long mine = 0ull;
            for (uint32_t w = 0; w < npass; w++) {
                const unsigned long long word = __ballot((hits >> w) & 1u);
                if (lane == w) mine = word;
            }
            if (lane < npass) s_ballot[j * KDB_FILTER_TILE_WORDS + wb + lane] = mine;
        }
    }
    __syncthreads(); // (one wave: the ballots become visible to the lanes that store them)
    constexpr uint32_t GROUPS = KDB_FILTER_WAVE / KDB_FILTER_TILE_WORDS; // programs written per round
    const uint32_t g = lane / KDB_FILTER_TILE_WORDS, wl = lane % KDB_FILTER_TILE_WORDS;
    for (uint32_t j0 = 0; j0 < np; j0 += GROUPS) {
        const uint32_t j = j0 + g;
        const bool mine = j < np && wl < nw;
        unsigned long long word = 0ull;
        if (mine) {
            word = s_ballot[j * KDB_FILTER_TILE_WORDS + wl];
            lists[kdb_filter_list_word(p0 + j, words_per_list) + w0 + wl] = word;
        }
        uint32_t n = (uint32_t)__popcll(word);
#pragma unroll
        for (int o = (int)KDB_FILTER_TILE_WORDS / 2; o >= 1; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, 64);
        if (card && wl == 0 && j < np && n) atomicAdd(card + p0 + j, n);
    }
}

} // namespace

int kdb_launch_col_fill(void *d_col, uint32_t kind, size_t first, size_t n, hipStream_t s) {
    if (n == 0) return KDB_OK;
    hipLaunchKernelGGL(col_fill_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, d_col, kind, first, n);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}

int kdb_launch_filter_eval(kdb_index *idx, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P, uint64_t *d_lists,
                           uint64_t words_per_list, uint32_t *d_card, hipStream_t s) {
    const uint32_t n_chunks = kdb_filter_chunks(P);
    std::vector<uint32_t> masks(n_chunks ? n_chunks : 1u, 0u);
    uint32_t bad = 0;
    const int vrc = kdb_filter_validate(terms, prog_offsets, P, idx->col_kind, masks.data(), &bad); // (before any offset is trusted)
    if (vrc) {
        kdb_set_error("filter_eval: program %u: %s", bad, kdb_filter_strerror(vrc));
        return KDB_ERR_INVALID;
    }
    const uint64_t n_terms = prog_offsets[P];
    const KdbFilterStage L = kdb_filter_stage(n_terms, P);
    // one host image of the staged buffer, one copy (pageable memory: consumed before hipMemcpyAsync returns, like the grouped scan's tables)
    std::vector<unsigned char> img((size_t)L.total, 0);
    memcpy(img.data() + L.o_terms, terms, (size_t)n_terms * sizeof(kdb_filter_term));
    memcpy(img.data() + L.o_offsets, prog_offsets, ((size_t)P + 1u) * 4u);
    memcpy(img.data() + L.o_masks, masks.data(), (size_t)n_chunks * 4u);
    for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++) {
        const uint64_t addr = reinterpret_cast<uintptr_t>(idx->d_col[c]);
        memcpy(img.data() + L.o_cols + (size_t)c * 8u, &addr, 8);
        memcpy(img.data() + L.o_cols + (size_t)KDB_MAX_COLUMNS * 8u + (size_t)c * 4u, &idx->col_kind[c], 4);
    }
    int rc = kdb_ensure_scratch(idx, (size_t)L.total);
    if (rc) return rc;
    unsigned char *d = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch);
    KDB_HIP(hipMemcpyAsync(d, img.data(), (size_t)L.total, hipMemcpyHostToDevice, s));
    if (d_card) KDB_HIP(hipMemsetAsync(d_card, 0, (size_t)P * 4u, s));
    uint32_t lds = 0; // the cells of the chunk that needs most
    for (uint32_t m : masks) lds = std::max(lds, kdb_filter_lds_bytes(kdb_filter_popcount(m)));
    const dim3 grid((unsigned)kdb_filter_tiles(words_per_list), n_chunks);
    hipLaunchKernelGGL(filter_eval_kernel, grid, dim3(KDB_FILTER_WAVE), lds, s, reinterpret_cast<const uint64_t *>(d + L.o_cols),
                       reinterpret_cast<const uint32_t *>(d + L.o_cols + (size_t)KDB_MAX_COLUMNS * 8u), idx->d_deleted, idx->count,
                       reinterpret_cast<const kdb_filter_term *>(d + L.o_terms), reinterpret_cast<const uint32_t *>(d + L.o_offsets),
                       reinterpret_cast<const uint32_t *>(d + L.o_masks), P, reinterpret_cast<unsigned long long *>(d_lists), words_per_list, d_card);
    KDB_HIP(hipGetLastError());
    return KDB_OK;
}

// ---------------------------------------------------------------------------------------------
// kdb_filter_parse -- the grammar of FindIDsByFilter (pkg/core/core.go:1766-1839) / evaluateBooleanFilter (:1900-2034) restated for
// the host; no device is touched.  kektor_hip.h has the contract.
// ---------------------------------------------------------------------------------------------
namespace {

inline bool fp_re_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\f' || c == '\r'; } // RE2's \s
inline bool fp_trim_space(char c) { return fp_re_space(c) || c == '\v'; }                                 // strings.TrimSpace, ASCII
inline char fp_upper(char c) { return c >= 'a' && c <= 'z' ? (char)(c - 32) : c; }

struct FpSpan {
    size_t a, b; // [a, b) of the filter
};
inline FpSpan fp_trim(const char *s, FpSpan x) {
    while (x.a < x.b && fp_trim_space(s[x.a])) x.a++;
    while (x.b > x.a && fp_trim_space(s[x.b - 1])) x.b--;
    return x;
}
// regexp.Split(x, -1) for (?i)\s+WORD\s+: leftmost matches, each as long as it can be, the search resuming behind a match
void fp_split(const char *s, FpSpan x, const char *word, std::vector<FpSpan> &out) {
    const size_t wl = strlen(word);
    size_t piece = x.a, i = x.a;
    while (i < x.b) {
        if (!fp_re_space(s[i])) {
            i++;
            continue;
        }
        size_t j = i;
        while (j < x.b && fp_re_space(s[j])) j++; // \s+ takes the whole run (the word begins with a letter: giving back does not help)
        bool m = j + wl < x.b;
        for (size_t c = 0; m && c < wl; c++) m = fp_upper(s[j + c]) == word[c];
        if (m && fp_re_space(s[j + wl])) {
            size_t e = j + wl;
            while (e < x.b && fp_re_space(s[e])) e++;
            out.push_back({piece, i});
            piece = i = e;
        } else {
            i = j; // no match starts inside this run
        }
    }
    out.push_back({piece, x.b});
}
// strconv.ParseFloat(v, 64) == nil error, through strtod in the C locale behind a syntax check of what the two disagree on
bool fp_number(const char *s, size_t n, double *out) {
    if (n == 0 || n > 4096) return false;
    size_t i = 0;
    if (s[i] == '+' || s[i] == '-') i++;
    if (i >= n) return false;
    const bool hex = i + 1 < n && s[i] == '0' && (s[i + 1] == 'x' || s[i + 1] == 'X');
    bool has_p = false;
    for (size_t j = i; j < n; j++) {
        const char c = s[j];
        if (fp_trim_space(c) || c == '(' || c == '_') return false; // strtod skips leading blanks and reads nan(...); Go does neither
        if (hex && (c == 'p' || c == 'P')) has_p = true;
    }
    if (hex && !has_p) return false; // Go: a hexadecimal mantissa needs its p exponent
    static locale_t c_loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    std::string z(s, n);
    if (strlen(z.c_str()) != n) return false; // (an embedded NUL)
    char *end = nullptr;
    errno = 0;
    const double v = c_loc ? strtod_l(z.c_str(), &end, c_loc) : strtod(z.c_str(), &end);
    if (end != z.c_str() + n) return false;
    if (errno == ERANGE && isinf(v)) return false; // ParseFloat: value out of range is an error
    *out = v;
    return true;
}

} // namespace

extern "C" int kdb_filter_parse(const char *filter, kdb_filter_atom *atoms, uint32_t cap, uint32_t *n_atoms) {
    if (n_atoms) *n_atoms = 0;
    if (!filter || !n_atoms || (cap && !atoms)) {
        kdb_set_error("filter_parse: null argument");
        return KDB_ERR_INVALID;
    }
    const size_t len = strlen(filter);
    if (len > 0x7fffffffu) {
        kdb_set_error("filter_parse: filter too long");
        return KDB_ERR_INVALID;
    }
    const FpSpan all = fp_trim(filter, {0, len});
    if (all.a == all.b) {
        kdb_set_error("filter_parse: empty filter");
        return KDB_ERR_INVALID;
    }
    std::vector<FpSpan> blocks, subs;
    fp_split(filter, all, "OR", blocks);
    uint32_t n = 0;
    for (FpSpan blk : blocks) {
        blk = fp_trim(filter, blk);
        if (blk.a == blk.b) continue;
        subs.clear();
        fp_split(filter, blk, "AND", subs);
        uint32_t in_block = 0;
        for (FpSpan sub : subs) {
            sub = fp_trim(filter, sub);
            if (sub.a == sub.b) continue;
            // findFilterOperator (:1866-1897)
            bool in_single = false, in_double = false;
            size_t op_at = sub.b, op_len = 0;
            uint8_t op = 0;
            for (size_t i = sub.a; i < sub.b; i++) {
                const char c = filter[i];
                if (c == '\'') {
                    if (!in_double) in_single = !in_single;
                    continue;
                }
                if (c == '"') {
                    if (!in_single) in_double = !in_double;
                    continue;
                }
                if (in_single || in_double) continue;
                if (i + 1 < sub.b && filter[i + 1] == '=' && (c == '!' || c == '<' || c == '>')) {
                    op = c == '!' ? KDB_FA_NE : c == '<' ? KDB_FA_LE : KDB_FA_GE;
                    op_at = i, op_len = 2;
                    break;
                }
                if (c == '=' || c == '<' || c == '>') {
                    op = c == '=' ? KDB_FA_EQ : c == '<' ? KDB_FA_LT : KDB_FA_GT;
                    op_at = i, op_len = 1;
                    break;
                }
            }
            if (!op_len) {
                kdb_set_error("filter_parse: error in filter '%.*s': invalid filter format", (int)(sub.b - sub.a > 200 ? 200 : sub.b - sub.a), filter + sub.a);
                return KDB_ERR_INVALID;
            }
            const FpSpan key = fp_trim(filter, {sub.a, op_at});
            FpSpan val = fp_trim(filter, {op_at + op_len, sub.b});
            while (val.a < val.b && (filter[val.a] == '\'' || filter[val.a] == '"')) val.a++; // strings.Trim(v, "'\"")
            while (val.b > val.a && (filter[val.b - 1] == '\'' || filter[val.b - 1] == '"')) val.b--;
            double num = 0.0;
            const bool numeric = fp_number(filter + val.a, val.b - val.a, &num);
            if (numeric && num != num) {
                kdb_set_error("filter_parse: error in filter '%.*s': a NaN operand is not accepted", (int)(sub.b - sub.a > 200 ? 200 : sub.b - sub.a), filter + sub.a);
                return KDB_ERR_INVALID;
            }
            if (!numeric && op >= KDB_FA_LT) {
                kdb_set_error("filter_parse: error in filter '%.*s': value must be numeric for a range operator", (int)(sub.b - sub.a > 200 ? 200 : sub.b - sub.a),
                              filter + sub.a);
                return KDB_ERR_INVALID;
            }
            if (n < cap) {
                kdb_filter_atom a{};
                a.key_off = (uint32_t)key.a, a.key_len = (uint32_t)(key.b - key.a);
                a.val_off = (uint32_t)val.a, a.val_len = (uint32_t)(val.b - val.a);
                a.op = op;
                a.is_numeric = numeric ? 1 : 0;
                a.number = numeric ? num : 0.0;
                atoms[n] = a;
            }
            n++;
            in_block++;
        }
        if (in_block && n - 1 < cap) atoms[n - 1].flags |= KDB_FT_END_BLOCK; // (a block without clauses is skipped, :1828-1833)
    }
    *n_atoms = n;
    return KDB_OK;
}
