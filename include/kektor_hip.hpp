// kektor_hip.hpp -- header-only C++ host mirror of the reference's index interface over the C ABI.
//
// Plays the role of hnsw.Index for the search path (pkg/core/hnsw/hnsw_index.go:42-135): same method
// names, argument meaning and error behaviour as the Go code a shim would keep --
//   SearchWithScores(query, k, allowList, efSearch) -> []SearchResult   (hnsw_index.go:343-366,
//                                                                        core.VectorIndex, vector_index.go:35)
//   Delete(ids), Close(), Metric(), Precision()
// plus the batch entry points the shim's micro-batcher calls, and that micro-batcher itself (MicroBatcher).  Errors of the search path are swallowed
// to an empty result exactly like the reference (":356-359 slog.Error + empty slice"); everything else
// throws kektor::Error carrying kdb_last_error().
#pragma once
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <linux/futex.h> // (the batcher's followers sleep on a futex word: Linux, like the library itself)
#include <sys/syscall.h>
#include <unistd.h>

#include "kektor_hip.h"

namespace kektor {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &what) : std::runtime_error(what + ": " + kdb_last_error()), status(st) {}
};

// types.SearchResult (pkg/core/types/types.go:12-15)
// a query that is not finite gets no results (the library answers it with count 0 as well; checked here so that the caller's log
// line is the reference's, hnsw_index.go:356-359): exponent all ones = NaN or infinity
inline bool AllFinite(const float *x, size_t n) {
    for (size_t i = 0; i < n; i++) {
        uint32_t u;
        std::memcpy(&u, x + i, 4);
        if ((u & 0x7f800000u) == 0x7f800000u) return false;
    }
    return true;
}

struct SearchResult {
    uint32_t DocID;
    double Score;
};

// Dense stand-in for *roaring.Bitmap over internal ids (the shim converts).
struct AllowList {
    std::vector<uint64_t> words; // ((count >> 6) + 1) words; all zero = the non-nil EMPTY list
    explicit AllowList(uint32_t count) : words((count >> 6) + 1, 0) {}
    void Add(uint32_t id) { words[id >> 6] |= 1ull << (id & 63); }
    bool Contains(uint32_t id) const { return (id >> 6) < words.size() && ((words[id >> 6] >> (id & 63)) & 1ull); }
};

// CalculateConsensus (pkg/engine/epistemic_types.go:126-178) with the per-node similarity of Engine.VBeliefState (epistemic.go:81) for n
// vectors that are in host memory already, all of them active: the arithmetic of kdb_consensus_batch restated on the host (kektor_hip.h
// has the definition), bit for bit -- float32 centroid accumulated node after node from 0 and divided once, every dot product and
// squared norm a float64 sum over the columns in ascending order (each norm is summed once instead of once per CosineDistance call:
// the same additions in the same order).  gram (optional): (n + 1) x (n + 1), index n the centroid, as out_gram.
struct ConsensusResult {
    kdb_consensus rec{};
    std::vector<float> centroid;    // dim floats (zeros for n == 0)
    std::vector<double> similarity; // n doubles; empty without a query
    std::vector<double> gram;       // filled when asked for
};
namespace detail {
inline double cosine_distance(double dot, double na, double nb) { // :299-320 from its three sums
    if (na == 0.0 || nb == 0.0) return 1.0;
    double sim = dot / (std::sqrt(na) * std::sqrt(nb));
    if (sim > 1.0) sim = 1.0;   // math.Min(1, sim): a NaN stays
    if (sim <= 0.0) sim = 0.0;  // math.Max(0, sim): -0 becomes +0, a NaN stays
    return 1.0 - sim;
}
// out[j] = sum over the columns, ascending, of a[c] * rows[j][c] for j in [j0, j1): four independent chains at a time
inline void dots(const float *a, const float *rows, size_t dim, size_t j0, size_t j1, double *out) {
    size_t j = j0;
    for (; j + 4 <= j1; j += 4) {
        const float *r0 = rows + j * dim, *r1 = r0 + dim, *r2 = r1 + dim, *r3 = r2 + dim;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (size_t c = 0; c < dim; c++) {
            const double x = (double)a[c];
            s0 += x * (double)r0[c];
            s1 += x * (double)r1[c];
            s2 += x * (double)r2[c];
            s3 += x * (double)r3[c];
        }
        out[j] = s0, out[j + 1] = s1, out[j + 2] = s2, out[j + 3] = s3;
    }
    for (; j < j1; j++) {
        const float *r = rows + j * dim;
        double s0 = 0;
        for (size_t c = 0; c < dim; c++) s0 += (double)a[c] * (double)r[c];
        out[j] = s0;
    }
}
} // namespace detail
inline ConsensusResult consensus_host(const float *rows, uint32_t n, uint32_t dim, const float *query = nullptr, bool wantGram = false) {
    ConsensusResult r;
    r.rec.n_found = r.rec.n_active = n;
    r.centroid.assign(dim, 0.f);
    const size_t N = n, D = dim, W = N + 1;
    std::vector<double> g(W * W, 0.0); // dots of the n rows and (index n) the centroid
    if (n == 1) std::memcpy(r.centroid.data(), rows, D * 4); // "return 1.0, 0.0, nodes[0].Vector"
    else if (n > 1) {
        for (size_t i = 0; i < N; i++)
            for (size_t c = 0; c < D; c++) r.centroid[c] += rows[i * D + c];
        for (size_t c = 0; c < D; c++) r.centroid[c] /= (float)n;
    }
    std::vector<double> tmp(N + 1);
    for (size_t i = 0; i < N; i++) { // row i against rows i .. n - 1
        detail::dots(rows + i * D, rows, D, i, N, tmp.data());
        for (size_t j = i; j < N; j++) g[i * W + j] = g[j * W + i] = tmp[j];
    }
    if (n) {
        detail::dots(r.centroid.data(), rows, D, 0, N, tmp.data());
        for (size_t j = 0; j < N; j++) g[N * W + j] = g[j * W + N] = tmp[j];
        detail::dots(r.centroid.data(), r.centroid.data(), D, 0, 1, &g[N * W + N]);
    }
    if (query) {
        r.similarity.resize(N);
        double qq = 0;
        detail::dots(query, query, D, 0, 1, &qq);
        detail::dots(query, rows, D, 0, N, tmp.data());
        for (size_t i = 0; i < N; i++) r.similarity[i] = 1.0 - detail::cosine_distance(tmp[i], g[i * W + i], qq);
    }
    if (n == 1) r.rec.score = 1.0;
    else if (n > 1) {
        double sum = 0.0;
        for (size_t i = 0; i < N; i++) {
            const double d = detail::cosine_distance(g[i * W + N], g[i * W + i], g[N * W + N]);
            sum += d * d;
        }
        r.rec.variance = sum / (double)n;
        double mv = 0.0;
        for (size_t i = 0; i < N; i++)
            for (size_t j = i + 1; j < N; j++) {
                const double d = detail::cosine_distance(g[i * W + j], g[i * W + i], g[j * W + j]);
                if (d > mv) mv = d;
            }
        r.rec.max_pair = mv;
        if (mv < 1e-10) r.rec.score = 1.0;
        else {
            double q = r.rec.variance / (mv * mv);
            if (q > 1.0) q = 1.0; // math.Min(q, 1): a NaN stays
            r.rec.score = 1.0 - q;
        }
    }
    if (wantGram) r.gram = std::move(g);
    return r;
}

namespace hnsw {

class Index {
  public:
    Index(uint32_t dim, uint32_t metric, uint32_t precision, uint32_t m, uint32_t efConstruction, uint32_t capacity,
          int device = 0)
        : dim_(dim), metric_(metric), precision_(precision) {
        kdb_index_desc d{dim, metric, precision, m, efConstruction, capacity, device, 0};
        int rc = kdb_index_create(&d, &h_);
        if (rc) throw Error(rc, "hnsw.New");
        (void)kdb_index_set_launch_timing(h_, 0); // a serving mirror never reads last_kernel_ms: two queue packets less per call
    }
    ~Index() { Close(); }
    void SetLaunchTiming(bool on) { (void)kdb_index_set_launch_timing(h_, on ? 1 : 0); } // measurement harnesses
    // DB.Compress (core.go:1128-1290) on the device: a new index of `precision` (KDB_PREC_F16 / KDB_PREC_I8) over the same
    // graph (or re-inserted by the GPU builder when rebuildGraph); this index stays as it is
    std::unique_ptr<Index> Compress(uint32_t precision, bool rebuildGraph = false) const {
        kdb_index *h = nullptr;
        check(kdb_index_compress(h_, precision, rebuildGraph ? KDB_COMPRESS_REBUILD_GRAPH : 0u, &h), "compress");
        return std::unique_ptr<Index>(new Index(h, dim_, metric_, precision));
    }
    Index(const Index &) = delete;
    Index &operator=(const Index &) = delete;

    void Close() { // hnsw_index.go:3533-3586
        if (h_) kdb_index_destroy(h_);
        h_ = nullptr;
    }
    uint32_t Metric() const { return metric_; }
    uint32_t Precision() const { return precision_; }
    void SetNeedsRefine(bool v) { needsRefine_ = v; } // hnsw_index.go:3590
    void SetHeapOrder(bool v) { heapOrder_ = v; }     // (on by default: the reference's answer when distances tie)
    void Reserve(uint32_t capacity) { check(kdb_index_reserve(h_, capacity), "reserve"); } // growNodes, hnsw_index.go:2732-2768

    // rows in stored form (see kdb_index_upload_rows); graph as exported by SnapshotData
    void UploadRows(uint32_t firstID, uint32_t n, const void *rows) { check(kdb_index_upload_rows(h_, firstID, n, rows), "upload_rows"); }
    void UploadArena(const std::string &dir, uint32_t count, const uint32_t *slotTable = nullptr) {
        check(kdb_index_upload_arena(h_, dir.c_str(), slotTable, count), "upload_arena");
    }
    void UploadGraph(const kdb_graph_view &g) { check(kdb_index_upload_graph(h_, &g), "upload_graph"); }
    void Build(uint32_t count, uint64_t seed = 1, uint32_t batch = 0) { // addBatchInternal on the GPU
        kdb_build_params p{batch, 0, seed, 0, 0};
        check(kdb_index_build(h_, count, &p), "build");
    }
    // Add (hnsw_index.go:472-809) on the device for rows already uploaded at firstID ..: n nodes one after another, each linked against
    // the graph the nodes before it left; levels[i] as drawn by the caller (capped at maxLevel+1 as randomLevel does)
    kdb_add_stats Add(uint32_t firstID, const uint8_t *levels, uint32_t n, uint32_t efConstruction = 0) {
        kdb_add_params p{efConstruction, 0};
        kdb_add_stats st{};
        check(kdb_index_add(h_, firstID, n, levels, &p, &st), "add");
        return st;
    }
    // GraphOptimizer.Refine (optimizer.go:288-464) on the device: the lists of `ids` (empty: every live node) against the graph as it is
    kdb_refine_stats Refine(const std::vector<uint32_t> &ids = {}, uint32_t efConstruction = 0, uint32_t chunkNodes = 0) {
        kdb_refine_params p{efConstruction, 0, chunkNodes};
        kdb_refine_stats st{};
        check(kdb_index_refine(h_, ids.empty() ? nullptr : ids.data(), (uint32_t)ids.size(), &p, &st), "refine");
        return st;
    }
    kdb_refine_stats RunTurboRefine() { // optimizer.go:679-719: the whole graph, then SetNeedsRefine(false) (:716)
        kdb_refine_stats st = Refine();
        needsRefine_ = false;
        return st;
    }
    // GraphOptimizer.Vacuum (optimizer.go:133-277) on the device: nodes with links to deleted nodes re-linked as Refine does it, a
    // deleted entry point replaced (electTopLevel: by the live node of the highest level, not the lowest live id), deleted nodes cleared
    kdb_vacuum_stats Vacuum(uint32_t efConstruction = 0, bool electTopLevel = false, uint32_t chunkNodes = 0) {
        kdb_vacuum_params p{efConstruction, electTopLevel ? (uint32_t)KDB_VACUUM_ELECT_TOP_LEVEL : 0u, chunkNodes};
        kdb_vacuum_stats st{};
        check(kdb_index_vacuum(h_, &p, &st), "vacuum");
        return st;
    }
    // the census Vacuum makes (optimizer.go:165-193), read-only: the live nodes that hold a dead link, ascending
    struct DeadLinks {
        std::vector<uint32_t> ids;
        uint64_t deadLinks = 0, deadNodes = 0;
    };
    DeadLinks DeadLinkScan() {
        DeadLinks r;
        uint32_t n = 0;
        check(kdb_index_dead_link_scan(h_, nullptr, 0, &n, &r.deadLinks, &r.deadNodes), "dead_link_scan");
        r.ids.resize(n);
        if (n) check(kdb_index_dead_link_scan(h_, r.ids.data(), n, &n, &r.deadLinks, &r.deadNodes), "dead_link_scan");
        return r;
    }
    bool MaintenanceRun(const std::string &task) { // hnsw_index.go:976: "vacuum" | "refine"
        if (task == "vacuum") return Vacuum().dead_nodes > 0;
        if (task == "refine") return Refine().nodes_refined > 0;
        throw std::invalid_argument("unknown maintenance task " + task);
    }
    // incremental refresh of the mirror after writers touched a few nodes (see kdb_index_append_nodes)
    void AppendNodes(uint32_t firstID, const std::vector<uint8_t> &levels) {
        check(kdb_index_append_nodes(h_, firstID, (uint32_t)levels.size(), levels.data()), "append_nodes");
    }
    void PatchAdjacency(uint32_t level, const std::vector<uint32_t> &ids, const std::vector<std::vector<uint32_t>> &lists) {
        std::vector<uint64_t> off(ids.size() + 1, 0);
        std::vector<uint32_t> nb;
        for (size_t i = 0; i < ids.size(); i++) {
            nb.insert(nb.end(), lists[i].begin(), lists[i].end());
            off[i + 1] = nb.size();
        }
        if (nb.empty()) nb.push_back(0);
        check(kdb_index_patch_adjacency(h_, level, (uint32_t)ids.size(), ids.data(), off.data(), nb.data()), "patch_adjacency");
    }
    void SetEntry(uint32_t entry, int32_t maxLevel) { check(kdb_index_set_entry(h_, entry, maxLevel), "set_entry"); }
    void Delete(const std::vector<uint32_t> &ids) { check(kdb_index_mark_deleted(h_, ids.data(), (uint32_t)ids.size()), "delete"); }

    // core.VectorIndex.SearchWithScores: one query; empty slice on any error, closed index or empty allow list
    std::vector<SearchResult> SearchWithScores(const std::vector<float> &query, int k, const AllowList *allowList,
                                               int efSearch) const {
        std::vector<SearchResult> out;
        if (!h_ || k <= 0 || query.size() != dim_) return out;
        if (!AllFinite(query.data(), query.size())) return out; // (the library would answer it with count 0 too: kdb_load_query)
        std::vector<uint32_t> ids((size_t)k), cnt(1);
        DistBuf dist((size_t)k, wide());
        int rc = kdb_search_batch(h_, query.data(), 1, (uint32_t)k, (uint32_t)(efSearch > 0 ? efSearch : 0),
                                  allowList ? allowList->words.data() : nullptr, flags(), ids.data(), dist.ptr(), cnt.data());
        if (rc) return out; // ":356-359": log and return []
        for (uint32_t i = 0; i < cnt[0]; i++) out.push_back({ids[i], score(dist, i)});
        return out;
    }
    // the micro-batcher's call: B queries, row-major; results[b] has <= k entries
    std::vector<std::vector<SearchResult>> SearchBatch(const float *queries, uint32_t B, int k, const AllowList *allowList,
                                                       int efSearch) const {
        std::vector<std::vector<SearchResult>> out(B);
        if (!h_ || k <= 0 || B == 0) return out;
        std::vector<uint32_t> ids((size_t)B * k), cnt(B);
        DistBuf dist((size_t)B * k, wide());
        int rc = kdb_search_batch(h_, queries, B, (uint32_t)k, (uint32_t)(efSearch > 0 ? efSearch : 0),
                                  allowList ? allowList->words.data() : nullptr, flags(), ids.data(), dist.ptr(), cnt.data());
        if (rc) return out;
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t i = 0; i < cnt[b]; i++) out[b].push_back({ids[(size_t)b * k + i], score(dist, (size_t)b * k + i)});
        return out;
    }
    // B requests that differ in k and efSearch, ONE launch (kdb_search_batch_mixed): results[b] is what SearchWithScores(query b, ks[b],
    // allowList, efs[b]) returns; a k <= 0 anywhere, or any error, gives empty lists, like SearchBatch
    std::vector<std::vector<SearchResult>> SearchMixed(const float *queries, uint32_t B, const std::vector<int> &ks, const std::vector<int> &efs,
                                                       const AllowList *allowList) const {
        std::vector<std::vector<SearchResult>> out(B);
        if (!h_ || B == 0 || ks.size() != B || efs.size() != B) return out;
        std::vector<uint32_t> k(B), ef(B);
        uint32_t stride = 0;
        for (uint32_t b = 0; b < B; b++) {
            if (ks[b] <= 0) return out;
            k[b] = (uint32_t)ks[b];
            ef[b] = (uint32_t)(efs[b] > 0 ? efs[b] : 0);
            if (k[b] > stride) stride = k[b];
        }
        std::vector<uint32_t> ids((size_t)B * stride), cnt(B);
        DistBuf dist((size_t)B * stride, wide());
        int rc = kdb_search_batch_mixed(h_, queries, B, k.data(), ef.data(), stride, allowList ? allowList->words.data() : nullptr, flags(), ids.data(),
                                        dist.ptr(), cnt.data());
        if (rc) return out;
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t i = 0; i < cnt[b]; i++) out[b].push_back({ids[(size_t)b * stride + i], score(dist, (size_t)b * stride + i)});
        return out;
    }
    // exact scan over live (and allowed) rows: BruteForceIndex.SearchWithScores semantics (vector_index.go:104-140)
    std::vector<std::vector<SearchResult>> FlatScanBatch(const float *queries, uint32_t B, int k, const AllowList *allowList) const {
        std::vector<std::vector<SearchResult>> out(B);
        if (!h_ || k <= 0 || B == 0) return out;
        std::vector<uint32_t> ids((size_t)B * k), cnt(B);
        DistBuf dist((size_t)B * k, wide());
        check(kdb_flat_scan_batch(h_, queries, B, (uint32_t)k, allowList ? allowList->words.data() : nullptr, flags(), ids.data(),
                                  dist.ptr(), cnt.data()), "flat_scan");
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t i = 0; i < cnt[b]; i++) out[b].push_back({ids[(size_t)b * k + i], score(dist, (size_t)b * k + i)});
        return out;
    }
    // GetNodeData(id).Vector (hnsw_index.go:2909-2959) for every id, as Engine.VGetMany reads them: ids.size() x Dim() floats, row-major
    // (float16 widened, int8 dequantised); found (optional): one byte per id, 0 = no such live node (its row is zeros)
    std::vector<float> GetVectors(const std::vector<uint32_t> &ids, std::vector<uint8_t> *found = nullptr) const {
        std::vector<float> out(ids.size() * (size_t)dim_);
        if (found) found->assign(ids.size(), 0);
        if (!h_ || ids.empty()) return out;
        check(kdb_index_decode_rows(h_, ids.data(), (uint32_t)ids.size(), out.data(), found ? found->data() : nullptr), "decode_rows");
        return out;
    }
    // One page of the Gardener's loop (pkg/cognitive/gardener.go:803-869: VGetMany, then VSearchWithScores with every vData.Vector) as one
    // call: results[i] is what SearchWithScores(GetVectors({ids[i]}), k, allowList, efSearch) returns -- the rows never leave the device.
    // An id that is not found gets an empty list; dropSelf: without the id itself.  Empty lists on any error, like SearchWithScores.
    std::vector<std::vector<SearchResult>> SearchSimilar(const std::vector<uint32_t> &ids, int k, int efSearch, const AllowList *allowList = nullptr,
                                                         bool dropSelf = false) const {
        const uint32_t B = (uint32_t)ids.size();
        std::vector<std::vector<SearchResult>> out(B);
        if (!h_ || k <= 0 || B == 0) return out;
        std::vector<uint32_t> rid((size_t)B * k), cnt(B);
        DistBuf dist((size_t)B * k, wide());
        int rc = kdb_search_by_id(h_, ids.data(), B, (uint32_t)k, (uint32_t)(efSearch > 0 ? efSearch : 0), allowList ? allowList->words.data() : nullptr,
                                  flags() | (dropSelf ? (uint32_t)KDB_BY_ID_DROP_SELF : 0u), rid.data(), dist.ptr(), cnt.data());
        if (rc) return out; // ":356-359": log and return []
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t i = 0; i < cnt[b]; i++) out[b].push_back({rid[(size_t)b * k + i], score(dist, (size_t)b * k + i)});
        return out;
    }
    // CalculateConsensus (pkg/engine/epistemic_types.go:126-178) over the stored vectors of B id lists of `stride` entries each, on the
    // device (kdb_consensus_batch): counts / queries / activeList may be null; similarity (optional) receives B x stride doubles
    std::vector<kdb_consensus> Consensus(const uint32_t *ids, uint32_t B, uint32_t stride, const uint32_t *counts = nullptr, const float *queries = nullptr,
                                         const AllowList *activeList = nullptr, std::vector<double> *similarity = nullptr,
                                         std::vector<float> *centroid = nullptr) const {
        std::vector<kdb_consensus> out(B);
        if (similarity) similarity->assign(queries ? (size_t)B * stride : 0, -1.0);
        if (centroid) centroid->assign((size_t)B * dim_, 0.f);
        if (!h_ || B == 0) return out;
        check(kdb_consensus_batch(h_, ids, counts, B, stride, queries, activeList ? activeList->words.data() : nullptr, 0, out.data(),
                                  similarity && queries ? similarity->data() : nullptr, centroid ? centroid->data() : nullptr, nullptr), "consensus");
        return out;
    }
    // The vector half of Engine.VBeliefState (pkg/engine/epistemic.go:22-182) as one call (kdb_belief_batch): the search (k capped at
    // 50 as :31 does, efSearch 100 as :45) and CalculateConsensus over its active results; activeList: the ids that are NOT historical.
    // ok is false where the reference returns an error: no candidates, or no active node.
    struct Belief {
        bool ok = false;
        kdb_consensus consensus{};
        std::vector<SearchResult> nodes;
        std::vector<double> similarities;
    };
    Belief BeliefState(const std::vector<float> &query, int k, const AllowList *allowList = nullptr, const AllowList *activeList = nullptr,
                       int efSearch = 100) const {
        Belief r;
        if (k <= 0) k = 10;
        if (k > 50) k = 50;
        if (!h_ || query.size() != dim_) return r;
        std::vector<uint32_t> ids((size_t)k), cnt(1);
        std::vector<double> sim((size_t)k);
        DistBuf dist((size_t)k, wide());
        int rc = kdb_belief_batch(h_, query.data(), 1, (uint32_t)k, (uint32_t)(efSearch > 0 ? efSearch : 0), allowList ? allowList->words.data() : nullptr,
                                  activeList ? activeList->words.data() : nullptr, flags(), ids.data(), dist.ptr(), cnt.data(), &r.consensus, sim.data());
        if (rc) return r;
        for (uint32_t i = 0; i < (cnt[0] & KDB_COUNT_MASK); i++)
            if (sim[i] != -1.0) {
                r.nodes.push_back({ids[i], score(dist, i)});
                r.similarities.push_back(sim[i]);
            }
        r.ok = r.consensus.n_active > 0;
        return r;
    }
    // ---- metadata filters on the device (kektor_hip.h, "metadata filters"; the reference: DB.FindIDsByFilter, core.go:1766-1839) ----
    // One key of the mirror's schema: its numeric column (the reference's B-tree) and / or its code column with the dictionary of
    // the strings seen so far (its inverted index; bools are "true" / "false"); -1 = the key has no such column
    struct FilterKey {
        int f64Slot = -1, codeSlot = -1;
        std::map<std::string, uint32_t> dict; // string value -> code >= 1
    };
    using FilterSchema = std::map<std::string, FilterKey>;
    using FilterProgram = std::vector<kdb_filter_term>;
    // values[i] belongs to id firstID + i: doubles (NaN = no value) for KDB_COL_F64, uint32 codes (0 = no value) for KDB_COL_CODE
    void SetColumn(uint32_t slot, uint32_t kind, uint32_t firstID, uint32_t n, const void *values) {
        check(kdb_index_set_column(h_, slot, kind, firstID, n, values), "set_column");
    }
    void DropColumn(uint32_t slot) { check(kdb_index_drop_column(h_, slot), "drop_column"); }
    // A filter string -> one predicate program.  `k = v`: F64_EQ if v is numeric and k has a numeric column, CODE_EQ if k has a code
    // column and the dictionary knows v (the lenient union, core.go:1933-1944), NEVER if neither; `k != v`: the same clause with NOT;
    // a range operator: one F64 term, NEVER without a numeric column.  Throws kektor::Error where the reference returns an error.
    static FilterProgram CompileFilter(const std::string &filter, const FilterSchema &schema) {
        uint32_t n = 0;
        check(kdb_filter_parse(filter.c_str(), nullptr, 0, &n), "filter_parse");
        std::vector<kdb_filter_atom> atoms(n ? n : 1);
        check(kdb_filter_parse(filter.c_str(), atoms.data(), n, &n), "filter_parse");
        FilterProgram prog;
        auto term = [](uint8_t op, uint16_t col, uint32_t code, double value) {
            kdb_filter_term t;
            std::memset(&t, 0, sizeof t);
            t.op = op, t.col = col, t.code = code, t.value = value;
            return t;
        };
        for (uint32_t i = 0; i < n; i++) {
            const kdb_filter_atom &a = atoms[i];
            const auto it = schema.find(filter.substr(a.key_off, a.key_len));
            const FilterKey *key = it == schema.end() ? nullptr : &it->second;
            const size_t first = prog.size();
            if (a.op == KDB_FA_EQ || a.op == KDB_FA_NE) {
                if (key && a.is_numeric && key->f64Slot >= 0) prog.push_back(term(KDB_FOP_F64_EQ, (uint16_t)key->f64Slot, 0, a.number));
                if (key && key->codeSlot >= 0) {
                    const auto d = key->dict.find(filter.substr(a.val_off, a.val_len));
                    if (d != key->dict.end() && d->second) prog.push_back(term(KDB_FOP_CODE_EQ, (uint16_t)key->codeSlot, d->second, 0.0));
                }
            } else if (key && key->f64Slot >= 0) {
                const uint8_t op = a.op == KDB_FA_LT ? KDB_FOP_F64_LT : a.op == KDB_FA_LE ? KDB_FOP_F64_LE : a.op == KDB_FA_GT ? KDB_FOP_F64_GT : KDB_FOP_F64_GE;
                prog.push_back(term(op, (uint16_t)key->f64Slot, 0, a.number));
            }
            if (prog.size() == first) prog.push_back(term(KDB_FOP_NEVER, 0, 0, 0.0));
            for (size_t j = first; j + 1 < prog.size(); j++) prog[j].flags |= KDB_FT_OR_NEXT;
            if (a.op == KDB_FA_NE) prog[first].flags |= KDB_FT_NOT;
            if (a.flags & KDB_FT_END_BLOCK) prog.back().flags |= KDB_FT_END_BLOCK;
        }
        if (prog.empty()) { // every block was empty: the reference's empty bitmap
            prog.push_back(term(KDB_FOP_NEVER, 0, 0, 0.0));
            prog.back().flags = KDB_FT_END_BLOCK;
        }
        if (prog.size() > KDB_FILTER_MAX_TERMS) throw std::invalid_argument("CompileFilter: more than KDB_FILTER_MAX_TERMS terms");
        return prog;
    }
    // FindIDsByFilter for several programs in one pass over the columns: lists[p] as an AllowList, cards[p] its cardinality
    std::vector<AllowList> EvalFilters(const std::vector<FilterProgram> &programs, std::vector<uint32_t> *cards = nullptr) const {
        std::vector<kdb_filter_term> terms;
        std::vector<uint32_t> off;
        pack(programs, terms, off);
        const uint32_t P = (uint32_t)programs.size(), count = Count();
        const uint64_t words = ((uint64_t)count >> 6) + 1;
        std::vector<uint64_t> flat((size_t)P * words);
        std::vector<uint32_t> card(P);
        check(kdb_filter_eval(h_, terms.data(), off.data(), P, flat.data(), words, card.data()), "filter_eval");
        std::vector<AllowList> out;
        for (uint32_t p = 0; p < P; p++) {
            out.emplace_back(count);
            std::memcpy(out.back().words.data(), flat.data() + (size_t)p * words, (size_t)words * 8);
        }
        if (cards) *cards = card;
        return out;
    }
    // Engine.VSearch with a filter per request, as ONE call (kdb_search_filtered): query b uses programs[progOfQuery[b]]
    // (KDB_NO_FILTER: none).  results[b] is what SearchWithScores (the walk) or FlatScanBatch (a program that allows less than
    // flatSelectivity of the ids, k <= 1024) returns for it; a program that matches nothing gives [].  Empty lists on any error.
    std::vector<std::vector<SearchResult>> SearchFiltered(const float *queries, uint32_t B, int k, int efSearch, const std::vector<FilterProgram> &programs,
                                                          const std::vector<uint32_t> &progOfQuery, double flatSelectivity = 0.1,
                                                          std::vector<uint8_t> *routes = nullptr, std::vector<uint32_t> *cards = nullptr) const {
        std::vector<std::vector<SearchResult>> out(B);
        if (!h_ || k <= 0 || B == 0 || progOfQuery.size() != B || programs.empty()) return out;
        std::vector<kdb_filter_term> terms;
        std::vector<uint32_t> off;
        pack(programs, terms, off);
        std::vector<uint32_t> ids((size_t)B * k), cnt(B), card(programs.size());
        std::vector<float> dist((size_t)B * k);
        std::vector<uint8_t> route(B);
        int rc = kdb_search_filtered(h_, queries, B, (uint32_t)k, (uint32_t)(efSearch > 0 ? efSearch : 0), terms.data(), off.data(), (uint32_t)programs.size(),
                                     progOfQuery.data(), flatSelectivity, flags() & ~(uint32_t)KDB_SEARCH_DIST_F64, ids.data(), dist.data(), cnt.data(),
                                     route.data(), card.data());
        if (rc) return out;
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t i = 0; i < (cnt[b] & KDB_COUNT_MASK); i++) {
                const float d = dist[(size_t)b * k + i]; // (int8: the float64 distance rounded to float on the way out)
                out[b].push_back({ids[(size_t)b * k + i], (metric_ == KDB_METRIC_COSINE && precision_ == KDB_PREC_F32) ? 1.0 - (double)d : (double)d});
            }
        if (routes) *routes = route;
        if (cards) *cards = card;
        return out;
    }
    kdb_index *handle() const { return h_; }
    // concurrent kdb_search_batch calls of a few queries share launches inside the library (kektor_hip.h, "Conventions"): a
    // batcher in front of this index passes unfiltered one-query calls through
    bool CombinesConcurrentCalls() const { return true; }
    uint32_t Dim() const { return dim_; }
    uint32_t Count() const { // nodeCounter of the mirror
        uint32_t count = 0, entry = 0;
        int32_t maxLevel = -1;
        if (!h_ || kdb_index_graph_info(h_, &count, &entry, &maxLevel)) return 0;
        return count;
    }

  private:
    Index(kdb_index *h, uint32_t dim, uint32_t metric, uint32_t precision) : h_(h), dim_(dim), metric_(metric), precision_(precision) {
        (void)kdb_index_set_launch_timing(h_, 0);
    }
    // distances of one call: floats, or -- int8 indexes -- the float64 values the reference computes (hnsw_index.go:2429-2454),
    // asked for with KDB_SEARCH_DIST_F64
    struct DistBuf {
        std::vector<float> f;
        std::vector<double> d;
        DistBuf(size_t n, bool wide) : f(wide ? 0 : n), d(wide ? n : 0) {}
        float *ptr() { return d.empty() ? f.data() : reinterpret_cast<float *>(d.data()); }
    };
    bool wide() const { return precision_ == KDB_PREC_I8; }
    // the reference's f64 epilogue: float64(sum) (distance_go.go:67) / 1.0 - float64(dot) (:127)
    double score(const DistBuf &b, size_t i) const {
        if (!b.d.empty()) return b.d[i];
        return (metric_ == KDB_METRIC_COSINE && precision_ == KDB_PREC_F32) ? 1.0 - (double)b.f[i] : (double)b.f[i];
    }
    // KDB_SEARCH_HEAP_ORDER: queries whose walk meets equal distances (duplicate vectors) are walked again with the reference's two
    // heaps -- ids and their order are hnsw.Index's own, ties included; costs nothing while distances are distinct
    uint32_t flags() const {
        return (needsRefine_ ? (uint32_t)KDB_SEARCH_NEEDS_REFINE : 0u) | (wide() ? (uint32_t)KDB_SEARCH_DIST_F64 : 0u) |
               (heapOrder_ ? (uint32_t)KDB_SEARCH_HEAP_ORDER : 0u);
    }
    static void check(int rc, const char *what) {
        if (rc) throw Error(rc, what);
    }
    static void pack(const std::vector<FilterProgram> &programs, std::vector<kdb_filter_term> &terms, std::vector<uint32_t> &off) {
        off.assign(1, 0u);
        for (const FilterProgram &p : programs) {
            terms.insert(terms.end(), p.begin(), p.end());
            off.push_back((uint32_t)terms.size());
        }
        if (terms.empty()) terms.resize(1); // (a pointer the library refuses by its own rules, not a null one)
    }
    kdb_index *h_ = nullptr;
    uint32_t dim_, metric_, precision_;
    bool needsRefine_ = false;
    bool heapOrder_ = true;
};

// MicroBatcher -- turns concurrent one-query callers into GPU batches (the compiled counterpart of
// the Go shim's hipBatcher, integration/go/hnsw_hip.go).  SearchWithScores keeps the contract of
// hnsw.Index.SearchWithScores (hnsw_index.go:343-366): it blocks until the caller's answer is ready and returns an
// empty slice on any error, on a stopped batcher and for a non-nil empty allow list.
//   * callers that share (k, efSearch, allow-list object) share a group; the first caller of a group is its leader.  Over an index
//     that offers SearchMixed (kektor::hnsw::Index does: kdb_search_batch_mixed walks requests of different k and efSearch in one
//     launch) the callers of one allow list share a group WHATEVER their k and efSearch -- unless the list is so selective that the
//     group takes the exact scan (below), which has one k per call: those keep the full key;
//   * PIPELINED: up to `maxInFlight` (2) groups are on the device at once (the library serves concurrent calls from separate
//     slots: include/kektor_hip.h, "Conventions").  A leader that finds a turn free goes AT ONCE -- a lone caller never sleeps;
//     while every turn is taken its group stays open and grows for free, so batch size follows the load: everything that
//     arrived during the calls in flight leaves with the next one.  `window` > 0 additionally makes a leader that finds the
//     device idle wait that long for company (off by default);
//   * followers sleep on their group's futex word and are woken by one FUTEX_WAKE -- no condition variable, no mutex to
//     queue on when sixty answers arrive at once; no service thread, no timer thread;
//   * an index that combines concurrent calls itself (IndexT::CombinesConcurrentCalls(): kektor::hnsw::Index does -- the library
//     gathers one-query calls that find its slots busy into one launch and lets every caller leave when ITS walk is done, which
//     a batch call cannot) gets unfiltered queries handed through one by one; the batcher then only groups what the library does
//     not: queries that share an allow list (one upload of the list per group), and the routing below;
//   * a filter that allows less than `flatScanSelectivity` of the ids takes the exact scan: the reference's filtered
//     walk prunes non-allowed neighbours while traversing (hnsw_index.go:2545-2549) and falls apart there (the crossover is
//     measured: bench.py's filter_routing leg).
template <class IndexT>
class BasicMicroBatcher {
  public:
    struct Options {
        uint32_t maxBatch = 8192;                     // queries per GPU call
        std::chrono::microseconds window{0};          // > 0: a leader that finds the device idle waits this long for company
        // Measured (bench.py filter_routing legs, profiles/r05_*): on 1M x 768 and on 10M x 1536 the filtered walk at efSearch 100 / 400
        // returns ONE OR TWO answers instead of k at 1 %, 2 % and 5 % selectivity (a node keeps 32 x s allowed neighbours: the walk
        // starves) and k answers from 10 % on.  Below this bound the mirror answers with the exact scan -- deliberately the exact
        // filtered top-k where the reference returns what its starved walk found; from it on, the walk's answer is the reference's.
        double flatScanSelectivity = 0.1;
        uint32_t maxInFlight = 2;                     // GPU calls of this batcher on the device at once
    };
    struct Stats {
        uint64_t calls = 0, batches = 0, flatBatches = 0, largest = 0;
        uint64_t passedThrough = 0; // unfiltered calls handed to an index that combines concurrent calls itself
        uint64_t mixedBatches = 0;  // batches that went out through SearchMixed (callers of one allow list, any k and efSearch)
    };
    static constexpr int kMaxFlatK = 1024; // kdb_flat_scan_batch: k <= 1024
    explicit BasicMicroBatcher(IndexT &idx) : idx_(idx) {}
    BasicMicroBatcher(IndexT &idx, const Options &o) : idx_(idx), opt_(o) {
        if (opt_.maxInFlight == 0) opt_.maxInFlight = 1;
    }
    ~BasicMicroBatcher() { Stop(); }
    BasicMicroBatcher(const BasicMicroBatcher &) = delete;
    BasicMicroBatcher &operator=(const BasicMicroBatcher &) = delete;

    // pending callers and every later call get []
    void Stop() {
        std::lock_guard<std::mutex> lk(mu_);
        closed_ = true;
        turn_cv_.notify_all();
    }
    Stats stats() const {
        std::lock_guard<std::mutex> lk(mu_);
        return stats_;
    }

    std::vector<SearchResult> SearchWithScores(const std::vector<float> &query, int k, const AllowList *allowList, int efSearch) {
        if (k <= 0 || query.size() != idx_.Dim()) return {};
        if (!AllFinite(query.data(), query.size())) return {}; // (never into a batch with other callers' queries)
        if (!allowList && combines(idx_, 0)) {
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (closed_) return {};
                stats_.calls++;
                stats_.passedThrough++;
            }
            auto out = idx_.SearchBatch(query.data(), 1, k, nullptr, efSearch);
            return out.empty() ? std::vector<SearchResult>() : std::move(out[0]);
        }
        // one group per allow list whatever k and efSearch are, where the index can walk such a group in one launch and the list does
        // not send it to the exact scan (counted outside the lock: the list belongs to the caller)
        const bool mix = allowList && mixes(idx_, 0) && !takes_flat_scan(k, allowList);
        std::unique_lock<std::mutex> lk(mu_);
        if (closed_) return {};
        stats_.calls++;
        const Key key = mix ? Key{-1, -1, allowList} : Key{k, efSearch, allowList};
        std::shared_ptr<Group> g;
        auto it = groups_.find(key);
        const bool leader = it == groups_.end();
        if (leader) {
            g = std::make_shared<Group>();
            groups_[key] = g;
        } else {
            g = it->second;
        }
        const size_t me = g->queries.size();
        g->queries.push_back(query.data());
        g->ks.push_back(k);
        g->efs.push_back(efSearch);
        if (g->queries.size() >= opt_.maxBatch) { // full: later callers start the next group
            groups_.erase(key);
            g->sealed = true;
            if (!leader) turn_cv_.notify_all(); // (a leader waiting out its window)
        }
        if (!leader) {
            lk.unlock();
            g->wait_done();
            return std::move(g->results[me]); // (results has one entry per member, always)
        }
        // (wait_until on the system clock = pthread_cond_timedwait, which thread sanitizers intercept; wait_for would use
        // pthread_cond_clockwait, invisible to GCC 11's TSan)
        if (opt_.window.count() > 0 && inflight_ == 0)
            turn_cv_.wait_until(lk, std::chrono::system_clock::now() + opt_.window, [&] { return g->sealed || closed_; });
        // a turn on the device; while all are taken this group stays open and keeps growing
        turn_cv_.wait(lk, [&] { return inflight_ < opt_.maxInFlight || closed_; });
        if (!g->sealed) {
            auto cur = groups_.find(key);
            if (cur != groups_.end() && cur->second == g) groups_.erase(cur);
            g->sealed = true;
        }
        const bool stopped = closed_;
        if (!stopped) inflight_++;
        const uint32_t B = (uint32_t)g->queries.size(); // nobody can join a sealed group
        lk.unlock();
        std::vector<std::vector<SearchResult>> out;
        bool flat = false;
        if (!stopped) {
            const uint32_t dim = idx_.Dim();
            std::vector<float> Q((size_t)B * dim);
            for (uint32_t b = 0; b < B; b++) std::memcpy(Q.data() + (size_t)b * dim, g->queries[b], (size_t)dim * 4);
            if (allowList && !mix) flat = takes_flat_scan(k, allowList);
            try {
                out = flat  ? idx_.FlatScanBatch(Q.data(), B, k, allowList)
                      : mix ? search_mixed(idx_, 0, Q.data(), B, g->ks, g->efs, allowList)
                            : idx_.SearchBatch(Q.data(), B, k, allowList, efSearch);
            } catch (const std::exception &) {
                out.clear();
                if (flat) { // the scan refused (an argument it does not take): the walk is the reference's own path
                    flat = false;
                    try {
                        out = idx_.SearchBatch(Q.data(), B, k, allowList, efSearch);
                    } catch (const std::exception &) { // ":356-359": log and return []
                        out.clear();
                    }
                }
            }
        }
        lk.lock();
        if (!stopped) inflight_--;
        stats_.batches++;
        if (flat) stats_.flatBatches++;
        if (mix && !stopped) stats_.mixedBatches++;
        if (B > stats_.largest) stats_.largest = B;
        lk.unlock();
        turn_cv_.notify_all(); // (leaders only: one per open group)
        out.resize(B);
        std::vector<SearchResult> mine = std::move(out[me]);
        g->results = std::move(out);
        g->set_done();
        return mine;
    }

  private:
    // IndexT::CombinesConcurrentCalls() if it exists, else false (a test double, an index behind another transport)
    template <class T> static auto combines(const T &i, int) -> decltype(i.CombinesConcurrentCalls()) { return i.CombinesConcurrentCalls(); }
    template <class T> static bool combines(const T &, long) { return false; }
    // ... and IndexT::SearchMixed the same way: an index without it (today's test doubles) keeps the (k, efSearch, list) keying
    template <class T>
    static auto mixes(T &i, int) -> decltype(i.SearchMixed((const float *)nullptr, 0u, std::declval<const std::vector<int> &>(),
                                                                 std::declval<const std::vector<int> &>(), (const AllowList *)nullptr), true) {
        return true;
    }
    template <class T> static bool mixes(T &, long) { return false; }
    template <class T>
    static auto search_mixed(T &i, int, const float *q, uint32_t B, const std::vector<int> &ks, const std::vector<int> &efs, const AllowList *a)
        -> decltype(i.SearchMixed(q, B, ks, efs, a)) {
        return i.SearchMixed(q, B, ks, efs, a);
    }
    template <class T>
    static std::vector<std::vector<SearchResult>> search_mixed(T &, long, const float *, uint32_t, const std::vector<int> &, const std::vector<int> &,
                                                               const AllowList *) {
        return {};
    }
    // a filter that allows less than flatScanSelectivity of the ids takes the exact scan, which answers k <= kMaxFlatK
    // (kdb_flat_scan_batch); larger k keeps the graph walk, which still answers -- routing must never turn a query the reference
    // would answer into [].  The library states the same rule once more, per filter program, for kdb_search_filtered:
    // kdb_filter_route_of (kektordb_amd/csrc/kdb_filter_plan.h, tested by tests/cpp/filter_plan_test.cpp)
    bool takes_flat_scan(int k, const AllowList *allowList) const {
        uint64_t allowed = 0;
        for (uint64_t w : allowList->words) allowed += (uint64_t)__builtin_popcountll(w);
        const uint32_t count = idx_.Count();
        return allowed > 0 && count > 0 && k <= kMaxFlatK && (double)allowed < opt_.flatScanSelectivity * (double)count;
    }
    using Key = std::tuple<int, int, const AllowList *>;
    struct Group {
        std::vector<const float *> queries; // callers' buffers: they are blocked in SearchWithScores until done
        std::vector<int> ks, efs;           // ... and what each of them asked for (a group over SearchMixed holds several)
        std::vector<std::vector<SearchResult>> results;
        bool sealed = false;               // (under mu_)
        std::atomic<uint32_t> done{0};     // futex word
        void wait_done() {
            while (done.load(std::memory_order_acquire) == 0u)
                (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(&done), FUTEX_WAIT_PRIVATE, 0u, nullptr, nullptr, 0);
        }
        void set_done() {
            done.store(1u, std::memory_order_release);
            (void)syscall(SYS_futex, reinterpret_cast<uint32_t *>(&done), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
        }
    };
    IndexT &idx_;
    Options opt_;
    mutable std::mutex mu_;
    std::condition_variable turn_cv_; // leaders waiting for a turn (or out their window)
    std::map<Key, std::shared_ptr<Group>> groups_;
    uint32_t inflight_ = 0;
    bool closed_ = false;
    Stats stats_;
};

// IndexT needs Dim(), Count(), SearchBatch(), FlatScanBatch() with Index's signatures (a test double can stand in)
using MicroBatcher = BasicMicroBatcher<Index>;

} // namespace hnsw
} // namespace kektor
