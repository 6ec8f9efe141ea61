/*
 * kektor_hip.h -- C ABI of libkektor_hip.so: the MI355X (gfx950) HNSW / flat-scan search path
 * that drops in behind KektorDB's hnsw.Index.SearchWithScores.
 *
 * Reference interfaces each entry point replaces (paths relative to the upstream repo):
 *
 *   kdb_search_batch        hnsw.Index.SearchWithScores -> searchInternal -> searchLayerUnlocked
 *                           pkg/core/hnsw/hnsw_index.go:343-366, 369-468, 2351-2611
 *                           (interface: core.VectorIndex.SearchWithScores, pkg/core/vector_index.go:35;
 *                            engine call sites pkg/engine/ops.go:1006 and :1296)
 *   kdb_flat_scan_batch     BruteForceIndex.SearchWithScores, pkg/core/vector_index.go:104-140
 *                           (the exact scan north_star routes filtered queries to)
 *   kdb_distance_batch      the per-pair distance FFI of native/compute/include/kektordb_compute.h:8-11
 *                           (squared_euclidean_f32 / dot_product_f32 / squared_euclidean_f16 /
 *                            dot_product_i8, bound by pkg/core/distance/distance_rust.go:12-17,57-125),
 *                           batched: B queries x C gathered candidate rows per call
 *   kdb_index_upload_rows   Node.vec slices into mmap.VectorArena (pkg/core/hnsw/hnsw_index.go:602-633,
 *                           pkg/storage/mmap/arena.go:378-447): same dense row-major row layout
 *   kdb_index_upload_arena  the arena files themselves (pkg/storage/mmap/arena.go:14-23,90-95,335-342,403-404)
 *   kdb_index_upload_graph  Node.Connections (pkg/core/hnsw/hnsw_node.go:13-68) as exported by
 *                           SnapshotData (hnsw_index.go:3064): per-level adjacency, entry point, maxLevel
 *   kdb_index_mark_deleted  Node.Deleted soft delete (hnsw_index.go:2303)
 *   kdb_index_build         addBatchInternal (hnsw_index.go:1479-2088), phases 1-4, on the GPU (fast linking)
 *   kdb_index_add_batch     the same phases with the reference's own linking: lists equal the restated batch insert's
 *   kdb_index_add           Add (hnsw_index.go:472-809), the sequential single insert: one node after another, each against the
 *                           graph the nodes before it left
 *   kdb_index_refine        GraphOptimizer.Refine / RunTurboRefine (pkg/core/hnsw/optimizer.go:288-560, :679-719): every
 *                           selected node re-linked against the graph as the call found it
 *   kdb_index_vacuum        GraphOptimizer.Vacuum (optimizer.go:133-277): nodes with links to deleted nodes found and re-linked,
 *                           the entry point re-elected, the deleted nodes' lists and rows cleared
 *   kdb_index_decode_rows   GetNodeData(...).Vector (hnsw_index.go:2909-2959) / the vectors of Engine.VGetMany: stored rows as the float32
 *                           vectors the reference hands to its callers (float16 widened, int8 through Quantizer.Dequantize,
 *                           pkg/core/hnsw/quantizer.go:181-198)
 *   kdb_search_by_id        VSearchWithScores(index, VGetMany(ids)[i].Vector, k) for a page of ids -- the loop of
 *                           Gardener.findRedundantClusters (pkg/cognitive/gardener.go:803-869; again at :915, :1362, :2348) --
 *                           as ONE call in which the rows never leave the device
 *   kdb_flat_scan_by_id     the same in front of the exact scan (BruteForceIndex.SearchWithScores)
 *   kdb_consensus_batch     CalculateConsensus (pkg/engine/epistemic_types.go:126-178) over the stored vectors of id lists, with the
 *                           per-node similarity of Engine.VBeliefState (pkg/engine/epistemic.go:22-182, :81): centroid, distances to
 *                           it, pair distances and the score in ONE kernel, about 40 bytes per list back
 *   kdb_belief_batch        the search of VBeliefState (:45) and that consensus as one call: the k result rows never leave the device
 *   kdb_index_set_column    the metadata indexes AddMetadataUnlocked fills (pkg/core/core.go:1640-1758: strings and bools in the inverted
 *                           index, float64 in the B-tree) as per-id columns in HBM
 *   kdb_filter_parse        the filter grammar of DB.FindIDsByFilter / evaluateBooleanFilter / findFilterOperator (core.go:44-48,
 *                           :1766-1839, :1866-1897, :1900-2034), host only
 *   kdb_filter_eval         FindIDsByFilter itself for P filters at once: predicate programs over the columns -> P dense allow lists
 *                           and their cardinalities in one streaming kernel (`!=`: live minus matched, :1998-2029, without the walk over
 *                           every node of GetAllValidNodeIDs, hnsw_index.go:2884-2900)
 *   kdb_search_filtered     Engine.VSearch(index, query, k, filter, ...) from programs to answers (pkg/engine/ops.go:928-1007): lists,
 *                           routing between walk and exact scan, answers, as one call
 *   kdb_merge_topk          the merge step of the id-range shard (no reference
 *                           counterpart -- the reference is single process)
 *   kdb_sharded_search_batch  the same path over every GPU of a node from ONE process: fan-out,
 *                           one RCCL all-gather of the per-shard top-k, merge
 *
 * Conventions (mirroring native/compute's embedder half, native/compute/src/embedder.rs:33-63):
 *   - every function returns 0 on success and a negative kdb_status on failure; the message for the
 *     calling thread is available from kdb_last_error(); nothing throws or unwinds across the ABI;
 *   - the caller owns every buffer it passes; host inputs are consumed before the call returns
 *     (cgo rule: Go memory need not stay pinned after the call);
 *   - handles are opaque, usable from any thread, and CONCURRENT callers are served concurrently, as the reference's
 *     read lock allows (hnsw_index.go:343-352; pkg/engine/ops.go:1003-1007 calls SearchWithScores from a goroutine per
 *     request).  The host-pointer entry points (kdb_search_batch, kdb_flat_scan_batch, kdb_distance_batch) hold the handle's
 *     lock only to pick one of KDB_SLOTS (4, at most 16) slots -- a stream and a pair of staging buffers -- and to enqueue;
 *     they wait for their answers outside it.  One-query callers that find every slot busy are combined: calls of up to
 *     KDB_COMBINE_MAX_B (16) queries with the same flags and no allow list -- whatever their k and ef: the launch reads them
 *     per query, kdb_search_batch_mixed below; KDB_COMBINE_MIXED=0 at kdb_index_create: the same (k, ef) only -- leave as ONE
 *     launch as soon as a slot is
 *     free (no window, no timer: a lone caller never waits), and that launch stays open for KDB_SESSION_US (300) microseconds:
 *     a call it can hold that arrives while its kernel runs is written into its page-locked buffer and walked by a workgroup that
 *     waited for it -- no launch of its own (with KDB_SEARCH_HEAP_ORDER a query that meets equal distances is answered once its
 *     launch has closed: up to that window later); kdb_index_caller_stats counts launches and the calls they carried.
 *     Writers -- uploads, kdb_index_mark_deleted, kdb_index_set_entry, build / add_batch, reserve, destroy -- wait until no
 *     host-pointer call is in flight and hold new ones back meanwhile (the reference's write lock).  The *_dev entry points
 *     are asynchronous on the stream they are given; the index keeps a set of per-call scratch per stream in use (up to 18):
 *     a *_dev call on a stream other than the one that last used its set first waits -- on the device -- for that use, so
 *     any number of streams is SAFE; for kernels already launched on a caller's stream a writer's change is a snapshot;
 *   - ids are the reference's internal ids: uint32, 1-based, id 0 never names a vector
 *     (hnsw_index.go:590); at most 2^30-1 ids per index;
 *   - distances are returned as the RAW f32 accumulate: sum (q-x)^2 for KDB_METRIC_L2, the dot
 *     product for KDB_METRIC_COSINE (f32), the f64-scaled cosine distance for int8.  The shim applies
 *     the reference's f64 epilogue -- float64(sum) (distance_go.go:67) or 1.0-float64(dot)
 *     (distance_go.go:127) -- when it fills types.SearchResult.Score (pkg/core/types/types.go:12-15).
 *   - values that are not finite cannot hurt anybody else's call.  A graph-search query with a NaN or an infinity among its
 *     components is answered with NO results (out_count 0 -- the reference's "log and return an empty slice" for a search that
 *     fails, hnsw_index.go:356-359; the reference itself compares the NaN distances that follow like any others and returns
 *     whatever its heaps then hold: nothing to be bit-exact with) and never walks; the other queries of the batch -- and of a
 *     launch it was combined into -- are answered bit for bit as alone.  "Not finite" is judged on the PREPARED query, the form
 *     the rows are compared with: on a float16 index a finite component of 65520 or more is an infinity after the float16 round
 *     trip and the query is such a query (an int8 query is judged on the caller's values: its prepared form is integers); with
 *     KDB_SEARCH_PREPARED the caller's values are the prepared form.  ONE rule for every entry point: the graph search (either
 *     walk order), the search by stored id, the exact scans -- out_count 0, ids 0, distances +Inf -- and kdb_distance_batch[_dev],
 *     which reports +Inf for every candidate of such a query.  A stored row that yields a distance that is not a
 *     number is "infinitely far" in a walk, never nearer than anything.  Every node id is range-checked before a row or list
 *     address is formed from it;
 *   - there is NO CPU fallback: every compute entry point fails with KDB_ERR_NO_DEVICE when no gfx950
 *     device is visible.
 */
#ifndef KEKTOR_HIP_H
#define KEKTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDB_ABI_VERSION 2 /* 2: kdb_counters.n_tied; KDB_SEARCH_TIE_FLAG / KDB_SEARCH_HEAP_ORDER; kdb_index_reserve; cluster poisoning */
#if defined(__GNUC__)
#define KDB_API __attribute__((visibility("default")))
#else
#define KDB_API
#endif

typedef enum {
    KDB_OK = 0,
    KDB_ERR_INVALID = -1,   /* bad argument */
    KDB_ERR_NO_DEVICE = -2, /* no HIP device / not gfx950 */
    KDB_ERR_HIP = -3,       /* a HIP runtime call failed */
    KDB_ERR_OOM = -4,
    KDB_ERR_STATE = -5,     /* e.g. search before a graph was uploaded */
    KDB_ERR_UNSUPPORTED = -6,
    KDB_ERR_DIVERGED = -7   /* KDB_SEARCH_FAIL_ON_DROP: answers delivered, but a walk was not the reference's step for step */
} kdb_status;

enum { KDB_METRIC_L2 = 0, KDB_METRIC_COSINE = 1 };       /* distance.Euclidean / distance.Cosine */
enum { KDB_PREC_F32 = 0, KDB_PREC_F16 = 1, KDB_PREC_I8 = 2 }; /* arena.go:73-77 PrecFloat32/16/Int8 */

/* kdb_search_batch flags */
enum {
    KDB_SEARCH_STRICT = 0,            /* one candidate expanded per step: the reference's best-first order */
    KDB_SEARCH_NEEDS_REFINE = 1u << 0, /* apply the needsRefine ef boost (hnsw_index.go:387-399)            */
    KDB_SEARCH_PREPARED = 1u << 1,     /* queries are already in stored form (normalised); skip query prep  */
    KDB_SEARCH_FAIL_ON_DROP = 1u << 2  /* kdb_search_batch (host pointers) only: return KDB_ERR_DIVERGED when a walk had to discard  *
                                        * pending traversal-only candidates (more than 2047 soft-deleted nodes waiting at once:       *
                                        * kdb_counters.n_dropped > 0), i.e. when some answer may differ from the reference's walk.    *
                                        * The outputs are still filled.  Without the flag the count is only reported.                */
    ,
    KDB_SEARCH_DIST_F64 = 1u << 3      /* int8 indexes, kdb_search_batch[_dev] and kdb_flat_scan_batch[_dev]: out_dist points to B*k    *
                                        * DOUBLES and receives the reference's float64 distances (hnsw_index.go:2429-2454 computes and *
                                        * orders them as float64).  Without the flag the same doubles are rounded to float on the way  *
                                        * out; the ORDER of the results is the float64 order either way.  Other precisions: INVALID.   */
    ,
    /* Equal distances.  The reference keeps candidates and results in two binary heaps (hnsw_heap.go): when two DIFFERENT nodes
     * are at exactly the same distance from the query (duplicate vectors), which one it expands first, evicts from a full
     * result set or reports first depends on the history of those heaps.  The walk of this library orders such nodes by id, so
     * ids, their order and the walk's counters can differ from the reference's on exactly those queries -- and ONLY on those:
     * a walk that never holds two nodes at one distance is the reference's walk step for step.                            */
    KDB_SEARCH_TIE_FLAG = 1u << 4,    /* out_count[b] carries bit 31 (KDB_COUNT_TIED) when query b's walk met such a tie and *
                                       * was not re-walked: mask the count with KDB_COUNT_MASK.  A shim can route exactly    *
                                       * those queries to the reference's own Go walk.                                        */
    KDB_SEARCH_HEAP_ORDER = 1u << 5   /* every such query is walked again, in the same call, with the reference's two heaps and  *
                                       * their sift rules (hnsw_heap.go:53-82,122-151; search_heap.hip): ids, order, distances  *
                                       * and counters are then the reference's, ties included.  The fast path is untouched; a   *
                                       * tied query costs one slow walk.  With KDB_SEARCH_TIE_FLAG the bit stays set only on a   *
                                       * query whose candidate heap outgrew its scratch (counted in kdb_counters.n_dropped).    */
};
#define KDB_COUNT_TIED 0x80000000u
#define KDB_COUNT_MASK 0x7fffffffu

typedef struct kdb_index kdb_index;

typedef struct {
    uint32_t dim;
    uint32_t metric;     /* KDB_METRIC_*  */
    uint32_t precision;  /* KDB_PREC_*    */
    uint32_t m;          /* 0 -> 16; mMax0 = 2m (hnsw_index.go:140-151) */
    uint32_t ef_construction; /* 0 -> 200 */
    uint32_t capacity;   /* largest internal id the index may hold */
    int32_t device_id;   /* HIP device ordinal */
    uint32_t reserved;   /* flags: KDB_INDEX_NO_F16_SHADOW | KDB_INDEX_NO_WALK_PLANES */
} kdb_index_desc;
/* float32 indexes that are scanned exactly keep a second copy of the rows as halfs (+50 % row memory), made by the
 * FIRST kdb_flat_scan_* call (an index that is only walked never allocates it): the exact scan RANKS on it (half the
 * HBM bytes for small batches, the f16 MFMA for large ones) inside a rigorous error band and settles on the float32
 * rows, so answers are unchanged.  Set this bit to do without the copy for good.                               */
#define KDB_INDEX_NO_F16_SHADOW 1u
/* float32 cosine indexes of 768 columns that are walked in large batches at ef <= 256 (the one-wave kernel: more queries
 * than the latency modes take) keep the rows once more as two 16-bit planes -- the high and the low halves of every float --
 * and one float32 error bound per row: +100 % row memory while they exist (12.5M x 768: 38 GB of rows + 19 + 19 GB of
 * planes), made by the FIRST such walk (small batches, L2 and quantised indexes never allocate them).  A hop whose beam is
 * full reads the high plane first and fetches the low plane only of the candidates it cannot prove too far; the proof is
 * rigorous and survivors are evaluated on the reassembled float32 values, so answers, distances and counters are unchanged.
 * Set this bit to do without the planes for good.                                                                        */
#define KDB_INDEX_NO_WALK_PLANES 2u

/* Per-level CSR adjacency.  offsets[l] has count+2 entries: node i's neighbours at level l are
 * neighbors[l][offsets[l][i] .. offsets[l][i+1]) (empty when levels[i] < l).  Lists keep the
 * reference's stored order.                                                                     */
typedef struct {
    uint32_t count;        /* nodeCounter: ids 1..count exist                          */
    uint32_t entry;        /* entrypointID                                             */
    int32_t max_level;     /* maxLevel, -1 for an empty graph                          */
    uint32_t reserved;
    const uint8_t *levels;            /* [count+1], levels[0] ignored                  */
    const uint64_t *const *offsets;   /* [max_level+1] pointers                        */
    const uint32_t *const *neighbors; /* [max_level+1] pointers                        */
    const uint64_t *deleted_bits;     /* NULL or ((count>>6)+1) words, bit id set = deleted */
} kdb_graph_view;

typedef struct {
    uint64_t n_dist;       /* distance evaluations of the last search call             */
    uint64_t n_hops;       /* expanded candidates of the last search call; flat scan:  *
                            * low word = queries settled by the exact pass of the      *
                            * f16-ranked scan, high word = by the rescue pass           */
    uint64_t bytes;        /* algorithmic bytes of the last call   */
    double last_kernel_ms; /* HIP-event duration of the dominant kernel of the last call */
    uint64_t n_dropped;    /* graph search: pending traversal-only candidates (deleted    *
                            * nodes) discarded because more than 2048 were waiting; 0 =   *
                            * the walk was the reference's, step for step (under         *
                            * KDB_SEARCH_HEAP_ORDER also: tied walks left unresolved)     */
    uint64_t n_tied;       /* graph search: queries whose walk met two different nodes at  *
                            * EQUAL distance (the reference's order then depends on its    *
                            * heaps' history: KDB_SEARCH_TIE_FLAG / KDB_SEARCH_HEAP_ORDER)  */
} kdb_counters;

typedef struct {
    uint32_t batch;         /* nodes inserted per GPU round (0 = auto)                 */
    uint32_t ef_construction; /* 0 = index default                                     */
    uint64_t seed;          /* level draw (hnsw_index.go:2616-2625 uses the global RNG) */
    uint32_t flags;
    uint32_t reserved;
} kdb_build_params;

KDB_API int kdb_abi_version(void);
KDB_API int kdb_hip_device_count(void);
KDB_API const char *kdb_last_error(void);

KDB_API int kdb_index_create(const kdb_index_desc *desc, kdb_index **out);
KDB_API void kdb_index_destroy(kdb_index *idx);
/* growNodes (pkg/core/hnsw/hnsw_index.go:2732-2768: the reference doubles its node table when an id outgrows it): raise the
 * capacity of a live index.  Rows, ranking copy, norms, lists, levels and deleted bits move to larger allocations ON THE DEVICE
 * (nothing is re-uploaded; the graph stays); a capacity at or below the current one is a no-op; KDB_ERR_OOM leaves the index as
 * it was.  The call waits for the device (walks in flight read the arrays that move).                                       */
KDB_API int kdb_index_reserve(kdb_index *idx, uint32_t new_capacity);
/* Give back the half-precision ranking copy of a float32 index (see KDB_INDEX_NO_F16_SHADOW); the next exact scan makes it
 * again unless refuse_for_good != 0.                                                                                        */
KDB_API int kdb_index_drop_f16_shadow(kdb_index *idx, int refuse_for_good);
/* Give back the walk planes (see KDB_INDEX_NO_WALK_PLANES); the next large-batch walk makes them again unless
 * refuse_for_good != 0.                                                                                                    */
KDB_API int kdb_index_drop_walk_planes(kdb_index *idx, int refuse_for_good);

/* Incremental refresh of the mirror after writers (Add / AddBatch / optimizer) touched a FEW nodes, instead of a full
 * kdb_index_upload_graph:
 *   1. kdb_index_upload_rows for the new ids (they continue at count+1, as nodeCounter does, hnsw_index.go:590);
 *   2. kdb_index_append_nodes(first_id, n, levels) -- registers them (levels as len(Connections)-1), lists empty;
 *   3. kdb_index_patch_adjacency(level, ...) per level -- replaces the lists of the touched nodes (new nodes and
 *      every node whose Connections[level] changed: reverse links, re-prunes); lists keep the stored order;
 *   4. kdb_index_set_entry(entrypointID, maxLevel).
 * Searches issued between the steps see a graph that is consistent per list, exactly as concurrent readers of the
 * reference do under its fine-grained shard locks.                                                            */
KDB_API int kdb_index_append_nodes(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels);
KDB_API int kdb_index_patch_adjacency(kdb_index *idx, uint32_t level, uint32_t n, const uint32_t *ids,
                              const uint64_t *offsets /* n+1 */, const uint32_t *neighbors);
KDB_API int kdb_index_set_entry(kdb_index *idx, uint32_t entry, int32_t max_level);

/* Rows in stored form, row-major, `n` rows for ids first_id..first_id+n-1 (cosine/f32 rows already
 * normalised, f16 as IEEE binary16 bits, int8 quantised).  *_dev takes a device pointer.          */
KDB_API int kdb_index_upload_rows(kdb_index *idx, uint32_t first_id, uint32_t n, const void *rows);
KDB_API int kdb_index_upload_rows_dev(kdb_index *idx, uint32_t first_id, uint32_t n, const void *d_rows);
/* int8 only: quantizedNorms[id] (hnsw_index.go:3371-3377) and the quantizer's AbsMax.            */
KDB_API int kdb_index_upload_norms(kdb_index *idx, uint32_t first_id, uint32_t n, const float *norms);
KDB_API int kdb_index_set_quantizer(kdb_index *idx, float abs_max);
KDB_API int kdb_index_upload_graph(kdb_index *idx, const kdb_graph_view *g);
KDB_API int kdb_index_mark_deleted(kdb_index *idx, const uint32_t *ids, uint32_t n);
/* Populate rows 1..count straight from a KektorDB data directory: the arena_%04d.bin files of
 * pkg/storage/mmap/arena.go (64 MiB chunks, 64-byte header {LE u32 magic 0x4B414F4E, version 1, dim,
 * u8 precision}, rows dense at 64 + (slot % vecsPerChunk)*vectorSize).  slot_table[id] = physical slot
 * of internal id (ArenaState.SlotTable, arena.go:252-270; 0xFFFFFFFF = unallocated -> zero row), or
 * NULL for the identity id -> id-1.  kdb_arena_read_rows is the host-only half (no GPU needed): it
 * gathers rows first_id..first_id+n-1 into a dense buffer.                                          */
KDB_API int kdb_index_upload_arena(kdb_index *idx, const char *dir, const uint32_t *slot_table, uint32_t count);
KDB_API int kdb_arena_read_rows(const char *dir, uint32_t dim, uint32_t precision, const uint32_t *slot_table,
                        uint32_t first_id, uint32_t n, void *out_rows);
/* Rows without a graph (flat scan only): declare ids 1..count present.                            */
KDB_API int kdb_index_set_count(kdb_index *idx, uint32_t count);

/* Copies the device graph back in the kdb_graph_view layout.  Call once with neighbors == NULL to
 * get sizes: level_sizes[l] = number of neighbour ids at level l (array of max_level+1).         */
KDB_API int kdb_index_graph_info(kdb_index *idx, uint32_t *count, uint32_t *entry, int32_t *max_level);
KDB_API int kdb_index_download_graph(kdb_index *idx, uint8_t *levels, uint64_t *const *offsets,
                             uint32_t *const *neighbors, uint64_t *level_sizes);
KDB_API int kdb_index_download_rows(kdb_index *idx, uint32_t first_id, uint32_t n, void *rows);

/* Heterogeneous batch: what a micro-batcher hands over when concurrent SearchWithScores callers carry DIFFERENT
 * allow lists (ops.go builds one roaring bitmap per request).  d_allow_lists holds G dense bitsets back to back,
 * words_per_list (>= (count>>6)+1) uint64 words each; query b uses list d_allow_of_query[b], KDB_NO_FILTER = no
 * list.  Per query the result is exactly that of kdb_search_batch with its list (entry-point substitution, empty
 * list => no results, hnsw_index.go:437-447, decided per list on the device).  Device pointers.                */
#define KDB_NO_FILTER 0xffffffffu
KDB_API int kdb_search_batch_multi_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                               const uint64_t *d_allow_lists, uint32_t G, uint64_t words_per_list,
                               const uint32_t *d_allow_of_query, uint32_t flags, uint32_t *d_out_ids,
                               float *d_out_dist, uint32_t *d_out_count, void *stream);

/* SearchWithScores for B requests that differ in k and efSearch: query b is answered exactly as kdb_search_batch answers it alone
 * with (k[b], ef[b]) -- ids, distances, order, counters.  out_ids / out_dist are [B][k_stride], out_count [B]; positions
 * [count, k_stride) of a row hold id 0 and +inf.  ONE launch walks them all: its beam is sized for the largest effective ef of the
 * batch (the KDB_SEARCH_NEEDS_REFINE boost first, then max(ef, k)), rounded up to the top of its beam class -- 64, 128, 256, or the
 * value itself above 256 (kdb_mixed_plan.h holds the rules).  A small-ef query walked in a larger class returns the same answer.
 * Host pointers: any k[b] == 0 or k[b] > k_stride is KDB_ERR_INVALID and nothing is launched; allow_bits as for kdb_search_batch
 * (one optional list for the whole batch).  Flags as for kdb_search_batch; kdb_search_set_trace applies.  The call goes out alone,
 * through a slot or (traced, KDB_SEARCH_FAIL_ON_DROP, too large for a slot) on a turn of the index's staging buffer; it is not cut
 * into chunks.
 * Device pointers: the host cannot read d_k / d_ef, so the caller states ef_max, the largest effective ef it will send; a query with
 * k == 0, k > k_stride or an effective ef above the launch's capacity comes back as count 0 | KDB_MIXED_BAD_QUERY (bit 30 of
 * out_count) and is never walked.  Per-query allow lists as for kdb_search_batch_multi_dev; G == 0: d_allow_lists is one optional
 * list shared by the batch, as kdb_search_batch_dev has it.
 * kdb_index_mixed_stats, out[4]: [0] launches that carried at least two distinct (k, effective ef), [1] the calls they carried,
 * [2] callers that could not join an open launch because of their k or ef, [3] reserved (0).  ([0] and [1] count host-pointer
 * calls: the library never reads the device arrays of the _dev form.) */
#define KDB_MIXED_BAD_QUERY 0x40000000u
KDB_API int kdb_search_batch_mixed(kdb_index *idx, const float *queries, uint32_t B, const uint32_t *k, const uint32_t *ef,
                                   uint32_t k_stride, const uint64_t *allow_bits, uint32_t flags,
                                   uint32_t *out_ids, float *out_dist, uint32_t *out_count);
KDB_API int kdb_search_batch_mixed_dev(kdb_index *idx, const float *d_queries, uint32_t B, const uint32_t *d_k, const uint32_t *d_ef,
                                       uint32_t k_stride, uint32_t ef_max,
                                       const uint64_t *d_allow_lists, uint32_t G, uint64_t words_per_list, const uint32_t *d_allow_of_query,
                                       uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream);
KDB_API int kdb_index_mixed_stats(kdb_index *idx, uint64_t *out /* [4] */);

/* SearchWithScores for B queries.  queries: [B][dim] f32, un-normalised (the library performs the
 * reference's query prep, hnsw_index.go:404-434).  allow_bits: NULL (nil allow-list) or
 * ((count>>6)+1) uint64 words (a zero bitmap is the non-nil EMPTY list -> zero results).
 * Outputs: out_ids/out_dist [B][k], out_count [B].
 * Host pointers: batches of 8192 queries and more run as four chunks that alternate between two internal
 * streams, so the copies of one chunk travel under the walk of another (32768 queries: 9.8 -> 8.4 ms including
 * both copies); the answers are those of one launch.                                               */
KDB_API int kdb_search_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef,
                     const uint64_t *allow_bits, uint32_t flags, uint32_t *out_ids, float *out_dist,
                     uint32_t *out_count);
/* Same with every pointer in device memory, asynchronous on `stream` (a hipStream_t, may be NULL). */
KDB_API int kdb_search_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                         const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids,
                         float *d_out_dist, uint32_t *d_out_count, void *stream);
/* Optional per-query instrumentation of the NEXT search call: device or host arrays [B] are filled
 * with n_dist / n_hops per query (pass NULL to disable).                                          */
KDB_API int kdb_search_set_trace(kdb_index *idx, uint32_t *per_query_ndist, uint32_t *per_query_nhops, int on_device);

/* Exact scan over every non-deleted (and allowed) row.  An EMPTY allow list means "no filter"
 * (vector_index.go:130).  k <= 1024 (the matrix-core kernels serve k <= 128; above that every distance is computed in the final order and a radix select per query picks the k smallest: exact for any k, HBM-bound on the rows).  The answer is the exact top-k under the index's own distance (total order:
 * distance, then id); reported distances are computed in the accumulation order of kdb_search_batch, so a (query,
 * row) pair has the same distance bits from either entry point.  Internally the matrix cores rank (f32 / f16 / i8
 * MFMA; float32 rows of large batches on the f16 MFMA inside a rigorous error band) and the finalists are re-scored;
 * queries the band cannot settle are answered by the exact kernel in the same call.                          */
KDB_API int kdb_flat_scan_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k,
                        const uint64_t *allow_bits, uint32_t flags, uint32_t *out_ids, float *out_dist,
                        uint32_t *out_count);
KDB_API int kdb_flat_scan_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k,
                            const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids,
                            float *d_out_dist, uint32_t *d_out_count, void *stream);

/* Grouped exact scan -- the filtered path for a micro-batch whose callers carry DIFFERENT allow lists: the queries
 * of group g are rows [group_offsets[g], group_offsets[g+1]) of d_queries (group_offsets: HOST array of G+1 entries,
 * 0 ... B) and are scanned against the rows list g allows (a list that allows nothing yields no results; deleted
 * rows never appear).  d_allow_lists: G dense bitsets back to back, words_per_list uint64 words each.
 * max_total_allowed: an upper bound on the summed cardinalities of the lists (the shim has them from roaring in
 * O(1)); 0 = let the library count (one small read-back).  float32 / float16 indexes.                          */
KDB_API int kdb_flat_scan_groups_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t G,
                             const uint32_t *group_offsets, const uint64_t *d_allow_lists, uint64_t words_per_list,
                             uint64_t max_total_allowed, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist,
                             uint32_t *d_out_count, void *stream);

/* GetNodeData(id).Vector (hnsw_index.go:2909-2959), the vectors Engine.VGetMany returns, for n ids: out[i] = the stored row of
 * ids[i] as `dim` float32 (out: [n][dim], dense, no padding) --
 *   float32   the stored row, bit for bit (a cosine row stays normalised, as stored);
 *   float16   every half widened (exact);
 *   int8      Quantizer.Dequantize (quantizer.go:181-198): (float32(v) / 127) * AbsMax, in that order, in correctly rounded
 *             float32; AbsMax == 0 (untrained): zeros.
 * An id that is 0, above count, or marked deleted is "not found" (:2921-2931): its row is zeros and out_found[i] = 0.  out_found:
 * NULL or n BYTES (uint8_t), 1 = found.  ids may repeat.  Every id is range-checked before an address is formed from it.  One
 * gather kernel (by_id.hip).  The host-pointer form stages through the index in pieces of at most 64 MiB of vectors.            */
KDB_API int kdb_index_decode_rows(kdb_index *idx, const uint32_t *ids, uint32_t n, float *out, uint8_t *out_found);
KDB_API int kdb_index_decode_rows_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t n, float *d_out, uint8_t *d_out_found, void *stream);

/* Search BY STORED ID -- "more like this".  Gardener.findRedundantClusters (pkg/cognitive/gardener.go:803-869) pages 500 ids with
 * VGetIDsByCursor, reads them with VGetMany and runs VSearchWithScores(indexName, vData.Vector, 10) for each (the same loop at
 * :915, :1362 and :2348): every query is a vector that was just read OUT of the index.  Here the page is one call and an id is what
 * crosses the bus.
 * DEFINITION: query b is the vector kdb_index_decode_rows gives for ids[b]; the answer -- ids, distance bits, out_count, the
 * per-query trace (kdb_search_set_trace) and kdb_counters -- is exactly that of kdb_search_batch[_dev] for that float32 vector with
 * the same (k, ef, allow list, flags).  The call IS that composition: the rows are decoded into scratch of their own and the
 * existing walk runs on them, query prep included (searchInternal prepares GetNodeData's vector like any other, :404-434: a
 * float32 cosine row is normalised again, an int8 row quantised again) -- KDB_SEARCH_PREPARED is therefore refused (KDB_ERR_INVALID).
 * A source id that is not found (0, above count, deleted) gets out_count[b] = 0 and a zeroed id row and is never walked (inside,
 * it is a query that is not finite: "Conventions"); the other queries are unaffected.  A stored row that holds a NaN or an
 * infinity is such a query too.  A batch of not-found ids only: KDB_OK, every count 0.
 * Flags: KDB_SEARCH_NEEDS_REFINE, KDB_SEARCH_FAIL_ON_DROP (kdb_search_by_id only), KDB_SEARCH_DIST_F64 (int8 only),
 * KDB_SEARCH_TIE_FLAG, KDB_SEARCH_HEAP_ORDER, and
 *   KDB_BY_ID_DROP_SELF   a stored row's nearest neighbour is itself.  The call runs with k + 1 and the caller's [B][k] arrays
 *                         receive that answer WITHOUT the entry whose id is ids[b] (there is at most one), or -- when it is not
 *                         among them, e.g. the allow list excludes it -- without the LAST entry if all k + 1 came back.  Order
 *                         and distance bits are otherwise those of the k + 1 call, out_count is adjusted (bit 31 kept), the trace
 *                         and the counters are those of the k + 1 call.  kdb_flat_scan_by_id: k <= 1023, else KDB_ERR_INVALID.
 * kdb_search_by_id (host pointers) takes turns on the index's staging buffer like kdb_distance_batch, synchronises once and is
 * never combined with other callers' queries; kdb_flat_scan_by_id[_dev] is the same composition in front of kdb_flat_scan_batch
 * (k <= 1024).  The grouped scan, the multi-list walk and the sharded entry points have no by-id form.                          */
#define KDB_BY_ID_DROP_SELF (1u << 8)
KDB_API int kdb_search_by_id(kdb_index *idx, const uint32_t *ids, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                             uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count);
KDB_API int kdb_search_by_id_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t B, uint32_t k, uint32_t ef,
                                 const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist,
                                 uint32_t *d_out_count, void *stream);
KDB_API int kdb_flat_scan_by_id(kdb_index *idx, const uint32_t *ids, uint32_t B, uint32_t k, const uint64_t *allow_bits,
                                uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count);
KDB_API int kdb_flat_scan_by_id_dev(kdb_index *idx, const uint32_t *d_ids, uint32_t B, uint32_t k, const uint64_t *d_allow_bits,
                                    uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream);

/* CalculateConsensus ON THE DEVICE for B id lists (consensus.hip) -- the arithmetic half of Engine.VBeliefState
 * (pkg/engine/epistemic.go:22-182; the Gardener calls it per reflection, pkg/cognitive/gardener.go:3358-3421), which searches, reads
 * the k result vectors back with VGet and runs CalculateConsensus (pkg/engine/epistemic_types.go:126-178) on them.
 * A LIST: list b is ids[b][0 .. counts[b] & KDB_COUNT_MASK) of the array ids[B][stride]; a search call's out_count can be passed
 * straight in, tie bit included.  counts == NULL: every list has `stride` entries.  stride <= KDB_CONSENSUS_MAX_K and every count
 * <= stride, else KDB_ERR_INVALID (the _dev form cannot see device counts: it clamps a count to stride).  Ids may repeat; each
 * occurrence is a node.
 * A NODE'S VECTOR is what kdb_index_decode_rows gives for the id (float32 as stored, float16 widened, int8 dequantised; the same
 * device routine, kdb_decode.cuh).  An id that is 0, above count or deleted is skipped, as the `continue` at epistemic.go:56 does;
 * every id is range-checked before an address is formed.  The metric of the index plays no part: the reference calls
 * CosineDistance (epistemic_types.go:299-320) whatever the index is.
 * active_bits: NULL (all active) or a bitset laid out like an allow list ((count >> 6) + 1 words, bit id).  Found nodes whose bit is
 * clear are the historical ones (epistemic.go:104-111): they count in n_found and get a similarity, and take no part in the
 * consensus.
 * THE CONSENSUS, over the active nodes in list order (:126-178):
 *   n_active == 0   score 0, variance 0, max_pair 0, a zero centroid; the call still returns KDB_OK;
 *   n_active == 1   score 1, variance 0, max_pair 0, the centroid is that vector, bit for bit;
 *   otherwise       the centroid is accumulated per column in float32 from 0, node after node, then divided by float32(n) (correctly
 *                   rounded); variance = (sum over the nodes, in order, of CosineDistance(node, centroid)^2) / n; max_pair = the
 *                   largest CosineDistance of a pair (maxVar: a NaN never wins, `d > maxVar` is false for it); score = 1 when
 *                   max_pair < 1e-10, else 1 - math.Min(variance / (max_pair * max_pair), 1).
 *   CosineDistance  dot, |a|^2 and |b|^2 are float64 sums over the columns in ascending order of products of widened float32
 *                   values (exact in float64, so fused and unfused multiply-add agree); a zero norm gives 1; otherwise
 *                   1 - max(0, min(1, dot / (sqrt(|a|^2) * sqrt(|b|^2)))) with Go's math.Max / math.Min: a NaN stays a NaN.
 * out_similarity: NULL or [B][stride] doubles: 1 - CosineDistance(vector_i, queries[b]) with the raw query, not normalised (:81), for
 * every found entry, active or not; -1.0 for an entry that was not found or lies beyond the count.  queries (float32 [B][dim]) may
 * be NULL only if out_similarity is NULL, else KDB_ERR_INVALID.
 * out_centroid: NULL or [B][dim] float32.  out_gram: NULL or [B][stride + 1][stride + 1] doubles, the raw accumulators: entry
 * (i, j) is the dot product of list entries i and j, the diagonal holds the squared norms, index `stride` is the centroid; rows
 * and columns of entries that are not active (not found, historical, beyond the count) are zero.
 * The Gardener's centroid of stored ids (gardener.go:3403-3412) is out_centroid of a call on that list.
 * flags must be 0.  B == 0: KDB_OK.  Nothing is written to the index: ordered like a search.  The host-pointer form takes turns on
 * the index's staging buffer like kdb_search_by_id and synchronises once.                                                          */
#define KDB_CONSENSUS_MAX_K 64u          /* the reference caps k at 50 (epistemic.go:31) */
typedef struct kdb_consensus {           /* 32 bytes */
    double score, variance, max_pair;    /* CalculateConsensus's score, variance, maxVar */
    uint32_t n_found;                    /* len(nodes): list entries whose row was found */
    uint32_t n_active;                   /* len(activeNodes) */
} kdb_consensus;
KDB_API int kdb_consensus_batch(kdb_index *idx, const uint32_t *ids, const uint32_t *counts, uint32_t B, uint32_t stride,
                                const float *queries, const uint64_t *active_bits, uint32_t flags, kdb_consensus *out,
                                double *out_similarity, float *out_centroid, double *out_gram);
KDB_API int kdb_consensus_batch_dev(kdb_index *idx, const uint32_t *d_ids, const uint32_t *d_counts, uint32_t B, uint32_t stride,
                                    const float *d_queries, const uint64_t *d_active_bits, uint32_t flags, kdb_consensus *d_out,
                                    double *d_out_similarity, float *d_out_centroid, double *d_out_gram, void *stream);
/* VBeliefState's search and consensus as ONE call, a composition like the by-id calls: kdb_search_batch[_dev] runs unchanged with
 * (k <= KDB_CONSENSUS_MAX_K, ef, allow list, flags) -- out_ids, out_dist, out_count, the trace and the counters are exactly its own
 * -- and the consensus kernel then runs on those id lists and counts with the same queries (stride = k).  out_similarity: NULL or
 * [B][k].  KDB_SEARCH_PREPARED is refused: the similarity is defined on the raw query.  The host-pointer form takes turns on the
 * staging buffer like kdb_search_by_id and is never combined with other callers' queries.                                         */
KDB_API int kdb_belief_batch(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                             const uint64_t *active_bits, uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count,
                             kdb_consensus *out, double *out_similarity);
KDB_API int kdb_belief_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                                 const uint64_t *d_allow_bits, const uint64_t *d_active_bits, uint32_t flags, uint32_t *d_out_ids,
                                 float *d_out_dist, uint32_t *d_out_count, kdb_consensus *d_out, double *d_out_similarity, void *stream);

/* ---- metadata filters on the device (filter.hip; geometry and validation in kdb_filter_plan.h) ---------------------------------
 * The reference turns a filter string into a roaring bitmap on the host: DB.FindIDsByFilter (pkg/core/core.go:1766-1839) splits on
 * OR, then AND, and evaluateBooleanFilter (:1900-2034) answers each comparison from the inverted index (strings, bools) or the
 * B-tree (float64), both filled by AddMetadataUnlocked (:1640-1758); Engine.VSearch hands the bitmap to SearchWithScores as the
 * allow list.  Here the metadata lives in HBM as COLUMNS indexed by internal id, a filter is a small PREDICATE PROGRAM, and one
 * streaming kernel writes the allow lists -- in the layout every filtered entry point above takes -- and their cardinalities.
 *
 * COLUMNS.  A node has at most one value per key: a string / bool (inverted index) or a float64 (B-tree).  Up to KDB_MAX_COLUMNS
 * slots per index, each capacity+1 entries:
 *   KDB_COL_F64   8 bytes per id, the B-tree value; NaN = the node has no numeric value for the key.  JSON carries neither NaN nor
 *                 +-inf: kdb_index_set_column refuses +-inf (KDB_ERR_INVALID, nothing written); kdb_index_set_column_dev cannot
 *                 look: the caller keeps +-inf out (an infinity would compare like any other double);
 *   KDB_COL_CODE  4 bytes per id, the caller's dictionary code of the string value (bools are "true" / "false"); 0 = no value.
 * kdb_index_set_column writes values[0..n) to ids first_id .. first_id+n-1 (1 <= first_id, first_id+n-1 <= capacity; ids above
 * count may be filled ahead of their rows).  The first upload of a slot allocates it filled with "absent"; later calls overwrite
 * their range and must name the same kind; n = 1 is VSetMetadata.  A writer in the sense of "Conventions".  kdb_index_reserve moves
 * live columns with the other arrays (absent tail; KDB_ERR_OOM leaves the index as it was), kdb_index_compress copies them device to
 * device to the new index, kdb_index_destroy frees them.  An index that never uploads a column allocates nothing.
 * kdb_index_column_info: *kind = 0 and *bytes = 0 for an empty slot.
 *
 * PROGRAMS.  A term compares one column with one constant:
 *   KDB_FOP_F64_EQ / LT / LE / GT / GE   column value <op> term.value, IEEE double compare: an absent value (NaN) never matches,
 *                                        -0.0 == 0.0 (Go's == and <, :1924, :1965-1989); a NaN term.value is refused;
 *   KDB_FOP_CODE_EQ                      column code == term.code (term.code != 0);
 *   KDB_FOP_NEVER                        false (a key nobody has a column for: `indexInv[key]` / `indexBTree[key]` missing).
 * A CLAUSE is a maximal run of terms chained by KDB_FT_OR_NEXT (set on every term but the clause's last); its value is the OR of
 * its terms, inverted when its FIRST term carries KDB_FT_NOT.  A BLOCK is a run of clauses ended by KDB_FT_END_BLOCK on its last
 * term (a term with END_BLOCK must not carry OR_NEXT): the AND of its clauses.  A PROGRAM is the OR of its blocks, ANDed with LIVE:
 * 1 <= id <= count and not deleted.  The last term of a program must carry END_BLOCK; 1..KDB_FILTER_MAX_TERMS terms per program,
 * 1..KDB_FILTER_MAX_PROGRAMS programs per call; a term's column must be a live slot of the kind its op reads.
 * The reference maps onto this as: `k = v` one clause of up to two alternatives -- F64_EQ if v parses as a number and k has a
 * numeric column, CODE_EQ if k has a code column and the dictionary knows v (the "lenient union" of :1933-1944), NEVER if
 * neither; `k != v` the same clause with NOT (live minus matched, :1998-2029); `<`, `<=`, `>`, `>=` one F64 term; AND within a block,
 * OR between blocks (:1785-1836).  The AND with live is exact: VDelete removes a node's metadata (pkg/engine/ops.go:428), so no index
 * of the reference names a deleted node, and `!=` starts from the non-deleted nodes (GetAllValidNodeIDs, hnsw_index.go:2884-2900).
 *
 * kdb_filter_eval_dev: `terms` and `prog_offsets` (P+1 entries, program p = terms[prog_offsets[p] .. prog_offsets[p+1])) are HOST
 * arrays, staged by the library like group_offsets of kdb_flat_scan_groups_dev.  d_lists receives P lists back to back,
 * words_per_list >= (count>>6)+1 uint64 words each; EVERY word is written: bit 0 clear, bits above count clear, padding words zero.
 * d_card: NULL or P uint32, the cardinality of each list (zeroed by the call, then one vector atomic add per (tile, program)).
 * Asynchronous on `stream`, per-stream scratch as for the other _dev calls: a search queued behind it on the same stream needs no
 * host synchronisation.  kdb_filter_eval is the host-output form (out_lists may be NULL when only out_card is wanted; not both).
 * One lane per id; a wave's ballot is a list word; a wave covers KDB_FILTER_TILE_WORDS (16) consecutive words so each list receives
 * contiguous runs of 128 bytes; the programs are taken KDB_FILTER_CHUNK (32) at a time and a column element is read once per (tile,
 * chunk); a program's terms are fetched once per pass of up to 16 words, not once per word (kdb_filter_plan.h). */
#define KDB_MAX_COLUMNS 16u
enum { KDB_COL_F64 = 1, KDB_COL_CODE = 2 };
enum { KDB_FOP_NEVER = 0, KDB_FOP_F64_EQ = 1, KDB_FOP_F64_LT = 2, KDB_FOP_F64_LE = 3, KDB_FOP_F64_GT = 4, KDB_FOP_F64_GE = 5, KDB_FOP_CODE_EQ = 6 };
enum { KDB_FT_OR_NEXT = 1, KDB_FT_NOT = 2, KDB_FT_END_BLOCK = 4 };
#define KDB_FILTER_MAX_TERMS 64u
#define KDB_FILTER_MAX_PROGRAMS 4096u
typedef struct { uint8_t op; uint8_t flags; uint16_t col; uint32_t code; double value; } kdb_filter_term; /* 16 bytes */
KDB_API int kdb_index_set_column(kdb_index *idx, uint32_t col, uint32_t kind, uint32_t first_id, uint32_t n, const void *values);
KDB_API int kdb_index_set_column_dev(kdb_index *idx, uint32_t col, uint32_t kind, uint32_t first_id, uint32_t n, const void *d_values);
KDB_API int kdb_index_drop_column(kdb_index *idx, uint32_t col);
KDB_API int kdb_index_column_info(kdb_index *idx, uint32_t col, uint32_t *kind, uint64_t *bytes);
KDB_API int kdb_filter_eval_dev(kdb_index *idx, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P,
                                uint64_t *d_lists, uint64_t words_per_list, uint32_t *d_card, void *stream);
KDB_API int kdb_filter_eval(kdb_index *idx, const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P,
                            uint64_t *out_lists, uint64_t words_per_list, uint32_t *out_card);

/* The filter STRING, host only (works without a GPU): the grammar of FindIDsByFilter restated, not improved.
 *   - the filter is trimmed; empty: KDB_ERR_INVALID "empty filter" (:1777-1780);
 *   - split on (?i)\s+OR\s+, each piece on (?i)\s+AND\s+ (core.go:44,48; leftmost matches, not quote-aware, as there); pieces are
 *     trimmed, empty ones skipped, a block left without clauses is skipped (:1828-1833);
 *   - the operator is the first of != <= >= = < > outside '...' / "..." (findFilterOperator, :1866-1897; compound ones first);
 *     none: KDB_ERR_INVALID "invalid filter format";
 *   - key = trimmed text before it; value = trimmed text after it, then stripped of every leading and trailing ' and " (:1908-1910);
 *   - is_numeric / number: strtod over the WHOLE value in the C locale.  Known differences from Go's strconv.ParseFloat: Go accepts
 *     underscores in hexadecimal mantissas and requires a p-exponent on them; both are refused / required here too by a syntax
 *     check, so what remains is strtod's "nan(chars)" form (refused) -- report others as bugs.  A value out of double range is not
 *     numeric, as ParseFloat's error makes it.  A range operator with a value that is not numeric: KDB_ERR_INVALID "value must be
 *     numeric"; a NaN operand with ANY operator: KDB_ERR_INVALID (the reference's B-tree walk returns every item for `< NaN`; not
 *     reproduced).  Whitespace is ASCII: \t \n \f \r and space split, those and \v trim.
 * CONTAINS(...) never reaches this function: the engine strips it first (parseHybridFilter).
 * Output: atoms in order; spans are byte offsets into `filter` as passed.  *n_atoms = the number of atoms the filter has; at most
 * `cap` are written (atoms may be NULL when cap is 0: count first, then fill).  The mirrors turn atoms into terms with their own
 * schema (key -> slots) and dictionary (kektordb_amd.index.compile_filter, kektor::hnsw::Index::CompileFilter). */
enum { KDB_FA_EQ = 0, KDB_FA_NE = 1, KDB_FA_LT = 2, KDB_FA_LE = 3, KDB_FA_GT = 4, KDB_FA_GE = 5 };
typedef struct {
    uint32_t key_off, key_len;   /* span of the key inside `filter` */
    uint32_t val_off, val_len;   /* span of the value, quotes stripped */
    uint8_t op;                  /* KDB_FA_* */
    uint8_t flags;               /* KDB_FT_END_BLOCK on the last atom of a block */
    uint8_t is_numeric;          /* the value parses as a float64: `number` holds it */
    uint8_t reserved[5];
    double number;
} kdb_filter_atom; /* 32 bytes */
KDB_API int kdb_filter_parse(const char *filter, kdb_filter_atom *atoms, uint32_t cap, uint32_t *n_atoms);

/* A filtered request as ONE call (host pointers; a composition like kdb_search_by_id): Engine.VSearch(index, query, k, filter)
 * from programs to answers.  B queries; P programs as for kdb_filter_eval; prog_of_query[b] = the program of query b or
 * KDB_NO_FILTER.  The call evaluates the programs, reads the P cardinalities back and routes PER PROGRAM by the rule of the
 * micro-batcher's takes_flat_scan (include/kektor_hip.hpp), unchanged:
 *   card == 0                                          route 2: out_count = 0, never scanned and never walked -- an empty list means
 *                                                      "no filter" to the exact scan (vector_index.go:130) but "no results" to the
 *                                                      engine (pkg/engine/ops.go:937-939);
 *   k <= 1024 and card < flat_selectivity * count      route 1: the exact scan (kdb_flat_scan_groups_dev for float32 / float16 at
 *                                                      k <= 128; one kdb_flat_scan_batch_dev per list for int8 and for k above 128,
 *                                                      which the grouped scan does not serve);
 *   otherwise, and KDB_NO_FILTER queries               route 0: kdb_search_batch_multi_dev.
 * Per query the answer -- ids, distance bits, count -- is bit for bit what kdb_search_batch (route 0) or kdb_flat_scan_batch
 * (route 1) returns for that query alone with that list; rows beyond the count hold what those calls leave there.
 * out_route: NULL or [B]; out_card: NULL or [P].  flags: KDB_SEARCH_NEEDS_REFINE, KDB_SEARCH_TIE_FLAG, KDB_SEARCH_HEAP_ORDER
 * (walk only).  flat_selectivity: 0 <= f <= 1 (0: nothing takes the scan).  Takes turns on the index's staging buffer like
 * kdb_search_by_id and is never combined with other callers' queries. */
KDB_API int kdb_search_filtered(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef,
                                const kdb_filter_term *terms, const uint32_t *prog_offsets, uint32_t P, const uint32_t *prog_of_query,
                                double flat_selectivity, uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count,
                                uint8_t *out_route, uint32_t *out_card);

/* B queries x C candidate ids each (ids[B][C], id 0 = skip -> +inf): raw accumulates out[B][C].   */
KDB_API int kdb_distance_batch(kdb_index *idx, const float *queries, uint32_t B, const uint32_t *ids, uint32_t C,
                       uint32_t flags, float *out);
KDB_API int kdb_distance_batch_dev(kdb_index *idx, const float *d_queries, uint32_t B, const uint32_t *d_ids,
                           uint32_t C, uint32_t flags, float *d_out, void *stream);

/* DB.Compress (pkg/core/core.go:1128-1290) on the device: a new index of `precision` (KDB_PREC_F16 / KDB_PREC_I8) from a
 * float32 one, rows never leaving HBM.  int8: Quantizer.Train (quantizer.go:49-135: strided sample, 99.9th percentile of
 * |v|, found exactly by a radix select), Quantize and the stored norms for every row; float16: RNE conversion.  The new
 * index keeps the float32 index's GRAPH (ids, links, deleted bits) unless KDB_COMPRESS_REBUILD_GRAPH asks the GPU builder
 * to re-insert every row with the new precision's distances (float16 squared L2; int8: the float64 cosine distance over
 * the quantised rows and stored norms), which is what the reference's AddBatch loop does (core.go:1236-1283).
 * Deleted nodes (the reference collects the vectors with IterateRaw, which skips them):
 *   - Train: the training set is the live rows (deleted bit clear) of 1..count in ascending id order; totalVectors, the
 *     10 000 threshold, targetSize, step and the break of quantizer.go:49-94 apply to that list.  No live row:
 *     KDB_ERR_STATE, as for an empty index (core.go:1168-1170), for both precisions;
 *   - rows: every row 1..count is converted or quantised and keeps its id, deleted or not (the mirror does not renumber);
 *   - deleted bits: both modes carry the source's deleted bits and their count into the new index, with or without a
 *     graph.  With KDB_COMPRESS_REBUILD_GRAPH the builder inserts every id 1..count and the deleted ones are marked
 *     deleted again afterwards -- the reference's state between Delete and Vacuum: walks may pass through them, no search
 *     or scan returns them, kdb_index_dead_link_scan counts them and kdb_index_vacuum removes them.
 * The source is left as it is; the caller owns *out (kdb_index_destroy).                                           */
#define KDB_COMPRESS_REBUILD_GRAPH 1u
KDB_API int kdb_index_compress(kdb_index *src, uint32_t precision, uint32_t flags, kdb_index **out);
KDB_API int kdb_index_get_quantizer(kdb_index *idx, float *abs_max);

/* GPU batched graph construction over rows 1..count already uploaded (efConstruction up to 512).  Deterministic: two builds
 * of the same rows with the same parameters give the same graph, list for list (a target that more new nodes ask for a
 * reverse link than it has request slots keeps the NEAREST requesters, not the first to arrive).                       */
KDB_API int kdb_index_build(kdb_index *idx, uint32_t count, const kdb_build_params *params);

/* AddBatch -> addBatchInternal (hnsw_index.go:1479-2088) for rows ALREADY uploaded at ids first_id .. first_id+n-1 (phase 0 /
 * 1B of the reference = kdb_index_upload_rows [+ norms]): phase 1 (every new node searches the graph as the batch found it),
 * phases 2-3 linked EXACTLY as the reference links them -- a request for all efConstruction candidates and a reverse request to
 * each of them, per target the sorted de-duplicated union, stored as it is (ascending ids) up to maxM entries, else scored,
 * sorted by (distance, id) and pruned by selectNeighbors -- and phase 4 (entry point / maxLevel).  The lists equal those of
 * the restated batch insert (oracle) link for link (tests/test_gpu_build.py); kdb_index_build is the FAST builder (its
 * linking differs by design).  levels[i] = len(Connections)-1 of node first_id+i as the caller drew it
 * (randomLevel, :2616-2625; capped at maxLevel+1 like there).  first_id = count+1 appends; first_id = count re-uses the last
 * slot, which is what the reference's id arithmetic does for the first batch after single Adds (:1620 vs :590).  The index
 * must hold a graph (the reference inserts its first efConstruction nodes one by one, :1505-1516: upload those).
 * Any number of nodes per call (the reference's Compress re-inserts 5000 at a time, core.go:1240): a target whose union of links
 * and requests outgrows LDS (4096 entries) is sorted in HBM scratch.  A re-used slot that is asked for links above its new
 * level GROWS, as the reference's node does (:2049-2053): afterwards its level is the highest one asked for.  efConstruction
 * up to 512.  A failure BEFORE the first link is written (arguments, allocations: everything is allocated up front) leaves the index as
 * it was; a device failure later restores count, entry point and levels on the host, but lists already rewritten -- the re-used
 * slot's among them -- stay as they are: upload the graph again.  float32 / float16 / int8.                              */
#define KDB_ADD_REFERENCE_LINKS 1u /* (the only linking this entry point has; accepted for symmetry with kdb_build_params.flags) */
KDB_API int kdb_index_add_batch(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels, uint32_t ef_construction,
                                uint32_t flags);

/* Add (pkg/core/hnsw/hnsw_index.go:472-809), the sequential single insert behind Engine.VAdd, on the device: afterwards the
 * index is the one that n consecutive calls of the reference's Add would leave, on a single goroutine, for rows ALREADY uploaded
 * at ids first_id .. first_id+n-1 in stored form (phase 0 / 1B = kdb_index_upload_rows [+ kdb_index_upload_norms], as for
 * kdb_index_add_batch).  Per new node x, in id order:
 *   - levels[i] = len(Connections)-1 as the caller drew it, capped at maxLevel+1 as randomLevel does (:2620-2623) -- the maxLevel
 *     THAT NODE sees, i.e. after the nodes before it in the same call;
 *   - empty graph (maxLevel -1; an index that holds rows and no graph at all counts as one: its rows are nodes without links):
 *     x becomes the entry point, maxLevel its level, no links (:657-670);
 *   - otherwise a descent with ef = 1 from maxLevel down to level(x)+1 (:685-690), then for l = min(level(x), maxLevel) .. 0:
 *     searchLayerUnlocked(stored row of x, ep, efC, l, nil, efC) -- deleted nodes are traversed, never returned; int8: the packed
 *     row with its norm (0 -> 1); selectNeighbors(candidates, mMax0 at level 0 else m) in the walk's ascending order becomes x's
 *     list (:711-722); each selected neighbour r, in that order (:725-783): a list of r at l shorter than maxM gains x at its
 *     end, a full one becomes selectNeighbors over its live existing links IN STORED ORDER, each at its node-to-node distance
 *     from r, followed by x at d(r, x) -- so a full list that is pruned drops its links to deleted nodes (:756-761); ep becomes
 *     the walk's nearest candidate (:786-788);
 *   - level(x) above the maxLevel x found: x becomes the entry point, maxLevel its level (:793-801).
 * Ties: selectNeighbors takes candidates "in the order given"; when a walk holds two different nodes at exactly equal distance
 * the reference's order depends on its heaps' history ("Equal distances" above).  The walk here orders such nodes by id, as the
 * builder and Refine do; a new node one of whose walks set the beam's tied bit is counted in tied_nodes, and its lists may differ
 * from the reference's only where those equal distances meet.  Every other node is the reference's, step for step (float32 /
 * float16: up to the summation order of the pair distances inside selectNeighbors; int8: bit for bit).
 * NOT mirrored:
 *   - a selected neighbour whose level is below l: the reference grows that node (:775-779).  It cannot occur on a graph that Add
 *     or AddBatch made (a level-l list holds only nodes of level >= l); it is skipped and counted in reverse_skipped;
 *   - training the quantizer on the first vector (:519-524): the caller sets the quantizer, as everywhere else in this ABI;
 *   - external ids, the arena, and concurrency between Adds.
 * first_id must equal count+1 (the slot re-use quirk belongs to kdb_index_add_batch alone), first_id+n-1 must stay within
 * capacity, levels must not be NULL: otherwise KDB_ERR_INVALID, nothing touched.  n == 0: KDB_OK.  ef_construction outside
 * 1..512, mMax0 > 64, rows beyond the limit of kdb_index_refine, or rows so long that a kernel's LDS (prune tiles + the walk's
 * row, beam and side list) would exceed the device's: KDB_ERR_UNSUPPORTED, nothing touched.  A writer exactly
 * like kdb_index_add_batch (same lock, same device-wide wait; the new nodes are registered as kdb_index_append_nodes registers
 * them).  The inserts are a chain on the index's stream -- two launches per (node, level), no host synchronisation per node, no
 * workgroup ever waits for another; everything is allocated before the first launch.  A device failure after the first launch
 * returns its error with count, entry point and maxLevel unchanged on the host, but lists already rewritten stay as they are:
 * upload the graph again.  Entry point, maxLevel and count change only after the final synchronisation succeeded.            */
typedef struct {
    uint32_t ef_construction; /* 0 = the index's; 1..512 */
    uint32_t flags;           /* 0 */
} kdb_add_params;
typedef struct {
    uint64_t nodes_added;
    uint64_t forward_lists;     /* (new node, level) lists written */
    uint64_t reverse_appended;  /* neighbour lists that had room: new id appended (:748-752) */
    uint64_t reverse_pruned;    /* neighbour lists that were full: selectNeighbors over old links + new node (:753-771) */
    uint64_t tied_nodes;        /* new nodes one of whose walks held two different nodes at equal distance (see "Ties") */
    uint64_t reverse_skipped;   /* selected neighbours whose level is below the link's level (see "NOT mirrored") */
    uint32_t entry;             /* after the call */
    int32_t  max_level;         /* after the call */
} kdb_add_stats;
KDB_API int kdb_index_add(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels,
                          const kdb_add_params *params, kdb_add_stats *out /* may be NULL */);

/* GraphOptimizer.Refine (pkg/core/hnsw/optimizer.go:288-464; MaintenanceRun("refine"), RunTurboRefine :679-719) on the device:
 * the neighbour lists of the selected nodes are computed again against the graph AS THE CALL FOUND IT and replace the stored
 * ones.  ids == NULL: every live node 1..count (what Refine() does as written: its collection loop, :340-346, ignores the
 * cursor range); otherwise n ids in host memory -- 0 or an id above count: KDB_ERR_INVALID, nothing touched; deleted ids are
 * skipped (:341); an id named twice is refined once.  Per node x and level l <= level(x), computeNewConnections (:466-560):
 *   1. searchLayer(stored row of x, the index's entry point, ef, l) started ON level l (no descent), visited set per layer;
 *      deleted nodes are traversed, never returned; int8: the packed row with its stored norm (0 -> 1);
 *   2. the current neighbours of x at l that the walk did not return, exist and are not deleted, with their node-to-node distance;
 *   3. without x itself;   4. sorted by (distance, id) -- the reference's sort.Slice leaves equal distances undefined; this is
 *      the tie rule of kdb_index_add_batch;   5. selectNeighbors(.., mMax0 at level 0, m above) replaces the list (possibly empty).
 * Links are one-directional: no reverse requests.  Entry point, maxLevel, levels and deleted bits do not change.
 * SNAPSHOT: the new lists are staged in device scratch and committed by one kernel after every selected node has been
 * searched and selected (phase 1 / phase 2 of the reference, :354-461), so a node never sees another node's new list and the
 * result does not depend on chunk_nodes.  Everything is allocated up front: a failure before the commit leaves the graph as
 * it was.  Vacuum's reconnectNode loop (:200-221) is sequential -- each repair walks lists earlier repairs rewrote -- and is
 * NOT mirrored; a host that wants repair after deletes calls kdb_index_vacuum, which finds the nodes that hold a dead link
 * on the device (kdb_index_dead_link_scan hands out their ids) and re-links them this way.
 * float32 / float16 / int8, ef up to 512, mMax0 <= 64.  A writer like kdb_index_add_batch.                                 */
typedef struct {
    uint32_t ef_construction; /* 0 = the index's; 1..512 */
    uint32_t flags;           /* 0 */
    uint32_t chunk_nodes;     /* nodes searched per scratch chunk (bounds the candidate arrays); 0 = library default (65536) */
} kdb_refine_params;
typedef struct {
    uint64_t nodes_refined;      /* live nodes selected, each counted once */
    uint64_t lists_written;      /* (node, level) lists replaced */
    uint64_t lists_changed;      /* ... of which at least one stored word differs from before */
    uint64_t dead_links_dropped; /* entries of the replaced lists that named a deleted node (or no node) */
} kdb_refine_stats;
KDB_API int kdb_index_refine(kdb_index *idx, const uint32_t *ids, uint32_t n, const kdb_refine_params *params, kdb_refine_stats *out);

/* GraphOptimizer.Vacuum (pkg/core/hnsw/optimizer.go:133-277; MaintenanceRun("vacuum"), hnsw_index.go:976) on the device: what
 * kdb_index_mark_deleted left behind is repaired and cleared.  A writer like kdb_index_refine (same lock, same device-wide wait).
 *   1. D = the ids 1..count whose deleted bit is set when the call starts (deletedSet, :143-148).  D empty (:151), no graph or
 *      entry 0: KDB_OK, ALL-ZERO statistics (entry and max_level fields too), nothing touched.
 *   2. R = every live node with a dead link on one of its levels 0..min(level(x), maxLevel), ascending (:165-193).  A dead link
 *      is a non-zero adjacency word that names an id of D or an id outside 1..count -- what kdb_refine_stats.dead_links_dropped
 *      counts; the zero words behind a list's end are padding.  One streaming kernel over the adjacency writes a flag bitmap.
 *   3. Every node of R is re-linked exactly as kdb_index_refine(ids = R) does it, SNAPSHOT semantics included: under a writer's
 *      lock ignoreSet equals the deleted bits, and reconnectNode (:565-674) is step for step computeNewConnections (:466-560).
 *      The reference's loop (:200-221) commits each node before the next one walks; that ORDER IS NOT MIRRORED, for the reason
 *      given above for Refine: every repair would walk lists earlier repairs rewrote, one node at a time.  The walks start at
 *      the entry point as the call found it, dead or not.
 *   4. Entry point (:232-250), after the commit: a live entry is never changed.  A deleted one is replaced by the LOWEST LIVE ID
 *      and maxLevel becomes THAT node's level (the reference's rule as written: on a graph of any size it almost always elects
 *      a level-0 node and so gives the upper layers up).  KDB_VACUUM_ELECT_TOP_LEVEL: the live node of the highest level
 *      instead, the lowest id among equals, maxLevel = that level.  No live node: entry 0, maxLevel -1 -- from then on the
 *      index answers like one whose uploaded graph has max_level -1.
 *   5. Cleanup (:256-273), for every id of D: its lists on every level become empty (zero words), its stored row and its row of
 *      the half-precision ranking copy (if there is one) are zeroed.  Its deleted bit STAYS SET: that is the mirror's "no node
 *      here" (nodes[id] = nil) -- the exact scan keeps skipping the row, kdb_index_refine / kdb_index_add_batch keep treating
 *      the id as not linkable.  Levels, count, capacity, the int8 norms and the number of deleted nodes do not change; ids are
 *      not reused and no memory is given back (nodeCounter never goes back in the reference either).
 * Failure: the census is read-only and its scratch is allocated before it; the repair's workspace (its size depends on |R|) is
 * allocated before the first repair launch; a failure before the commit kernel leaves the graph as it was.  Commit, cleanup and
 * the entry / maxLevel update follow the last check with no allocation in between, and entry / maxLevel change only after the
 * final synchronisation succeeded.  A second call right after the first changes no adjacency word, no row and no header field
 * (nodes_repaired 0).  ef_construction outside 1..512: KDB_ERR_UNSUPPORTED, nothing touched.                               */
#define KDB_VACUUM_ELECT_TOP_LEVEL 1u
typedef struct {
    uint32_t ef_construction; /* 0 = the index's; 1..512 */
    uint32_t flags;           /* KDB_VACUUM_ELECT_TOP_LEVEL */
    uint32_t chunk_nodes;     /* as kdb_refine_params */
} kdb_vacuum_params;
typedef struct {
    uint64_t dead_nodes;         /* |D| */
    uint64_t nodes_repaired;     /* |R| */
    uint64_t lists_written;      /* (node, level) lists replaced */
    uint64_t lists_changed;      /* ... of which at least one stored word differs from before */
    uint64_t dead_links_dropped; /* as kdb_refine_stats, for R */
    uint64_t dead_links_found;   /* counted by the scan: equals dead_links_dropped (the nodes that hold dead links are the nodes repaired) */
    uint32_t entry;              /* entry after the call */
    int32_t  max_level;          /* max_level after the call */
    uint32_t entry_changed;      /* 1: the entry the call found was deleted and has been replaced */
    uint32_t reserved;
} kdb_vacuum_stats;
KDB_API int kdb_index_vacuum(kdb_index *idx, const kdb_vacuum_params *params, kdb_vacuum_stats *out);

/* Read-only: the census that step 2 makes.  Ascending ids of R into out_ids (host, `cap` entries; NULL = counts
 * only); *n_nodes = |R| whatever cap is; *n_dead_links = total dead links in live nodes' lists; *n_dead = |D|.  The numbers a
 * host's maintenance policy (RunCycle's thresholds, optimizer.go) needs without downloading the graph.  No graph: all zero.  */
KDB_API int kdb_index_dead_link_scan(kdb_index *idx, uint32_t *out_ids, uint32_t cap, uint32_t *n_nodes, uint64_t *n_dead_links,
                                     uint64_t *n_dead);

/* TEST HOOK -- selectNeighbors (hnsw_index.go:2629-2701) exactly as the GPU builder runs it (build_select_kernel's
 * workgroup routine), on caller-supplied candidate lists: list t holds cand_cnt[t] <= stride <= 576 entries at
 * cand_ids / cand_keys + t*stride, ids of rows already uploaded, keys = distance of the candidate to the centre in the
 * library's ordering form, ASCENDING: FLOATS for float32 / float16 indexes (squared L2; MINUS the dot product for cosine),
 * DOUBLES for int8 indexes (the reference's float64 cosine distance, hnsw_index.go:317-336).  out_ids: [n_lists][maxm],
 * 0-filled behind out_cnt[t].  maxm <= 64.  Host pointers.  Exists so that the parity suite can hand identical lists to
 * this and to the oracle's select_neighbors; the shim has no use for it.                                          */
KDB_API int kdb_test_select_neighbors(kdb_index *idx, uint32_t n_lists, uint32_t stride, const uint32_t *cand_ids,
                                      const void *cand_keys, const uint32_t *cand_cnt, uint32_t maxm, uint32_t *out_ids,
                                      uint32_t *out_cnt);

/* Shard merge: G per-shard results for B queries -> global top-k.  in_ids/in_dist: [G][B][k],
 * in_count: [G][B]; id_base: NULL or [G] offsets added to shard g's (local, 1-based) ids so that
 * global id = id_base[g] + local id (shard g owns the contiguous id range that starts at id_base[g]+1).
 * Ordering: ascending raw L2 sum, or descending dot for cosine/f32, ties by global id.
 * A shard's count may carry KDB_COUNT_TIED (it searched with KDB_SEARCH_TIE_FLAG): the length of its list is
 * in_count & KDB_COUNT_MASK, and out_count[b] carries the bit when the count of ANY shard did for query b (every
 * merge entry point below does the same).  Behind out_count[b] & KDB_COUNT_MASK: id 0, distance +Inf.
 * kdb_merge_topk takes host pointers (host-side glue of the shim); *_dev device pointers.           */
KDB_API int kdb_merge_topk(uint32_t metric, uint32_t precision, uint32_t G, uint32_t B, uint32_t k,
                   const uint32_t *in_ids, const float *in_dist, const uint32_t *in_count,
                   const uint32_t *id_base, uint32_t *out_ids, float *out_dist, uint32_t *out_count);
/* Host merge for int8 shards: float64 distances in and out (the reference's own order, hnsw_index.go:2429-2454), (distance, global id). */
KDB_API int kdb_merge_topk_f64(uint32_t G, uint32_t B, uint32_t k, const uint32_t *in_ids, const double *in_dist, const uint32_t *in_count,
                               const uint32_t *id_base, uint32_t *out_ids, double *out_dist, uint32_t *out_count);
KDB_API int kdb_merge_topk_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_in_ids,
                       const float *d_in_dist, const uint32_t *d_in_count, const uint32_t *d_id_base,
                       uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, void *stream);
/* The same merge over the PACKED per-shard block that ONE all-gather delivers (one collective per query
 * batch instead of three): shard g's block starts at d_packed + g*stride_words (32-bit words, stride >=
 * 2*B*k + B) and holds ids[B][k] | raw distances[B][k] (f32 bits) | count[B].                         */
KDB_API int kdb_merge_topk_packed_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_packed,
                              uint64_t stride_words, const uint32_t *d_id_base, uint32_t *d_out_ids,
                              float *d_out_dist, uint32_t *d_out_count, void *stream);

/* The same for int8 shards, whose distances the reference computes and ORDERS as float64 (hnsw_index.go:2429-2454): shard
 * g's block holds dist64[B][k] (doubles, as KDB_SEARCH_DIST_F64 writes them) | ids[B][k] | count[B]; stride_words even and
 * >= 3*B*k + B; d_out_dist receives doubles.  (A merge over floats would rank two distinct doubles that round to one float
 * by id.)                                                                                                        */
KDB_API int kdb_merge_topk_packed_f64_dev(kdb_index *idx, uint32_t G, uint32_t B, uint32_t k, const uint32_t *d_packed,
                                          uint64_t stride_words, const uint32_t *d_id_base, uint32_t *d_out_ids,
                                          double *d_out_dist, uint32_t *d_out_count, void *stream);

/* ---- the id-range shards of one node behind one handle (single-process callers: the Go shim) ------------------------
 * shards[g]: an index created on its device (kdb_index_desc.device_id) that owns the global ids id_base[g]+1 ...
 * id_base[g]+count_g (local id i <-> global id id_base[g]+i); bases ascend, shards of one device are consecutive and
 * every device holds the same number.  The cluster borrows the handles (destroy it before them).
 * kdb_sharded_search_batch = SearchWithScores over the whole corpus: the batch visits every shard (each on its own
 * GPU), ONE RCCL all-gather of the per-shard top-k blocks over xGMI, merge under the total order (distance, global id).
 * allow_bits: NULL or a dense bitset over GLOBAL ids (allow_words uint64 words), sliced per shard by the library; the
 * per-shard semantics are those of kdb_search_batch (a list that allows nothing in a shard yields nothing from it).
 * Host pointers; ids returned are global.  kdb_sharded_flat_scan_batch: the exact scan, same exchange; as for
 * kdb_flat_scan_batch a list that names NO id at all means no filter, but a list that names ids, none of them in shard g,
 * brings nothing back from shard g (the emptiness that counts is the whole list's, never a slice's).
 * flags go to every shard as they are: with KDB_SEARCH_TIE_FLAG out_count[b] carries KDB_COUNT_TIED when the walk of ANY
 * shard did for query b (mask with KDB_COUNT_MASK); KDB_SEARCH_HEAP_ORDER re-walks the tied queries shard by shard.
 * RCCL (librccl.so.1) is loaded at the first kdb_cluster_create.                                                 */
typedef struct kdb_cluster kdb_cluster;
KDB_API int kdb_cluster_create(kdb_index *const *shards, const uint32_t *id_base, uint32_t n_shards, kdb_cluster **out);
KDB_API void kdb_cluster_destroy(kdb_cluster *c);
KDB_API int kdb_cluster_info(const kdb_cluster *c, uint32_t *n_shards, uint32_t *n_devices, uint32_t *shards_per_device);
KDB_API int kdb_sharded_search_batch(kdb_cluster *c, const float *queries, uint32_t B, uint32_t k, uint32_t ef,
                                     const uint64_t *allow_bits, uint64_t allow_words, uint32_t flags, uint32_t *out_ids,
                                     float *out_dist, uint32_t *out_count);
KDB_API int kdb_sharded_flat_scan_batch(kdb_cluster *c, const float *queries, uint32_t B, uint32_t k,
                                        const uint64_t *allow_bits, uint64_t allow_words, uint32_t flags, uint32_t *out_ids,
                                        float *out_dist, uint32_t *out_count);
/* Failure model of a cluster: an error BEFORE anything was queued (bad argument, allocation) or BETWEEN two collectives (a
 * shard's search refuses its arguments) leaves the handle usable.  A failure INSIDE an RCCL group -- a collective queued on
 * some devices and not on others, after which the next collective would wait for ever -- POISONS the handle: every
 * communicator is aborted (ncclCommAbort), the failing call returns its error, and every later call returns KDB_ERR_STATE
 * at once (never a hang); destroy the cluster and create a new one.  kdb_cluster_comm_info: the number of ranks the
 * communicator itself reports (ncclCommCount: the devices ncclCommInitAll joined) and whether the handle is poisoned.  */
KDB_API int kdb_cluster_comm_info(const kdb_cluster *c, uint32_t *ranks_in_communicator, uint32_t *poisoned);
/* TEST HOOK -- the next sharded call fails inside the RCCL group of stage 1 (query broadcast) or 2 (all-gather), with the
 * collective queued on every device but the last: exercises the poisoning path without broken hardware.  0 disarms.  */
KDB_API int kdb_cluster_debug_fail_next(kdb_cluster *c, uint32_t stage);

/* MEASUREMENT HOOKS (probe.hip) -- what this device delivers on the two access patterns of the hot path, on the index's own row
 * array: a uniform random whole-row gather (16 lanes per row, best of four launch shapes) and one coalesced streaming pass.
 * which: 0 = the stored rows, 1 = the half-precision ranking copy, 2 (kdb_probe_gather only) = the high walk plane of a float32
 * cosine index of 768 columns (1536-byte rows; KDB_ERR_UNSUPPORTED until a planes walk has made the planes).
 * *ms = duration of the best launch, *bytes = what it read.
 * bench.py reports its roofline fractions against these beside the nominal HBM peak.  Blocking.              */
KDB_API int kdb_probe_gather(kdb_index *idx, int which, uint64_t n_reads, float *ms, uint64_t *bytes);
KDB_API int kdb_probe_stream(kdb_index *idx, int which, float *ms, uint64_t *bytes);
/* TEST HOOK (probe.hip): fills the LDS of every CU with `pattern` (0 = a pseudo-random word per address) on the index's stream and
 * waits.  LDS keeps what the previous kernel left; called between launches it makes a kernel that reads LDS it never wrote show
 * (the parity tests of the exact scan use it: a race of that kind survived the suite until HBM and LDS were poisoned).  Blocking. */
KDB_API int kdb_probe_poison_lds(kdb_index *idx, uint32_t pattern);
/* TEST HOOK: which kernel the last `last_n` (<= 64) launches ran, oldest first -- the same launches, in the same order, as
 * kdb_get_launch_stats.  out[last_n][KDB_LAUNCH_SHAPE_WORDS], all zero for a launch that was not a graph search:
 *   [0] 1 = a graph search                     [1] precision   [2] metric
 *   [3] row-width unroll NCH (ld = 64 * NCH; 0 = any width)     [4] beam slots BS (1 / 2 / 4 in registers, 0 = the LDS beam)
 *   [5] words of the LDS visited hash (0 = the HBM bitset alone) [6] waves per query (1 / 2 / 4)
 *   [7] 1 = the planes kernel                  [8] 1 = heap-order pass armed (KDB_SEARCH_HEAP_ORDER)
 *   [9] that pass's NCH   [10] its LDS hash words   [11] 1 = its result heap in registers   [12] 1 = it runs beside the search kernel
 *   [13] workgroups of the search kernel       [14] its LDS bytes per workgroup      [15] queries
 * Host-side bookkeeping only: the tests use it to assert that a case reached the template instantiation it was written for.   */
#define KDB_LAUNCH_SHAPE_WORDS 16u
KDB_API int kdb_probe_launch_shape(kdb_index *idx, uint32_t last_n, uint32_t *out);
/* TEST HOOK: the plan of the heap-order pass (KDB_SEARCH_HEAP_ORDER) that a search of B queries with this k and efSearch would
 * launch on the index as it stands.  out[KDB_HEAP_PLAN_WORDS]:
 *   [0] words of the LDS visited hash (0 = the HBM bitset alone)   [1] 1 = the result heap in registers
 *   [2] candidate-heap entries kept in LDS (nl_c)                  [3] ... and in all, LDS + HBM tail (cap_c): a walk whose
 *       candidate heap outgrows it keeps the fast walk's answer and its tie bit and is counted in n_dropped
 *   [4] LDS bytes per workgroup   [5] workgroups of a pass behind the search kernel   [6] bytes of all their HBM tails
 * Launches nothing.  The tests take their thresholds from it: which walks reach the tail, which overflow.                    */
#define KDB_HEAP_PLAN_WORDS 7u
KDB_API int kdb_probe_heap_plan(kdb_index *idx, uint32_t k, uint32_t ef, uint32_t B, uint64_t *out);

KDB_API int kdb_get_counters(kdb_index *idx, kdb_counters *out);
/* Statistics of the last `last_n` (<= 64) search / flat-scan / distance launches, oldest first: each
 * launch records its own HIP event pair on the launch stream and its own counter slot, so a timed
 * loop can run unsynchronised and be read afterwards.                                             */
KDB_API int kdb_get_launch_stats(kdb_index *idx, uint32_t last_n, kdb_counters *out);
/* The graph-search launches are bracketed by two HIP events (kdb_counters.last_kernel_ms).  on = 0 drops them: two packets
 * less in the queue per call (9 us of a small-batch call); the counters stay, last_kernel_ms reads 0.  Default: on. */
KDB_API int kdb_index_set_launch_timing(kdb_index *idx, int on);
/* Statistics of the concurrent host-pointer calls (see "Conventions"), out[10]: [0] launches that left through a slot, [1] the calls
 * they carried ([1] / [0] = callers per launch), [2] the largest number of queries one launch carried, [3] the number of slots of
 * this index; combined searches only: [4] calls, [5] nanoseconds they waited for their group's launch (sum), [6] nanoseconds from
 * the launch until the caller saw its own answer complete (sum), [7] nanoseconds threads spent launching groups (sum), [8] timed
 * naps of the waiting callers, [9] the running estimate of a call's wait (ns) that sizes the first nap. */
KDB_API int kdb_index_caller_stats(kdb_index *idx, uint64_t *out);
/* Block until all work queued on the index's internal stream has finished. */
KDB_API int kdb_index_sync(kdb_index *idx);

#ifdef __cplusplus
}
#endif
#endif /* KEKTOR_HIP_H */
