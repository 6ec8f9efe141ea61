// kdb_api.hip -- host side of the C ABI declared in include/kektor_hip.h.
// Memory layout in HBM (one index):
//   rows     (cap+1) x ld elements, row-major, row 0 and the pad columns zero  (arena row layout,
//            pkg/storage/mmap/arena.go:403-404, with the 64-byte chunk headers stripped)
//   adj0     (cap+1) x mMax0 uint32, level-0 neighbour ids in stored order, 0 = empty slot
//   adj_up   upper-level pool, m uint32 per (node, level>=1) slot; up_idx[id] = first slot of a node
//   levels   (cap+1) uint8;  deleted: bitset;  norms: (cap+1) f32 (int8 norms / L2 row norms)
//   visited  one bitset of (cap>>5)+1 words per resident search wave
#include "kdb_internal.h"
#include "kdb_host.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

void kdb_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *kdb_last_error(void) { return g_err; }

// Kernels of different streams run side by side only on different HARDWARE queues, and the runtime gives a process four unless
// GPU_MAX_HW_QUEUES says otherwise (measured: scripts/micro/launch_rate.hip -- 8 threads with a 150 us kernel each reach 25.6 k
// launches/s on four queues, 42.7 k on eight).  The library does NOT touch the environment (round 5 did, from a constructor: a
// process-wide side effect, and setenv is not thread-safe under a dlopen from a threaded host): the host that wants eight queues
// sets the variable before the runtime starts -- INTEGRATION.md ("Contract notes").  Nothing in this repository sets it: not the
// Python package, not bench.py, not the tests.
extern "C" int kdb_abi_version(void) { return KDB_ABI_VERSION; }

extern "C" int kdb_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int check_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        kdb_set_error("no HIP device visible: libkektor_hip has no CPU fallback");
        return KDB_ERR_NO_DEVICE;
    }
    if (dev < 0 || dev >= n) {
        kdb_set_error("device_id %d out of range (0..%d)", dev, n - 1);
        return KDB_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    KDB_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        kdb_set_error("device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
        return KDB_ERR_NO_DEVICE;
    }
    return KDB_OK;
}

KdbView kdb_make_view(const kdb_index *idx) {
    KdbView v;
    v.rows = idx->d_rows;
    v.norms = idx->d_norms;
    v.adj0 = idx->d_adj0;
    v.adj_up = idx->d_adj_up;
    v.up_idx = idx->d_up_idx;
    v.adj_up_slot = nullptr; // kdb_search_dev_locked hands the table over once it is known to be current
    v.levels = idx->d_levels;
    v.deleted = idx->d_deleted;
    v.dim = idx->desc.dim;
    v.ld = idx->ld;
    v.deg0 = idx->deg0;
    v.deg_up = idx->deg_up;
    v.count = idx->count;
    v.entry = idx->entry;
    v.max_level = idx->max_level;
    v.metric = idx->desc.metric;
    v.precision = idx->desc.precision;
    v.vis_words = (idx->cap >> 5) + 1;
    v.vis_words = (v.vis_words + 3u) & ~3u;
    v.q_absmax = idx->absmax;
    v.has_deleted = idx->n_deleted > 0 ? 1u : 0u;
    return v;
}

// Scratch grows in powers of two while small (batches of concurrent callers come in every size: a re-allocation is a device-wide
// synchronisation), by a quarter beyond
static size_t grown(size_t bytes) {
    if (bytes >= ((size_t)32 << 20)) return bytes + bytes / 4;
    size_t w = (size_t)64 << 10;
    while (w < bytes) w <<= 1;
    return w;
}

// One routine grows every device buffer of the host API: nothing to do while *p holds `need` units; else the old buffer goes (behind
// a device-wide synchronisation) and `want` units of `unit` bytes are allocated.  Under idx->mu.  The callers state their growth rule.
template <typename P, typename N>
static int ensure_buf(kdb_index *idx, P **p, N *have, size_t need, size_t want, size_t unit = 1) {
    if (*have >= need) return KDB_OK;
    if (*p) {
        kdb_close_session(idx); // (an open launch would sit out its 0.5 s device-side safety under this synchronisation: closing it needs idx->mu, which this thread holds)
        KDB_HIP(hipDeviceSynchronize()); // growth is rare; work of callers' streams may still use the old buffer
        KDB_HIP(hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    KDB_HIP(hipMalloc(p, want * unit));
    *have = (N)want;
    return KDB_OK;
}

// the scratch lane's buffers (kdb_lane; the call has taken its lane: kdb_lane_acquire) ...
int kdb_ensure_scratch(kdb_index *idx, size_t bytes) { return ensure_buf(idx, &kdb_cur(idx).d_scratch, &kdb_cur(idx).scratch_bytes, bytes, grown(bytes)); }
int kdb_ensure_tie_scratch(kdb_index *idx, size_t bytes) { return ensure_buf(idx, &kdb_cur(idx).d_tie, &kdb_cur(idx).tie_bytes, bytes, grown(bytes)); }
int kdb_ensure_qbuf(kdb_index *idx, size_t bytes) { return ensure_buf(idx, &kdb_cur(idx).d_qbuf, &kdb_cur(idx).qbuf_bytes, bytes, grown(bytes)); }
int kdb_ensure_byid(kdb_index *idx, size_t bytes) { return ensure_buf(idx, &kdb_cur(idx).d_byid, &kdb_cur(idx).byid_bytes, bytes, grown(bytes)); }
int kdb_ensure_group_entries(kdb_index *idx, uint32_t n) { return ensure_buf(idx, &kdb_cur(idx).d_gentry, &kdb_cur(idx).gentry_cap, n, (size_t)n + n / 4 + 64, 4); }
// ... and the staging buffer of the turns (HostTurn), which belongs to the index
int kdb_ensure_iobuf(kdb_index *idx, size_t bytes) { return ensure_buf(idx, &idx->d_iobuf, &idx->iobuf_bytes, bytes, bytes + bytes / 4); }

// A call's lane: the one last used on its stream, else the least recently used one -- behind a device-side wait for that lane's last
// call.  The lane's buffers are stored once, in the lane: kdb_cur(idx) names them until the next acquire.
int kdb_lane_acquire(kdb_index *idx, hipStream_t s) {
    int pick = -1;
    for (int i = 0; i < KDB_LANES; i++)
        if (idx->lanes[i].used && idx->lanes[i].last_stream == s) pick = i; // same stream: ordered already
    if (pick < 0) {
        pick = 0;
        for (int i = 1; i < KDB_LANES; i++)
            if (idx->lanes[i].last_use < idx->lanes[pick].last_use) pick = i;
        if (idx->lanes[pick].used) KDB_HIP(hipStreamWaitEvent(s, idx->lanes[pick].done, 0));
    }
    idx->cur_lane = pick;
    return KDB_OK;
}

int kdb_lane_release(kdb_index *idx, hipStream_t s) {
    kdb_lane &l = kdb_cur(idx);
    l.last_stream = s;
    l.used = true;
    l.last_use = ++idx->lane_clock;
    KDB_HIP(hipEventRecord(l.done, s));
    return KDB_OK;
}

int kdb_ensure_visited(kdb_index *idx, uint32_t slots, hipStream_t s) {
    kdb_lane &l = kdb_cur(idx);
    if (l.vis_slots >= slots) return KDB_OK;
    if (l.d_visited) {
        kdb_close_session(idx); // (an open launch would sit out its 0.5 s device-side safety under this synchronisation: closing it needs idx->mu, which this thread holds)
        KDB_HIP(hipDeviceSynchronize()); // growth is rare; work of callers' streams may still use the old buffer
        KDB_HIP(hipFree(l.d_visited));
        l.d_visited = nullptr;
        l.vis_slots = 0;
    }
    uint32_t words = (((idx->cap >> 5) + 1) + 3u) & ~3u;
    // growth in powers of two while that costs less than 1 GiB (batches of concurrent callers come in every size: no re-allocation --
    // a device-wide synchronisation -- per new size), exact beyond
    uint32_t want = 16u;
    while (want < slots) want *= 2u;
    if ((size_t)want * words * 4 > ((size_t)1 << 30)) want = slots;
    slots = want;
    KDB_HIP(hipMalloc(&l.d_visited, (size_t)slots * words * 4));
    KDB_HIP(hipMemsetAsync(l.d_visited, 0, (size_t)slots * words * 4, s)); // on the stream the walk will run on
    l.vis_slots = slots;
    return KDB_OK;
}

unsigned long long *kdb_stats_begin(kdb_index *idx, int kind, uint32_t B, uint32_t C) {
    const uint32_t slot = (uint32_t)(idx->launch_seq % kdb_index::RING);
    idx->launch_seq++;
    idx->ev0 = idx->ring_ev0[slot];
    idx->ev1 = idx->ring_ev1[slot];
    idx->ring_kind[slot] = kind;
    idx->ring_timed[slot] = kind != 1 || idx->time_launches;
    idx->ring_B[slot] = B;
    idx->ring_C[slot] = C;
    memset(idx->ring_shape[slot], 0, sizeof idx->ring_shape[slot]);
    idx->last_kind = kind;
    idx->last_B = B;
    idx->last_C = C;
    return idx->d_ctr + (size_t)slot * 4; // [0] n_dist / rows scanned, [1] n_hops, [2] work counter of the launch
}

static int stats_of_slot(kdb_index *idx, uint32_t slot, kdb_counters *out) {
    unsigned long long c[4] = {0, 0, 0, 0};
    float ms = 0.f;
    if (!idx->ring_timed[slot]) {
        KDB_HIP(hipDeviceSynchronize()); // no event to wait for: the launch may still be running on a stream of the caller
    } else if (hipEventSynchronize(idx->ring_ev1[slot]) != hipSuccess ||
               hipEventElapsedTime(&ms, idx->ring_ev0[slot], idx->ring_ev1[slot]) != hipSuccess) {
        ms = 0.f;
    }
    KDB_HIP(hipMemcpy(c, idx->d_ctr + (size_t)slot * 4, 32, hipMemcpyDeviceToHost));
    kdb_counters r{};
    r.last_kernel_ms = ms;
    const uint64_t row_bytes = (uint64_t)idx->desc.dim * idx->elem;
    const int kind = idx->ring_kind[slot];
    if (kind == 1) { // n_dist*(dim*elem) + n_hops*(deg_cap*4) + n_dist*4
        r.n_dist = c[0];
        r.n_hops = c[1];
        r.n_dropped = c[3];
        r.n_tied = c[2];
        r.bytes = c[0] * row_bytes + c[1] * (uint64_t)idx->deg0 * 4 + c[0] * 4;
    } else if (kind == 2) { // N_scanned*dim*elem + B*dim*elem + B*k*8 (k*8 added by the caller)
        r.n_dist = c[0] * (uint64_t)idx->ring_B[slot]; // rows scanned (after filter / deletes) x queries
        r.n_hops = c[1];                               // f16-ranked scan: queries settled by the exact pass
        r.n_dropped = c[2];                            // big-tile kernel under KDB_FB_DBG=32 (measurement build): wave cycles in
        r.bytes = c[0] * row_bytes + (uint64_t)idx->ring_B[slot] * row_bytes;
        if (c[3]) r.bytes = c[3];                      // the selection phases / in the compaction rounds
    } else if (kind == 3) {
        r.n_dist = (uint64_t)idx->ring_B[slot] * idx->ring_C[slot];
        r.bytes = r.n_dist * row_bytes + r.n_dist * 8 + (uint64_t)idx->ring_B[slot] * row_bytes;
    }
    *out = r;
    return KDB_OK;
}

extern "C" int kdb_get_counters(kdb_index *idx, kdb_counters *out) {
    KDB_CHECK_IDX(idx);
    if (!out) return KDB_ERR_INVALID;
    std::lock_guard<std::mutex> lk(idx->mu);
    KDB_HIP(hipSetDevice(idx->device));
    if (idx->launch_seq == 0) {
        *out = kdb_counters{};
        return KDB_OK;
    }
    return stats_of_slot(idx, (uint32_t)((idx->launch_seq - 1) % kdb_index::RING), out);
}

extern "C" int kdb_get_launch_stats(kdb_index *idx, uint32_t last_n, kdb_counters *out) {
    KDB_CHECK_IDX(idx);
    if (!out || last_n == 0 || last_n > kdb_index::RING || last_n > idx->launch_seq) {
        kdb_set_error("get_launch_stats: last_n must be 1..min(%u, launches so far)", kdb_index::RING);
        return KDB_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    KDB_HIP(hipSetDevice(idx->device));
    for (uint32_t i = 0; i < last_n; i++) {
        const uint64_t seq = idx->launch_seq - last_n + i;
        int rc = stats_of_slot(idx, (uint32_t)(seq % kdb_index::RING), out + i);
        if (rc) return rc;
    }
    return KDB_OK;
}

// TEST HOOK: the launch shapes of the same slots (host words, written under mu by the launch itself: nothing to wait for)
extern "C" int kdb_probe_launch_shape(kdb_index *idx, uint32_t last_n, uint32_t *out) {
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!out || last_n == 0 || last_n > kdb_index::RING || last_n > idx->launch_seq) {
        kdb_set_error("probe_launch_shape: last_n must be 1..min(%u, launches so far)", kdb_index::RING);
        return KDB_ERR_INVALID;
    }
    for (uint32_t i = 0; i < last_n; i++) {
        const uint64_t seq = idx->launch_seq - last_n + i;
        memcpy(out + (size_t)i * KDB_LAUNCH_SHAPE_WORDS, idx->ring_shape[seq % kdb_index::RING], sizeof idx->ring_shape[0]);
    }
    return KDB_OK;
}

// TEST HOOK: the plan of the heap-order pass a search of B queries with (k, ef) would launch on this index (kdb_heap_walk_plan)
extern "C" int kdb_probe_heap_plan(kdb_index *idx, uint32_t k, uint32_t ef, uint32_t B, uint64_t *out) {
    KDB_CHECK_IDX(idx);
    if (!out || k == 0 || B == 0) {
        kdb_set_error("probe_heap_plan: out, k and B must not be zero");
        return KDB_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    KDB_HIP(hipSetDevice(idx->device));
    const KdbView v = kdb_make_view(idx);
    KdbHeapPlan p{};
    const int rc = kdb_heap_walk_plan(idx, v, ef, k, B, &p);
    if (rc) return rc;
    out[0] = p.hsize, out[1] = p.reg_results, out[2] = p.nl_c, out[3] = p.cap_c, out[4] = p.lds, out[5] = p.grid, out[6] = p.tail_bytes;
    return KDB_OK;
}

extern "C" int kdb_index_set_launch_timing(kdb_index *idx, int on) {
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->time_launches = on != 0;
    return KDB_OK;
}

extern "C" int kdb_index_sync(kdb_index *idx) {
    KDB_CHECK_IDX(idx);
    KDB_HIP(hipSetDevice(idx->device));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    return KDB_OK;
}

// out[4]: [0] launches that carried at least two distinct (k, effective ef), [1] the calls they carried, [2] callers that could not
// join an open launch because of their k or ef, [3] reserved
extern "C" int kdb_index_mixed_stats(kdb_index *idx, uint64_t *out) {
    KDB_CHECK_IDX(idx);
    if (!out) return KDB_ERR_INVALID;
    std::lock_guard<std::mutex> lk(idx->mu);
    out[0] = idx->n_mixed_launches;
    out[1] = idx->n_mixed_calls;
    out[2] = idx->n_mixed_refused;
    out[3] = 0;
    return KDB_OK;
}

// statistics of the concurrent host-pointer calls, out[10]: [0] launches that left through a slot, [1] calls they carried, [2] the largest
// number of queries one launch carried, [3] slots of this index; combined searches: [4] calls, [5] ns they waited for a launch (sum),
// [6] ns from launch to their own completion word seen (sum), [7] ns threads spent launching groups (sum), [8] naps, [9] the running
// estimate of a call's wait in ns
extern "C" int kdb_index_caller_stats(kdb_index *idx, uint64_t *out) {
    KDB_CHECK_IDX(idx);
    if (!out) return KDB_ERR_INVALID;
    std::lock_guard<std::mutex> lk(idx->mu);
    out[0] = idx->n_groups;
    out[1] = idx->n_group_members;
    out[2] = idx->largest_group;
    out[3] = (uint64_t)idx->n_slots;
    out[4] = idx->n_combined_calls.load();
    out[5] = idx->ns_to_launch.load();
    out[6] = idx->ns_launch_to_done.load();
    out[7] = idx->ns_in_launch.load();
    out[8] = idx->n_naps.load();
    out[9] = idx->walk_ns.load();
    return KDB_OK;
}

extern "C" int kdb_search_set_trace(kdb_index *idx, uint32_t *per_query_ndist, uint32_t *per_query_nhops, int on_device) {
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->trace_ndist = per_query_ndist;
    idx->trace_nhops = per_query_nhops;
    idx->trace_on_device = on_device;
    return KDB_OK;
}

extern "C" int kdb_index_create(const kdb_index_desc *desc, kdb_index **out) {
    if (!desc || !out) {
        kdb_set_error("kdb_index_create: null argument");
        return KDB_ERR_INVALID;
    }
    *out = nullptr;
    if (desc->dim == 0 || desc->capacity == 0 || desc->capacity > KDB_ID_MASK - 1) {
        kdb_set_error("kdb_index_create: dim and capacity must be > 0 (capacity < 2^30)");
        return KDB_ERR_INVALID;
    }
    // hnsw.New validation (hnsw_index.go:203-229): f16 only euclidean, int8 only cosine
    if (desc->precision > KDB_PREC_I8 || desc->metric > KDB_METRIC_COSINE) {
        kdb_set_error("unsupported precision/metric enum");
        return KDB_ERR_INVALID;
    }
    if (desc->precision == KDB_PREC_F16 && desc->metric != KDB_METRIC_L2) {
        kdb_set_error("precision 'float16' only supports the 'euclidean' metric");
        return KDB_ERR_INVALID;
    }
    if (desc->precision == KDB_PREC_I8 && desc->metric != KDB_METRIC_COSINE) {
        kdb_set_error("precision 'int8' only supports the 'cosine' metric");
        return KDB_ERR_INVALID;
    }
    uint32_t m = desc->m ? desc->m : 16;
    if (2 * m > KDB_MAX_DEG0) {
        kdb_set_error("m=%u too large (mMax0 = 2m must be <= %u)", m, KDB_MAX_DEG0);
        return KDB_ERR_UNSUPPORTED;
    }
    int rc = check_device(desc->device_id);
    if (rc) return rc;
    KDB_HIP(hipSetDevice(desc->device_id));
    kdb_index *idx = new (std::nothrow) kdb_index();
    if (!idx) return KDB_ERR_OOM;
    idx->desc = *desc;
    idx->desc.m = m;
    if (!idx->desc.ef_construction) idx->desc.ef_construction = 200;
    idx->device = desc->device_id;
    idx->cap = desc->capacity;
    idx->deg0 = 2 * m;
    idx->deg_up = m;
    idx->elem = desc->precision == KDB_PREC_F32 ? 4 : desc->precision == KDB_PREC_F16 ? 2 : 1;
    idx->ld = (desc->dim + 15u) & ~15u;
    idx->ld16 = (idx->ld + 63u) & ~63u;
    auto fail = [&](int code) {
        kdb_index_destroy(idx);
        return code;
    };
#define KDB_TRY(call)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (call);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            kdb_set_error("%s failed: %s", #call, hipGetErrorString(_e));                              \
            return fail(_e == hipErrorOutOfMemory ? KDB_ERR_OOM : KDB_ERR_HIP);                        \
        }                                                                                              \
    } while (0)
    const size_t n1 = (size_t)idx->cap + 1;
    KDB_TRY(hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking));
    KDB_TRY(hipStreamCreateWithFlags(&idx->stream2, hipStreamNonBlocking));
    KDB_TRY(hipEventCreateWithFlags(&idx->ev_io, hipEventDisableTiming));
    {   // slots of the concurrent host-pointer calls: their streams get the highest priority the device offers, so that a one-query
        // walk is not queued behind the waves of a large batch
        const char *e = getenv("KDB_SLOTS");
        int ns = e ? atoi(e) : 4; // (four: the hardware queues a process has unless GPU_MAX_HW_QUEUES says otherwise; measured 4 vs 8: DESIGN 5.7)
        idx->n_slots = ns < 1 ? 1 : ns > KDB_MAX_SLOTS ? KDB_MAX_SLOTS : ns;
        const char *cm = getenv("KDB_COMBINE_MIXED"); // 0: callers combine with callers of their own (k, ef) only
        idx->combine_mixed = !(cm && atoi(cm) == 0);
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        for (int i = 0; i < idx->n_slots; i++) KDB_TRY(hipStreamCreateWithPriority(&idx->slots[i].stream, hipStreamNonBlocking, prio_hi));
        // completion words of the combined launches: page-locked, coherent, written by the kernels at system scope
        // (+ 16 words per group: the session word of an open launch, on a cache line of its own)
        KDB_TRY(hipHostMalloc(reinterpret_cast<void **>(&idx->h_done_pool), (size_t)KDB_GROUP_POOL * (KDB_GROUP_CAP + 16u) * 4, hipHostMallocCoherent | hipHostMallocMapped));
        memset(idx->h_done_pool, 0, (size_t)KDB_GROUP_POOL * (KDB_GROUP_CAP + 16u) * 4);
        for (int i = 0; i < KDB_GROUP_POOL; i++) {
            idx->groups[i].h_done = idx->h_done_pool + (size_t)i * (KDB_GROUP_CAP + 16u);
            idx->groups[i].h_ctl = idx->groups[i].h_done + KDB_GROUP_CAP;
        }
    }
    for (uint32_t i = 0; i < kdb_index::RING; i++) {
        KDB_TRY(hipEventCreate(&idx->ring_ev0[i]));
        KDB_TRY(hipEventCreate(&idx->ring_ev1[i]));
    }
    idx->ev0 = idx->ring_ev0[0];
    idx->ev1 = idx->ring_ev1[0];
    KDB_TRY(hipMalloc(&idx->d_rows, n1 * idx->ld * idx->elem));
    KDB_TRY(hipMemsetAsync(idx->d_rows, 0, (size_t)idx->ld * idx->elem, idx->stream)); // row 0
    // (the half-precision ranking copy of float32 rows is made by the first exact scan that can use it: kdb_ensure_rows16; the walk
    // planes by the first large-batch walk: kdb_ensure_walk_planes -- both convert row 0 with the rest)
    KDB_TRY(hipMalloc(&idx->d_norms, n1 * 4));
    KDB_TRY(hipMemsetAsync(idx->d_norms, 0, n1 * 4, idx->stream));
    KDB_TRY(hipMalloc(&idx->d_adj0, n1 * idx->deg0 * 4));
    KDB_TRY(hipMemsetAsync(idx->d_adj0, 0, n1 * idx->deg0 * 4, idx->stream));
    KDB_TRY(hipMalloc(&idx->d_up_idx, n1 * 4));
    KDB_TRY(hipMemsetAsync(idx->d_up_idx, 0, n1 * 4, idx->stream));
    KDB_TRY(hipMalloc(&idx->d_levels, n1));
    KDB_TRY(hipMemsetAsync(idx->d_levels, 0, n1, idx->stream));
    const size_t dw = ((n1 + 31) / 32 + 3) & ~(size_t)3;
    KDB_TRY(hipMalloc(&idx->d_deleted, dw * 4));
    KDB_TRY(hipMemsetAsync(idx->d_deleted, 0, dw * 4, idx->stream));
    for (int i = 0; i < KDB_LANES; i++) {
        KDB_TRY(hipEventCreateWithFlags(&idx->lanes[i].done, hipEventDisableTiming));
        KDB_TRY(hipMalloc(&idx->lanes[i].d_work, 64 * 4));
        KDB_TRY(hipMemsetAsync(idx->lanes[i].d_work, 0, 64 * 4, idx->stream));
    }
    {
        hipDeviceProp_t prop;
        KDB_TRY(hipGetDeviceProperties(&prop, desc->device_id));
        idx->n_cu = prop.multiProcessorCount;
    }
    KDB_TRY(hipMalloc(&idx->d_ctr, kdb_index::RING * 32));
    KDB_TRY(hipMemsetAsync(idx->d_ctr, 0, kdb_index::RING * 32, idx->stream));
    KDB_TRY(hipStreamSynchronize(idx->stream));
#undef KDB_TRY
    *out = idx;
    return KDB_OK;
}

extern "C" void kdb_index_destroy(kdb_index *idx) {
    if (!idx) return;
    { KdbWriteLock w(idx); } // host-pointer calls still in flight finish first (Close waits for the read locks, hnsw_index.go:3533)
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    (void)hipDeviceSynchronize(); // callers' streams may still run kernels of this index
    void *bufs[] = {idx->d_rows,  idx->d_norms,   idx->d_adj0,    idx->d_adj_up, idx->d_up_idx, idx->d_levels,
                    idx->d_deleted, idx->d_ctr, idx->d_iobuf, idx->d_build, idx->d_rows16, idx->d_adj_up_slot,
                    idx->d_walk_hi, idx->d_walk_lo, idx->d_walk_err};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    for (void *c : idx->d_col)
        if (c) (void)hipFree(c);
    for (kdb_lane &l : idx->lanes) {
        void *lb[] = {l.d_visited, l.d_scratch, l.d_qbuf, l.d_gentry, l.d_work, l.d_tie, l.d_byid};
        for (void *b : lb)
            if (b) (void)hipFree(b);
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.side_ev1) kdb_heap_overlap_forget(idx);
        if (l.side_ev0) (void)hipEventDestroy(l.side_ev0);
        if (l.side_ev1) (void)hipEventDestroy(l.side_ev1);
        if (l.side) (void)hipStreamDestroy(l.side);
    }
    for (uint32_t i = 0; i < kdb_index::RING; i++) {
        if (idx->ring_ev0[i]) (void)hipEventDestroy(idx->ring_ev0[i]);
        if (idx->ring_ev1[i]) (void)hipEventDestroy(idx->ring_ev1[i]);
    }
    if (idx->h_done_pool) (void)hipHostFree(idx->h_done_pool);
    for (kdb_slot &sl : idx->slots) {
        if (sl.d_io) (void)hipFree(sl.d_io);
        if (sl.h_pin) (void)hipHostFree(sl.h_pin);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
    }
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    if (idx->stream2) (void)hipStreamDestroy(idx->stream2);
    if (idx->ev_io) (void)hipEventDestroy(idx->ev_io);
    delete idx;
}

static int upload_rows_impl(kdb_index *idx, uint32_t first_id, uint32_t n, const void *rows, hipMemcpyKind kind) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!rows || first_id == 0 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("upload_rows: ids %u..%llu outside 1..%u", first_id, (unsigned long long)first_id + n - 1, idx->cap);
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    const size_t rb = (size_t)idx->desc.dim * idx->elem, lb = (size_t)idx->ld * idx->elem;
    unsigned char *dst = reinterpret_cast<unsigned char *>(idx->d_rows) + (size_t)first_id * lb;
    if (lb != rb) KDB_HIP(hipMemsetAsync(dst, 0, (size_t)n * lb, idx->stream)); // zero the pad columns
    KDB_HIP(hipMemcpy2DAsync(dst, lb, rows, rb, rb, n, kind, idx->stream));
    // ||x||^2 per row: ranking key of the L2 flat scan; for float32 rows also the largest one (error band of the
    // f16-ranked cosine scan: the reference normalises cosine rows at insert, the mirror does not assume it)
    if (idx->d_rows16) { // ranking copy of the new rows
        int rc = kdb_launch_rows_to_f16(reinterpret_cast<const float *>(idx->d_rows), idx->d_rows16, idx->ld, idx->ld16, first_id, n, idx->stream);
        if (rc) return rc;
    }
    if (idx->d_walk_hi) { // walk planes of the new rows
        int rc = kdb_launch_walk_planes(reinterpret_cast<const float *>(idx->d_rows), idx->d_walk_hi, idx->d_walk_lo, idx->d_walk_err, idx->ld, first_id, n, idx->stream);
        if (rc) return rc;
    }
    const bool want_norms = idx->desc.precision != KDB_PREC_I8 &&
                            (idx->desc.metric == KDB_METRIC_L2 || idx->desc.precision == KDB_PREC_F32);
    uint32_t max_bits = 0;
    if (want_norms) {
        KdbView v = kdb_make_view(idx);
        uint32_t *d_max = idx->desc.precision == KDB_PREC_F32 ? kdb_cur(idx).d_work + 12 : nullptr;
        if (d_max) KDB_HIP(hipMemsetAsync(d_max, 0, 4, idx->stream));
        int rc = kdb_launch_row_norms(v, idx->d_norms, first_id, n, d_max, idx->stream);
        if (rc) return rc;
        if (d_max) KDB_HIP(hipMemcpyAsync(&max_bits, d_max, 4, hipMemcpyDeviceToHost, idx->stream));
    }
    KDB_HIP(hipStreamSynchronize(idx->stream)); // host rows are consumed before returning (cgo rule)
    if (max_bits) {
        float m;
        memcpy(&m, &max_bits, 4);
        if (m > idx->max_norm2) idx->max_norm2 = m;
    }
    return KDB_OK;
}

extern "C" int kdb_index_upload_rows(kdb_index *idx, uint32_t first_id, uint32_t n, const void *rows) {
    return upload_rows_impl(idx, first_id, n, rows, hipMemcpyHostToDevice);
}
extern "C" int kdb_index_upload_rows_dev(kdb_index *idx, uint32_t first_id, uint32_t n, const void *d_rows) {
    return upload_rows_impl(idx, first_id, n, d_rows, hipMemcpyDeviceToDevice);
}

extern "C" int kdb_index_download_rows(kdb_index *idx, uint32_t first_id, uint32_t n, void *rows) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!rows || first_id == 0 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("download_rows: bad id range");
        return KDB_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    KDB_HIP(hipSetDevice(idx->device));
    const size_t rb = (size_t)idx->desc.dim * idx->elem, lb = (size_t)idx->ld * idx->elem;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(idx->d_rows) + (size_t)first_id * lb;
    KDB_HIP(hipMemcpy2DAsync(rows, rb, src, lb, rb, n, hipMemcpyDeviceToHost, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    return KDB_OK;
}

extern "C" int kdb_index_upload_norms(kdb_index *idx, uint32_t first_id, uint32_t n, const float *norms) {
    KDB_CHECK_IDX(idx);
    if (idx->desc.precision != KDB_PREC_I8) {
        kdb_set_error("upload_norms: only int8 indexes carry stored norms");
        return KDB_ERR_INVALID;
    }
    if (!norms || first_id == 0 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("upload_norms: bad id range");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    KDB_HIP(hipMemcpyAsync(idx->d_norms + first_id, norms, (size_t)n * 4, hipMemcpyHostToDevice, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    return KDB_OK;
}

extern "C" int kdb_index_set_quantizer(kdb_index *idx, float abs_max) {
    KDB_CHECK_IDX(idx);
    idx->absmax = abs_max;
    return KDB_OK;
}

extern "C" int kdb_index_get_quantizer(kdb_index *idx, float *abs_max) {
    KDB_CHECK_IDX(idx);
    if (!abs_max) return KDB_ERR_INVALID;
    *abs_max = idx->absmax;
    return KDB_OK;
}

extern "C" int kdb_index_set_count(kdb_index *idx, uint32_t count) {
    KDB_CHECK_IDX(idx);
    if (count > idx->cap) {
        kdb_set_error("set_count: %u exceeds capacity %u", count, idx->cap);
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (count != idx->count) idx->graph_epoch++; // the derived upper-slot table tests ids against count
    idx->count = count;
    return KDB_OK;
}

// growNodes (hnsw_index.go:2732-2768): the reference doubles `nodes` and `quantizedNorms` when an id outgrows them.  Here every
// per-id array of the mirror moves to a larger allocation ON THE DEVICE (rows, ranking copy, norms, level-0 lists, upper-slot
// index, levels, deleted bits); the upper pool and the graph itself are untouched.  Per-wave visited bitsets are sized by the
// capacity: they are dropped and re-made by the next search.  No-op when the capacity is already that large.
extern "C" int kdb_index_reserve(kdb_index *idx, uint32_t new_capacity) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (new_capacity <= idx->cap) return KDB_OK;
    if (new_capacity > KDB_ID_MASK - 1) {
        kdb_set_error("reserve: capacity %u exceeds the 2^30-1 ids of an index", new_capacity);
        return KDB_ERR_INVALID;
    }
    KDB_HIP(hipSetDevice(idx->device));
    // walks of callers' streams may still read the arrays that are about to move
    KDB_HIP(hipDeviceSynchronize());
    const size_t o1 = (size_t)idx->cap + 1, n1 = (size_t)new_capacity + 1;
    const size_t row_b = (size_t)idx->ld * idx->elem;
    auto words = [](size_t n) { return ((n + 31) / 32 + 3) & ~(size_t)3; };
    struct Arr {
        void **p;
        size_t old_bytes, new_bytes;
    };
    void *rows16 = idx->d_rows16;
    const size_t wp = idx->d_walk_hi ? 1 : 0; // the walk planes move with the rows (the new rows are zero: zero planes, bound 0)
    void *walk_hi = idx->d_walk_hi, *walk_lo = idx->d_walk_lo, *walk_err = idx->d_walk_err;
    void *cols[KDB_MAX_COLUMNS]; // live metadata columns move with the rest; their tail is "absent" (NaN for KDB_COL_F64), not zero
    for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++) cols[c] = idx->d_col[c];
    auto col_b = [&](uint32_t c) -> size_t { return idx->col_kind[c] == KDB_COL_F64 ? 8 : idx->col_kind[c] == KDB_COL_CODE ? 4 : 0; };
    std::vector<Arr> arrs = {{&idx->d_rows, o1 * row_b, n1 * row_b},
                  {&rows16, idx->d_rows16 ? o1 * idx->ld16 * 2 : 0, idx->d_rows16 ? n1 * idx->ld16 * 2 : 0},
                  {&walk_hi, wp * o1 * idx->ld * 2, wp * n1 * idx->ld * 2},
                  {&walk_lo, wp * o1 * idx->ld * 2, wp * n1 * idx->ld * 2},
                  {&walk_err, wp * o1 * 4, wp * n1 * 4},
                  {reinterpret_cast<void **>(&idx->d_norms), o1 * 4, n1 * 4},
                  {reinterpret_cast<void **>(&idx->d_adj0), o1 * idx->deg0 * 4, n1 * idx->deg0 * 4},
                  {reinterpret_cast<void **>(&idx->d_up_idx), o1 * 4, n1 * 4},
                  {reinterpret_cast<void **>(&idx->d_levels), o1, n1},
                  {reinterpret_cast<void **>(&idx->d_deleted), words(o1) * 4, words(n1) * 4}};
    for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++)
        if (cols[c]) arrs.push_back({&cols[c], o1 * col_b(c), n1 * col_b(c)});
    const int NA = (int)arrs.size();
    std::vector<void *> fresh((size_t)NA, nullptr);
    for (int i = 0; i < NA; i++) { // every allocation first: a failure leaves the index as it was
        if (!arrs[i].new_bytes) continue;
        if (hipMalloc(&fresh[i], arrs[i].new_bytes) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j < i; j++)
                if (fresh[j]) (void)hipFree(fresh[j]);
            kdb_set_error("reserve: no room for capacity %u (%zu bytes for array %d)", new_capacity, arrs[i].new_bytes, i);
            return KDB_ERR_OOM;
        }
    }
    hipStream_t s = idx->stream;
    for (int i = 0; i < NA; i++) {
        if (!fresh[i]) continue;
        KDB_HIP(hipMemcpyAsync(fresh[i], *arrs[i].p, arrs[i].old_bytes, hipMemcpyDeviceToDevice, s));
        KDB_HIP(hipMemsetAsync(reinterpret_cast<unsigned char *>(fresh[i]) + arrs[i].old_bytes, 0, arrs[i].new_bytes - arrs[i].old_bytes, s));
    }
    for (int i = 0; i < NA; i++) // (nothing is freed yet: a failure here leaves the index on its old arrays)
        for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++)
            if (fresh[i] && arrs[i].p == &cols[c] && idx->col_kind[c] == KDB_COL_F64) {
                const int frc = kdb_launch_col_fill(fresh[i], KDB_COL_F64, o1, n1 - o1, s);
                if (frc) {
                    (void)hipStreamSynchronize(s);
                    for (void *f : fresh)
                        if (f) (void)hipFree(f);
                    return frc;
                }
            }
    KDB_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < NA; i++) {
        if (!fresh[i]) continue;
        (void)hipFree(*arrs[i].p);
        *arrs[i].p = fresh[i];
    }
    for (uint32_t c = 0; c < KDB_MAX_COLUMNS; c++) idx->d_col[c] = cols[c];
    idx->d_rows16 = reinterpret_cast<uint16_t *>(rows16);
    idx->d_walk_hi = reinterpret_cast<uint16_t *>(walk_hi);
    idx->d_walk_lo = reinterpret_cast<uint16_t *>(walk_lo);
    idx->d_walk_err = reinterpret_cast<float *>(walk_err);
    // scratch whose size follows the capacity: visited bitsets of both lanes, the builders' workspace
    for (kdb_lane &l : idx->lanes) {
        if (l.d_visited) (void)hipFree(l.d_visited);
        l.d_visited = nullptr;
        l.vis_slots = 0;
    }
    if (idx->d_build) (void)hipFree(idx->d_build);
    idx->d_build = nullptr;
    idx->build_bytes = 0;
    idx->cap = new_capacity;
    idx->desc.capacity = new_capacity;
    return KDB_OK;
}

// float32 indexes: the half-precision RANKING copy of the rows (+50 % row memory) exists from the first exact scan on -- an
// index that is only ever walked never pays for it; KDB_INDEX_NO_F16_SHADOW keeps it away for good.  Called under idx->mu;
// every row uploaded so far is in HBM (add_vectors returns after its copies), later uploads convert their own rows.
int kdb_ensure_rows16(kdb_index *idx, hipStream_t s) {
    if (idx->d_rows16 || idx->rows16_refused || idx->desc.precision != KDB_PREC_F32 || (idx->desc.reserved & KDB_INDEX_NO_F16_SHADOW))
        return KDB_OK;
    const size_t n1 = (size_t)idx->cap + 1;
    uint16_t *copy = nullptr;
    if (hipMalloc(&copy, n1 * idx->ld16 * 2) != hipSuccess) {
        (void)hipGetLastError();
        idx->rows16_refused = true; // no room: the scan ranks on the float32 rows (same answers) and does not ask again
        return KDB_OK;
    }
    // The copy is published only once it is COMPLETE: scans of other streams (the cluster's second lane, a second caller)
    // and later uploads on idx->stream order against nothing but this wait -- a one-time cost of the first exact scan.
    int rc = kdb_launch_rows_to_f16(reinterpret_cast<const float *>(idx->d_rows), copy, idx->ld, idx->ld16, 0, idx->count + 1, s);
    if (rc == KDB_OK && hipStreamSynchronize(s) != hipSuccess) {
        kdb_set_error("half-precision ranking copy: conversion failed");
        rc = KDB_ERR_HIP;
    }
    if (rc) {
        (void)hipFree(copy);
        return rc;
    }
    idx->d_rows16 = copy;
    return KDB_OK;
}

// The half-precision ranking copy of a float32 index (made by its first exact scan, +50 % row memory) can be given back: an
// index that is mostly walked and scanned once in a while need not keep 19 GB per 12.5M x 768 shard.  The next exact scan makes
// it again (or never, with refuse_for_good != 0 -- the effect of KDB_INDEX_NO_F16_SHADOW from then on).
extern "C" int kdb_index_drop_f16_shadow(kdb_index *idx, int refuse_for_good) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    if (idx->d_rows16) {
        KDB_HIP(hipDeviceSynchronize()); // scans of callers' streams may still rank on it
        (void)hipFree(idx->d_rows16);
        idx->d_rows16 = nullptr;
    }
    idx->rows16_refused = false;
    if (refuse_for_good) idx->desc.reserved |= KDB_INDEX_NO_F16_SHADOW;
    return KDB_OK;
}

// The walk planes of a float32 cosine index (made by its first large-batch walk, +100 % row memory) can be given back the same
// way: the next such walk makes them again (or never, with refuse_for_good != 0 -- KDB_INDEX_NO_WALK_PLANES from then on).
static void free_walk_planes(kdb_index *idx) {
    if (idx->d_walk_hi) (void)hipFree(idx->d_walk_hi);
    if (idx->d_walk_lo) (void)hipFree(idx->d_walk_lo);
    if (idx->d_walk_err) (void)hipFree(idx->d_walk_err);
    idx->d_walk_hi = idx->d_walk_lo = nullptr;
    idx->d_walk_err = nullptr;
}
extern "C" int kdb_index_drop_walk_planes(kdb_index *idx, int refuse_for_good) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    if (idx->d_walk_hi) {
        KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read them
        free_walk_planes(idx);
    }
    idx->walk_refused = false;
    if (refuse_for_good) idx->desc.reserved |= KDB_INDEX_NO_WALK_PLANES;
    return KDB_OK;
}

// Called under idx->mu by the launch that has picked a planes kernel (search_kernel.cuh), so latency-mode walks, L2 and quantised
// indexes never get here.  Every row of the allocation is converted (rows uploaded ahead of set_count included; what was never
// uploaded converts to whatever it holds and is never read), and the planes are published only once they are COMPLETE: walks of
// other streams and later uploads on idx->stream order against nothing but this wait -- a one-time cost of the first such walk.
// No room: `walk_refused`, the walk carries on on the float32 rows and does not ask again.
int kdb_ensure_walk_planes(kdb_index *idx, hipStream_t s) {
    if (idx->d_walk_hi || idx->walk_refused || !kdb_walk_planes_shape(idx)) return KDB_OK;
    const size_t n1 = (size_t)idx->cap + 1;
    uint16_t *hi = nullptr, *lo = nullptr;
    float *err = nullptr;
    if (hipMalloc(&hi, n1 * idx->ld * 2) != hipSuccess || hipMalloc(&lo, n1 * idx->ld * 2) != hipSuccess || hipMalloc(&err, n1 * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (hi) (void)hipFree(hi);
        if (lo) (void)hipFree(lo);
        idx->walk_refused = true;
        return KDB_OK;
    }
    int rc = kdb_launch_walk_planes(reinterpret_cast<const float *>(idx->d_rows), hi, lo, err, idx->ld, 0, (uint32_t)n1, s);
    if (rc == KDB_OK && hipStreamSynchronize(s) != hipSuccess) {
        kdb_set_error("walk planes: conversion failed");
        rc = KDB_ERR_HIP;
    }
    if (rc) {
        (void)hipFree(hi);
        (void)hipFree(lo);
        (void)hipFree(err);
        return rc;
    }
    idx->d_walk_hi = hi;
    idx->d_walk_lo = lo;
    idx->d_walk_err = err;
    return KDB_OK;
}
