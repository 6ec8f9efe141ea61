// kdb_api_calls.hip -- host side of the C ABI (include/kektor_hip.h): how host-pointer calls of concurrent callers reach the device.
#include "kdb_internal.h"
#include "kdb_host.h"
#include <stdio.h>
#include <string.h>
#include <sched.h>
#include <time.h>
#include <sys/prctl.h>

// ---------------------------------------------------------------------------------------------
// Host-pointer calls: slots and groups (kdb_slot / kdb_group, kdb_internal.h)
//
// hnsw.Index.SearchWithScores takes activeMu.RLock (hnsw_index.go:343-352) and the engine calls it from one goroutine per request
// (pkg/engine/ops.go:1003-1007): any number of one-query calls are inside the index at once.  Here idx->mu is held only to pick a
// slot and to enqueue; staging copies, the wait for the answers and the copy back happen outside it.
//   * a call that finds a free slot goes out at once, alone (a lone caller never waits for company);
//   * a search of up to KDB_COMBINE_MAX_B queries without an allow list that finds every slot busy joins -- or founds -- the group
//     that waits for the next free slot: same flags = ONE launch, whatever k and ef are (the launch reads them per query:
//     kdb_mixed_plan.h; KDB_COMBINE_MIXED=0: same (k, ef) only).  The thread that frees a slot launches the group
//     (nobody is woken for it); the kernel reads the queries from the slot's page-locked buffer, writes the answers there and
//     publishes a completion word per query; every member watches its own words and leaves when ITS walk is done;
//   * writers wait until no such call is in flight and hold new ones back meanwhile (KdbWriteLock);
//   * everything else -- calls too large for a slot (KDB_HOST_PIN_MAX), traced calls, KDB_SEARCH_FAIL_ON_DROP, distances, by-id calls,
//     decode, consensus, belief -- takes a turn on the index's own staging buffer: HostTurn, below, is that protocol.
// ---------------------------------------------------------------------------------------------
// (KdbCarver's order: queries | k [B], ef [B] of a mixed call | allow list | ids | distances | counts; an absent region takes nothing)
StagedLayout kdb_staged_layout(const kdb_index *idx, uint32_t B, uint32_t k, bool allow, size_t dist_bytes, bool mixed) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    StagedLayout L;
    L.qbytes = (size_t)B * idx->desc.dim * 4;
    L.kbytes = mixed ? (size_t)B * 8 : 0;
    L.aw = allow ? kdb_bits_bytes(idx->count) : 0;
    KdbCarver cv;
    (void)cv.take(L.qbytes);
    L.o_keys = cv.take(L.kbytes);
    L.o_allow = cv.take(L.aw);
    L.o_ids = cv.take(0);
    L.o_dist = L.o_ids + (((size_t)B * k * 4 + 7) & ~(size_t)7); // 8-byte aligned: may hold doubles
    L.o_cnt = L.o_dist + (size_t)B * k * dist_bytes;
    L.out_span = L.o_cnt + (size_t)B * 4 - L.o_ids;
    L.total = al(L.o_cnt + (size_t)B * 4) + 1024;
    return L;
}

int kdb_slot_find_free(const kdb_index *idx) {
    for (int i = 0; i < idx->n_slots; i++)
        if (!idx->slots[i].busy) return i;
    return -1;
}

// under idx->mu, slot idle (its last call has left)
int kdb_slot_ensure(kdb_index *idx, kdb_slot &sl, size_t bytes) {
    if (sl.bytes >= bytes) return KDB_OK;
    kdb_close_session(idx); // (hipFree / hipMalloc synchronise the device: an open launch must be able to end)
    if (sl.d_io) (void)hipFree(sl.d_io);
    if (sl.h_pin) (void)hipHostFree(sl.h_pin);
    sl.d_io = sl.h_pin = nullptr;
    sl.bytes = 0;
    size_t want = bytes * 2 < ((size_t)1 << 20) ? ((size_t)1 << 20) : bytes + bytes / 4;
    KDB_HIP(hipMalloc(&sl.d_io, want));
    // (coherent + mapped: the kernels of small calls read their queries from and write their answers straight into this buffer)
    KDB_HIP(hipHostMalloc(&sl.h_pin, want, hipHostMallocCoherent | hipHostMallocMapped));
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, sl.h_pin, 0) != hipSuccess || dp != sl.h_pin) { // (one address space on this platform: kernels take the host pointer)
        kdb_set_error("page-locked staging memory is not addressable by the device under its host address");
        return KDB_ERR_HIP;
    }
    sl.bytes = want;
    return KDB_OK;
}

static size_t host_pin_max() { // calls whose buffers exceed this go through the index's own staging buffer, from / to pageable memory
    static const size_t v = [] { const char *e = getenv("KDB_HOST_PIN_MAX"); return e ? (size_t)atoll(e) : (size_t)4 << 20; }();
    return v;
}

// an upper bound of what a call needs in a slot (the allow list is sized by the count the caller saw: at most the capacity's)
bool kdb_fits_a_slot(const kdb_index *idx, uint32_t B, uint32_t k, bool allow, size_t dist_bytes, bool mixed) {
    return (size_t)B * idx->desc.dim * 4 + (mixed ? (size_t)B * 8 + 256 : 0) + (allow ? kdb_bits_bytes(idx->cap) : 0) + (size_t)B * k * (4 + dist_bytes) + (size_t)B * 4 + 4096 <= host_pin_max();
}

static uint64_t now_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// ---- combined searches -------------------------------------------------------------------------
static kdb_group *group_get(kdb_index *idx) { // under mu
    for (kdb_group &g : idx->groups)
        if (!g.in_use) {
            g.in_use = true;
            g.gen++;
            if (g.gen == 0u) g.gen = 1u; // (0 is what a fresh pool holds)
            g.nq = g.refs = 0;
            g.slot = -1;
            g.rc = KDB_OK;
            g.err[0] = 0;
            g.launched.store(0u, std::memory_order_relaxed);
            g.failed.store(0u, std::memory_order_relaxed);
            g.members.clear();
            g.open = false;
            g.cap_q = 0;
            g.mixed = false;
            g.h_kq = g.h_efq = nullptr;
            return &g;
        }
    return nullptr;
}

// ---- open launches ("sessions"): a combined launch keeps accepting queries for KDB_SESSION_US microseconds while its kernel runs --
// a caller that arrives meanwhile writes its query into the slot's page-locked buffer, publishes the new count in the session word
// and is walked by a workgroup that was waiting for exactly that ticket: no launch, no wait for a slot.  At most one launch is open.
static uint32_t session_us() {
    static const uint32_t v = [] { const char *e = getenv("KDB_SESSION_US"); return e ? (uint32_t)atoi(e) : 300u; }();
    return v;
}
static uint32_t sess_word(uint32_t gen, uint32_t n, bool closed) { return ((gen & 0xffffu) << 16) | (closed ? 0x8000u : 0u) | (n & 0x3ffu); }

void kdb_close_session(kdb_index *idx) { // under mu
    kdb_group *g = idx->open_session;
    if (!g) return;
    g->open = false;
    __atomic_store_n(g->h_ctl, sess_word(g->gen, g->nq, true), __ATOMIC_RELEASE); // workgroups waiting for later tickets leave
    idx->open_session = nullptr;
}

// under mu: an open launch whose window has passed stops accepting queries (any caller that takes the lock may find it so: the
// calls that never join a launch -- filtered, large, traced -- used to leave it to the next joinable caller)
void kdb_close_expired_session(kdb_index *idx) {
    kdb_group *os = idx->open_session;
    if (os && now_ns() - os->t_launch_ns.load(std::memory_order_relaxed) > (uint64_t)session_us() * 1000ull) kdb_close_session(idx);
}

static void group_fail(kdb_group *g, int rc) {
    g->rc = rc;
    snprintf(g->err, sizeof g->err, "%s", kdb_last_error());
    g->failed.store(1u, std::memory_order_release);
}

// Launch group g (sealed: no longer idx->forming) on the free slot si.  Under idx->mu on entry and exit; the lock is dropped
// while the members' queries are copied into the slot's page-locked buffer.  ONE kernel launch (two with KDB_SEARCH_HEAP_ORDER):
// no copy commands -- the kernel reads the queries from the page-locked buffer, writes the answers there and publishes a
// completion word per query.  Any thread may do this for any group: the founder when a slot is free, else whoever frees one.
static void launch_search_group(kdb_index *idx, std::unique_lock<std::mutex> &lk, kdb_group *g, int si) {
    const uint64_t t_in = now_ns();
    kdb_slot &sl = idx->slots[si];
    sl.busy = true;
    g->slot = si;
    idx->inflight++;
    const uint32_t nq = g->nq;
    idx->n_groups++;
    idx->n_group_members += g->members.size();
    if (nq > idx->largest_group) idx->largest_group = nq;
    // an open launch has room for KDB_GROUP_CAP queries (int8 indexes quantise their queries in a kernel of its own: closed launches)
    bool session = session_us() != 0u && idx->desc.precision != KDB_PREC_I8 && !idx->writers_waiting && nq < KDB_GROUP_CAP;
    MixedKeys mx;
    if (g->mixed) { // the launch's bounds are fixed HERE (kdb_mixed_plan.h): capacity from the largest effective ef, stride from the largest k
        mx.ef_cap = kdb_mixed_ef_cap(g->eff_max);
        uint32_t stride = session ? kdb_mixed_open_stride(g->k_max, mx.ef_cap, idx->desc.dim, (uint32_t)g->dist_bytes, host_pin_max()) : 0u;
        if (stride == 0u) { // (no room for KDB_GROUP_CAP rows of the founders' own k: a closed launch of exactly them)
            session = false;
            stride = g->k_max;
        }
        g->k = stride;
        g->ef = mx.ef_cap;
        idx->n_mixed_launches++;
        idx->n_mixed_calls += g->members.size();
    }
    g->cap_q = session ? KDB_GROUP_CAP : nq;
    const StagedLayout L = kdb_staged_layout(idx, g->cap_q, g->k, false, g->dist_bytes, g->mixed);
    int rc = kdb_slot_ensure(idx, sl, L.total);
    if (rc == KDB_OK) {
        unsigned char *const h = reinterpret_cast<unsigned char *>(sl.h_pin);
        const size_t dim = idx->desc.dim;
        lk.unlock(); // (inflight > 0 keeps writers out; the group is sealed: its member list is final)
        size_t o = 0;
        uint32_t *const kq = reinterpret_cast<uint32_t *>(h + L.o_keys), *const efq = kq + g->cap_q;
        uint32_t b = 0;
        for (const kdb_group::Member &m : g->members) {
            memcpy(h + o, m.q, (size_t)m.B * dim * 4);
            o += (size_t)m.B * dim * 4;
            if (g->mixed)
                for (uint32_t i = 0; i < m.B; i++, b++) kq[b] = m.k, efq[b] = m.ef;
        }
        lk.lock();
        if (g->mixed) {
            g->h_kq = kq;
            g->h_efq = efq;
            mx.d_k = kq;
            mx.d_ef = efq;
        }
        g->h_ids = h + L.o_ids;
        g->h_dist = h + L.o_dist;
        g->h_cnt = h + L.o_cnt;
        g->t_launch_ns = now_ns();
        KdbDone done{g->h_done, g->gen};
        if (session && !idx->writers_waiting) {
            kdb_close_session(idx); // (the previous open launch finishes what it has)
            __atomic_store_n(g->h_ctl, sess_word(g->gen, nq, false), __ATOMIC_RELEASE);
            g->open = true;
            idx->open_session = g;
            done.sess_ctl = g->h_ctl;
            done.sess_gen = g->gen & 0xffffu;
            // workgroups beyond the first queries' own: they wait for the tickets of the callers that join -- more of them when the
            // launch starts large (the load is high: 256 callers fill a launch within its window)
            uint32_t spare = 3u * nq > 48u ? 3u * nq : 48u;
            if (spare > KDB_GROUP_CAP - nq) spare = KDB_GROUP_CAP - nq;
            done.sess_grid = nq + spare;
        }
        g->launched.store(1u, std::memory_order_release); // (before the kernel can publish a word: a member that sees its word set finds these fields)
        KdbLaneGuard lane(idx, sl.stream);
        rc = lane.rc;
        if (rc == KDB_OK)
            rc = kdb_search_dev_locked(idx, reinterpret_cast<float *>(h), done.sess_ctl ? g->cap_q : nq, g->k, g->ef, nullptr, g->flags,
                                   reinterpret_cast<uint32_t *>(h + L.o_ids), reinterpret_cast<float *>(h + L.o_dist), reinterpret_cast<uint32_t *>(h + L.o_cnt),
                                   sl.stream, nullptr, &done, g->mixed ? &mx : nullptr);
        if (rc && idx->open_session == g) kdb_close_session(idx);
    }
    if (rc) group_fail(g, rc);
    idx->ns_in_launch.fetch_add(now_ns() - t_in, std::memory_order_relaxed);
}

void kdb_launch_forming(kdb_index *idx, std::unique_lock<std::mutex> &lk) {
    if (!idx->forming || idx->writers_waiting) return;
    // calls that wait for a slot themselves must not starve behind a stream of joinable callers: every other freed slot is theirs
    if (idx->slot_waiters && (idx->release_seq++ & 1u)) return;
    const int si = kdb_slot_find_free(idx);
    if (si < 0) return;
    kdb_group *g = idx->forming;
    idx->forming = nullptr;
    (void)hipSetDevice(idx->device);
    launch_search_group(idx, lk, g, si);
}

// A member watches its own completion words.  The first few watchers of an index spin politely (what hipStreamSynchronize does,
// without its queue of signals); the others sleep: once for most of the expected time, then in short naps -- 64 callers must not
// burn 64 cores (a serving process usually runs under a CPU quota).
static int watch_done_words(kdb_index *idx, kdb_group *g, uint32_t off, uint32_t B) {
    static const uint32_t spin_max = [] { const char *e = getenv("KDB_SPIN_WATCHERS"); return e ? (uint32_t)atoi(e) : 1u; }(); // (measured, 256 callers on 16 CPUs: 4 spinners 424-427 k QPS, 1: 449-475 k, 0: 456-458 k but a lone caller 0.22 instead of 0.20 ms)
    static thread_local bool slack_set = false;
    const uint32_t gen = g->gen;
    const uint32_t *w = g->h_done + off;
    auto ready = [&] {
        for (uint32_t i = 0; i < B; i++)
            if (__atomic_load_n(w + i, __ATOMIC_ACQUIRE) != gen) return false;
        return true;
    };
    const uint64_t t0 = now_ns();
    const bool spin = idx->flag_waiters.fetch_add(1u, std::memory_order_relaxed) < spin_max;
    int rc = KDB_OK;
    if (!spin && !slack_set) { // naps of 15 us need a timer slack below the default 50 us (this thread only)
        (void)prctl(PR_SET_TIMERSLACK, 2000ul, 0ul, 0ul, 0ul);
        slack_set = true;
    }
    auto nap = [](uint64_t ns) {
        struct timespec ts = {(time_t)(ns / 1000000000ull), (long)(ns % 1000000000ull)};
        (void)clock_nanosleep(CLOCK_MONOTONIC, 0, &ts, nullptr);
    };
    bool first = true;
    uint64_t last_check = t0, naps = 0;
    const uint64_t est0 = idx->walk_ns.load(std::memory_order_relaxed);
    // short naps, but no more than about ten per call however long calls take under the present load
    constexpr uint64_t nap_div = 10ull, nap_min = 15000ull;
    const uint64_t nap_ns = est0 / nap_div < nap_min ? nap_min : est0 / nap_div > 150000ull ? 150000ull : est0 / nap_div;
    const uint64_t sess_ns = (uint64_t)session_us() * 1000ull;
    for (;;) {
        if (ready()) break;
        if (g->failed.load(std::memory_order_acquire)) {
            rc = g->rc ? g->rc : KDB_ERR_HIP;
            kdb_set_error("%s", g->err);
            break;
        }
        // An open launch is closed by whoever notices that its window has passed -- the next caller, or a member that is still
        // waiting: a query that met equal distances (KDB_SEARCH_HEAP_ORDER) is answered by the pass BEHIND the search kernel, which
        // ends only when the launch is closed; with nobody else calling, its own watcher must do it (it used to wait out the
        // workgroups' 0.5 s safety: one lone call in thirty took half a second with the flag the mirrors set)
        if (g->open.load(std::memory_order_relaxed) && g->launched.load(std::memory_order_acquire) && now_ns() - g->t_launch_ns.load(std::memory_order_relaxed) > sess_ns) {
            std::lock_guard<std::mutex> lk(idx->mu);
            if (idx->open_session == g) kdb_close_session(idx);
        }
        const uint64_t el = now_ns() - t0;
        if (spin && el < 2000000ull) {
            sched_yield();
            continue;
        }
        naps++;
        if (first && !spin) {
            first = false;
            if (est0 * 3u / 4u > el + nap_ns) { // most of the expected time in one piece
                nap(est0 * 3u / 4u - el > 1000000ull ? 1000000ull : est0 * 3u / 4u - el);
                continue;
            }
        }
        nap(el < 2000000ull ? nap_ns : el < 100000000ull ? 200000ull : 1000000ull);
        // a device fault leaves the words unset for ever: now and then ask the stream (any member may; the answer is for all)
        const uint64_t t = now_ns();
        if (t - t0 > 2000000000ull && t - last_check > 500000000ull && g->launched.load(std::memory_order_acquire) && !g->failed.load(std::memory_order_acquire)) {
            last_check = t;
            const hipError_t e = hipStreamQuery(idx->slots[g->slot].stream);
            if (e != hipErrorNotReady && !ready()) {
                kdb_set_error(e == hipSuccess ? "combined search: the launch finished without publishing every answer" : "combined search: %s", hipGetErrorString(e));
                (void)hipGetLastError();
                group_fail(g, KDB_ERR_HIP);
            }
        }
    }
    idx->flag_waiters.fetch_sub(1u, std::memory_order_relaxed);
    idx->n_naps.fetch_add(naps, std::memory_order_relaxed);
    if (rc == KDB_OK) { // running estimate (1/8 weights) of what a caller waits, for the next watcher's first sleep
        const uint64_t t1 = now_ns(), el = t1 - t0;
        const uint64_t tl = g->t_launch_ns.load(std::memory_order_relaxed);
        idx->n_combined_calls.fetch_add(1u, std::memory_order_relaxed);
        idx->ns_to_launch.fetch_add(tl > t0 ? tl - t0 : 0u, std::memory_order_relaxed);
        idx->ns_launch_to_done.fetch_add(tl > t0 ? t1 - tl : el, std::memory_order_relaxed);
        const uint32_t old = idx->walk_ns.load(std::memory_order_relaxed);
        const uint64_t upd = ((uint64_t)old * 7u + (el > 2000000ull ? 2000000ull : el)) / 8u;
        idx->walk_ns.store((uint32_t)upd, std::memory_order_relaxed);
    }
    return rc;
}

int kdb_combined_search_call(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, uint32_t flags, uint32_t *out_ids,
                             void *out_dist, uint32_t *out_count) {
    const size_t dist_bytes = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    // callers combine across (k, ef) by the rules of kdb_mixed_plan.h: the forming group takes any key with equal flags and bytes per
    // distance, a running open launch whatever its stride and capacity admit.  (KDB_COMBINE_MIXED=0, or an ef beyond
    // KDB_MIXED_COMBINE_EF_MAX: with callers of the same key only.)
    const uint32_t eff = kdb_mixed_effective_ef(ef, k, (flags & KDB_SEARCH_NEEDS_REFINE) != 0u);
    const bool may_mix = idx->combine_mixed && eff <= KDB_MIXED_COMBINE_EF_MAX;
    std::unique_lock<std::mutex> lk(idx->mu);
    if (idx->writers_waiting) idx->slot_cv.wait(lk, [&] { return idx->writers_waiting == 0; });
    kdb_group *g = nullptr;
    uint32_t off = 0;
    if (kdb_group *os = idx->open_session) { // a launch that still accepts queries: write mine into its buffer, publish the count
        if (now_ns() - os->t_launch_ns.load(std::memory_order_relaxed) > (uint64_t)session_us() * 1000ull || idx->writers_waiting) {
            kdb_close_session(idx);
        } else if (os->flags == flags && os->dist_bytes == dist_bytes && os->nq + B <= os->cap_q && !os->failed.load(std::memory_order_relaxed) &&
                   !(os->mixed ? may_mix && kdb_mixed_admit(k, eff, flags, (uint32_t)dist_bytes, os->k, os->ef, os->flags, (uint32_t)os->dist_bytes)
                               : os->k == k && os->eff == eff)) {
            idx->n_mixed_refused++; // (its k or ef alone keeps this caller out of the running launch)
        } else if (os->flags == flags && os->dist_bytes == dist_bytes && os->nq + B <= os->cap_q && !os->failed.load(std::memory_order_relaxed)) {
            g = os;
            off = g->nq;
            memcpy(reinterpret_cast<unsigned char *>(idx->slots[g->slot].h_pin) + (size_t)off * idx->desc.dim * 4, queries, (size_t)B * idx->desc.dim * 4);
            if (g->mixed) { // my entries of the per-query arrays, BEFORE the new count is published below
                for (uint32_t i = 0; i < B; i++) g->h_kq[off + i] = k, g->h_efq[off + i] = ef;
                idx->n_mixed_calls++;
            }
            g->nq += B;
            g->refs++;
            idx->n_group_members++;
            if (g->nq > idx->largest_group) idx->largest_group = g->nq;
            __atomic_store_n(g->h_ctl, sess_word(g->gen, g->nq, false), __ATOMIC_RELEASE);
        }
    }
    if (g) {
        // (joined an open launch)
    } else if ((g = idx->forming) && g->flags == flags && g->dist_bytes == dist_bytes && g->nq + B <= KDB_GROUP_CAP &&
               ((g->k == k && g->eff == eff && !g->mixed) || (may_mix && g->eff_max <= KDB_MIXED_COMBINE_EF_MAX))) { // join the group that waits for a slot
        off = g->nq;
        g->nq += B;
        g->refs++;
        g->members.push_back({queries, B, k, ef});
        if (g->k != k || g->eff != eff) g->mixed = true; // (its stride and capacity are fixed when it is launched)
        if (k > g->k_max) g->k_max = k;
        if (eff > g->eff_max) g->eff_max = eff;
    } else {
        while (!(g = group_get(idx))) idx->slot_cv.wait(lk); // (more founders than group objects: wait for one to come back)
        g->k = g->k_max = k;
        g->ef = ef;
        g->eff = g->eff_max = eff;
        g->flags = flags;
        g->dist_bytes = dist_bytes;
        g->nq = B;
        g->refs = 1;
        g->members.push_back({queries, B, k, ef});
        int si = idx->writers_waiting ? -1 : kdb_slot_find_free(idx);
        if (si >= 0) {
            launch_search_group(idx, lk, g, si); // a free slot: out at once, alone
        } else if (!idx->forming) {
            idx->forming = g; // whoever frees a slot (or ends a write) launches it; callers arriving meanwhile join
        } else { // the forming group is full or has another key: wait for a slot like any other call
            idx->slot_waiters++;
            idx->slot_cv.wait(lk, [&] { return idx->writers_waiting == 0 && (si = kdb_slot_find_free(idx)) >= 0; });
            idx->slot_waiters--;
            launch_search_group(idx, lk, g, si);
        }
    }
    lk.unlock();
    int rc = watch_done_words(idx, g, off, B);
    if (rc == KDB_OK) {
        while (!g->launched.load(std::memory_order_acquire)) sched_yield(); // (set before the launch: orders the reads below behind the launcher's writes)
        const size_t stride = g->k; // (the caller's own k unless the launch is mixed: then row by row, the first k of every row)
        if (stride == k) {
            memcpy(out_ids, g->h_ids + (size_t)off * k * 4, (size_t)B * k * 4);
            memcpy(out_dist, g->h_dist + (size_t)off * k * dist_bytes, (size_t)B * k * dist_bytes);
        } else {
            for (uint32_t i = 0; i < B; i++) {
                memcpy(out_ids + (size_t)i * k, g->h_ids + ((size_t)off + i) * stride * 4, (size_t)k * 4);
                memcpy(reinterpret_cast<unsigned char *>(out_dist) + (size_t)i * k * dist_bytes, g->h_dist + ((size_t)off + i) * stride * dist_bytes, (size_t)k * dist_bytes);
            }
        }
        memcpy(out_count, g->h_cnt + (size_t)off * 4, (size_t)B * 4);
    }
    lk.lock();
    if (--g->refs == 0) { // the last member out: every walk of the launch is done (its words are set), the slot and the group object are free
        if (idx->open_session == g) kdb_close_session(idx); // (nobody else joined: its kernel may end)
        if (g->failed.load(std::memory_order_acquire) && g->slot >= 0) {
            lk.unlock();
            (void)hipStreamSynchronize(idx->slots[g->slot].stream); // (whatever was queued must not outlive the slot's next use)
            lk.lock();
        }
        if (g->slot >= 0) {
            idx->slots[g->slot].busy = false;
            idx->inflight--;
        } else if (idx->forming == g) {
            idx->forming = nullptr;
        }
        g->in_use = false;
        kdb_launch_forming(idx, lk); // the group that gathered meanwhile leaves NOW, launched by this thread
        idx->slot_cv.notify_all();
    }
    return rc;
}

// ---- turns on the index's own staging buffer (HostTurn, DropWatch: kdb_host.h) -------------------
HostTurn::HostTurn(kdb_index *i, bool stream2_too) : idx(i), big(i->big_mu), lk(i->mu), both_streams(stream2_too) {
    kdb_close_expired_session(idx);
    if (idx->writers_waiting) idx->slot_cv.wait(lk, [&] { return idx->writers_waiting == 0; });
}
unsigned char *HostTurn::stage(size_t bytes) { // under lk; null: rc and the error are set, nothing is counted
    if ((rc = kdb_ensure_iobuf(idx, bytes)) != KDB_OK) return nullptr;
    idx->inflight++;
    counted = true;
    return reinterpret_cast<unsigned char *>(idx->d_iobuf);
}
HostTurn::~HostTurn() {
    if (!counted) return;
    if (lk.owns_lock()) lk.unlock();
    (void)hipStreamSynchronize(idx->stream);
    if (both_streams) (void)hipStreamSynchronize(idx->stream2);
    lk.lock();
    idx->inflight--;
    if (idx->inflight == 0 && idx->writers_waiting) idx->slot_cv.notify_all();
}

int DropWatch::check(const kdb_index *idx, const char *who) const {
    if (n_deleted <= 2047u || seq == 0 || kind != 1) return KDB_OK;
    unsigned long long c[4] = {0, 0, 0, 0};
    KDB_HIP(hipMemcpy(c, idx->d_ctr + (size_t)((seq - 1) % kdb_index::RING) * 4, 32, hipMemcpyDeviceToHost));
    if (!c[3]) return KDB_OK;
    kdb_set_error("%s: %llu pending traversal-only candidates were discarded (more than 2047 deleted nodes waiting in one "
                  "walk): answers may differ from the reference's", who, c[3]);
    return KDB_ERR_DIVERGED;
}

// Host-pointer search of a large batch in chunks that alternate between two streams (and two scratch lanes): the
// H2D copy of chunk c+1 and the D2H copy of chunk c-1 run under the walk of chunk c, and the waves that idle at the end of
// one chunk's launch start on the next.  SURVEY 8d counts the copies into the QPS of this entry point.
int kdb_search_staged_chunks(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                             uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count, uint32_t chunk) {
    HostTurn turn(idx, true); // (both streams: the destructor waits for stream2 as well)
    const size_t dist_bytes = (flags & KDB_SEARCH_DIST_F64) ? 8 : 4;
    const size_t dim = idx->desc.dim;
    KdbStage st; // (the allow list is the one region copied whole; queries and answers go chunk by chunk, below)
    const KdbRegion r_q = st.dev((size_t)B * dim * 4), r_allow = st.in(allow_bits, kdb_bits_bytes(idx->count)), r_ids = st.dev((size_t)B * k * 4),
                    r_dist = st.dev((size_t)B * k * dist_bytes), r_cnt = st.dev((size_t)B * 4);
    unsigned char *const p = turn.stage(st.total() + 1024);
    if (!p) return turn.rc;
    int rc = KDB_OK;
    float *d_q = r_q.at<float>(p);
    uint64_t *d_allow = r_allow.at<uint64_t>(p);
    uint32_t *d_ids = r_ids.at<uint32_t>(p);
    unsigned char *d_dist = r_dist.at<unsigned char>(p);
    uint32_t *d_cnt = r_cnt.at<uint32_t>(p);
    hipStream_t s1 = idx->stream, s2 = idx->stream2;
    turn.lk.unlock();
    if (allow_bits) {
        KDB_HIP(hipMemcpyAsync(d_allow, allow_bits, r_allow.bytes, hipMemcpyHostToDevice, s1));
        KDB_HIP(hipEventRecord(idx->ev_io, s1));
        KDB_HIP(hipStreamWaitEvent(s2, idx->ev_io, 0));
    }
    // copies from / to pageable host memory hold the calling thread until they are done: the results of chunk c-1 are
    // fetched AFTER chunk c has been queued, so the device always has the next walk in its queue
    auto fetch = [&](uint32_t b0, uint32_t nb, hipStream_t s) -> int {
        KDB_HIP(hipMemcpyAsync(out_ids + (size_t)b0 * k, d_ids + (size_t)b0 * k, (size_t)nb * k * 4, hipMemcpyDeviceToHost, s));
        KDB_HIP(hipMemcpyAsync(reinterpret_cast<unsigned char *>(out_dist) + (size_t)b0 * k * dist_bytes, d_dist + (size_t)b0 * k * dist_bytes,
                               (size_t)nb * k * dist_bytes, hipMemcpyDeviceToHost, s));
        KDB_HIP(hipMemcpyAsync(out_count + b0, d_cnt + b0, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        return KDB_OK;
    };
    uint32_t c = 0, prev_b0 = 0, prev_nb = 0;
    hipStream_t prev_s = nullptr;
    for (uint32_t b0 = 0; b0 < B; b0 += chunk, c++) {
        const uint32_t nb = B - b0 < chunk ? B - b0 : chunk;
        hipStream_t s = (c & 1u) ? s2 : s1;
        KDB_HIP(hipMemcpyAsync(d_q + (size_t)b0 * dim, queries + (size_t)b0 * dim, (size_t)nb * dim * 4, hipMemcpyHostToDevice, s));
        {
            std::lock_guard<std::mutex> enq(idx->mu); // idx->mu only around the enqueue: small calls go on meanwhile
            KdbLaneGuard lane(idx, s);
            if (lane.rc) return lane.rc;
            rc = kdb_search_dev_locked(idx, d_q + (size_t)b0 * dim, nb, k, ef, d_allow, flags, d_ids + (size_t)b0 * k,
                                   reinterpret_cast<float *>(d_dist + (size_t)b0 * k * dist_bytes), d_cnt + b0, s);
            if (rc) return rc;
        }
        if (prev_s) {
            rc = fetch(prev_b0, prev_nb, prev_s);
            if (rc) return rc;
        }
        prev_b0 = b0;
        prev_nb = nb;
        prev_s = s;
    }
    if (prev_s) {
        rc = fetch(prev_b0, prev_nb, prev_s);
        if (rc) return rc;
    }
    KDB_HIP(hipStreamSynchronize(s1));
    KDB_HIP(hipStreamSynchronize(s2));
    return KDB_OK;
}
