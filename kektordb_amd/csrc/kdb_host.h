// kdb_host.h -- what the files of the host API share (kdb_api.hip, kdb_api_graph.hip, kdb_api_calls.hip, kdb_api_query.hip,
// kdb_api_filter.hip, kdb_api_merge.hip): host only, included by them alone.  The kernel files include kdb_internal.h.
#pragma once
#include "kdb_internal.h"
#include "kdb_stage.h"
#include <string.h>

#define KDB_CHECK_IDX(idx)                       \
    do {                                         \
        if (!(idx)) {                            \
            kdb_set_error("null index handle");  \
            return KDB_ERR_INVALID;              \
        }                                        \
    } while (0)

struct MixedKeys { // a mixed launch (kdb_search_batch_mixed[_dev]): k and ef of every query on the device, the launch's capacity
    const uint32_t *d_k = nullptr, *d_ef = nullptr;
    uint32_t ef_cap = 0;
};

struct HostKeys { // a mixed host-pointer call: the caller's k [B] and ef [B], staged beside the queries
    const uint32_t *k, *ef;
};

struct KdbDone { // completion words of a combined launch (KdbMultiAllow::done_flags) and, for an open launch, its session word
    uint32_t *flags;
    uint32_t gen;
    const uint32_t *sess_ctl = nullptr;
    uint32_t sess_gen = 0, sess_grid = 0;
};

struct MultiLists { // heterogeneous batch (kdb_search_batch_multi_dev): G lists back to back + the list of every query
    uint32_t G = 0;
    uint64_t words64 = 0;
    const uint32_t *d_of_query = nullptr;
};

struct StagedLayout { // one call's (or group's) buffers inside a slot: the same offsets on the device and in page-locked memory
    size_t qbytes, kbytes, aw, o_keys, o_allow, o_ids, o_dist, o_cnt, out_span, total;
    size_t in_span() const { return aw ? o_allow + aw : kbytes ? o_keys + kbytes : qbytes; } // queries | keys | allow list: one copy
};

// ---- what the API files call across a file boundary (each defined in the file named) ---------
// kdb_api.hip
int kdb_ensure_qbuf(kdb_index *idx, size_t bytes);
int kdb_ensure_byid(kdb_index *idx, size_t bytes);
int kdb_ensure_iobuf(kdb_index *idx, size_t bytes);
int kdb_ensure_rows16(kdb_index *idx, hipStream_t s);
// kdb_api_query.hip
int kdb_prepare_queries(kdb_index *idx, const KdbView &v, const float *d_queries, uint32_t B, uint32_t Bpad,
                        uint32_t flags, void **d_q, float **d_qnorm, hipStream_t s);
int kdb_search_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, uint32_t ef,
                          const uint64_t *d_allow_bits, uint32_t flags, uint32_t *d_out_ids, float *d_out_dist,
                          uint32_t *d_out_count, hipStream_t s, const MultiLists *ml = nullptr, const KdbDone *done = nullptr,
                          const MixedKeys *mx = nullptr /* set: k is the stride of the output rows, ef is not read */);
int kdb_flat_dev_locked(kdb_index *idx, const float *d_queries, uint32_t B, uint32_t k, const uint64_t *d_allow_bits,
                        uint32_t flags, uint32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_count, hipStream_t s);
// kdb_api_calls.hip
StagedLayout kdb_staged_layout(const kdb_index *idx, uint32_t B, uint32_t k, bool allow, size_t dist_bytes, bool mixed = false);
int kdb_slot_find_free(const kdb_index *idx);
int kdb_slot_ensure(kdb_index *idx, kdb_slot &sl, size_t bytes);
bool kdb_fits_a_slot(const kdb_index *idx, uint32_t B, uint32_t k, bool allow, size_t dist_bytes, bool mixed = false);
void kdb_close_expired_session(kdb_index *idx);
int kdb_combined_search_call(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, uint32_t flags, uint32_t *out_ids,
                             void *out_dist, uint32_t *out_count);
int kdb_search_staged_chunks(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, uint32_t ef, const uint64_t *allow_bits,
                             uint32_t flags, uint32_t *out_ids, float *out_dist, uint32_t *out_count, uint32_t chunk);

// The frame of a device-pointer (_dev) call: idx->mu, the index's device, the caller's stream (null: the index's own) and, unless
// the call needs no scratch, a scratch lane of that stream -- given back before the lock is.
struct DevCall {
    kdb_index *idx;
    std::lock_guard<std::mutex> lk;
    hipStream_t s;
    bool laned = false;
    int rc;
    DevCall(kdb_index *i, void *stream, bool lane = true) : idx(i), lk(i->mu), s(stream ? (hipStream_t)stream : i->stream), rc(enter(lane)) {}
    ~DevCall() { if (laned) (void)kdb_lane_release(idx, s); }
    int enter(bool lane) {
        KDB_HIP(hipSetDevice(idx->device));
        if (!lane) return KDB_OK;
        const int r = kdb_lane_acquire(idx, s);
        laned = r == KDB_OK;
        return r;
    }
};

// ---- turns on the index's own staging buffer ----------------------------------------------------
// Calls that do not fit a slot, traced calls, KDB_SEARCH_FAIL_ON_DROP and every host-pointer call that is not a search or a scan of
// queries (distances, by-id, decode, consensus, belief) stage through idx->d_iobuf with copies from / to the caller's pageable
// memory, one such call at a time.  HostTurn is that turn, and its only implementation:
//   * the constructor takes big_mu, then idx->mu, closes an open launch whose window has passed and waits while writers wait;
//   * stage() sizes the buffer and counts the call (inflight: writers stay out until it has left, so count, capacity, rows and
//     deleted bits cannot move) -- after it the caller drops and re-takes `lk` as it likes: copies outside it, enqueues under it;
//   * the destructor runs on EVERY exit, the error returns too: it waits for the stream(s) -- queued copies read and write the
//     CALLER's buffers -- and only then stops counting the call and wakes a waiting writer.
// A KdbLaneGuard lives in an inner scope of the caller: it is gone before the destructor drops idx->mu.
struct HostTurn {
    kdb_index *idx;
    std::lock_guard<std::mutex> big;
    std::unique_lock<std::mutex> lk;
    const bool both_streams; // the call also enqueues on idx->stream2
    bool counted = false;
    int rc = KDB_OK;
    explicit HostTurn(kdb_index *i, bool stream2_too = false);
    unsigned char *stage(size_t bytes); // under lk; null: rc and the error are set, nothing is counted
    ~HostTurn();
};

// KDB_SEARCH_FAIL_ON_DROP: which launch the call's walk was and how many deleted nodes it could meet (note(): under idx->mu, right
// behind the enqueue) and, once the stream is idle, whether that walk discarded pending candidates
struct DropWatch {
    uint32_t n_deleted = 0;
    uint64_t seq = 0;
    int kind = 0;
    void note(const kdb_index *idx) {
        n_deleted = idx->n_deleted;
        seq = idx->launch_seq;
        kind = idx->last_kind;
    }
    int check(const kdb_index *idx, const char *who) const; // kdb_api_calls.hip
};

// The frame of a call that takes ONE turn: the turn, the buffer, the copies in outside idx->mu, the enqueue under it on a scratch
// lane, the copies out outside it, the wait.  declare(st) runs under idx->mu right after the turn is taken (sizes that follow the
// index's count are read there) and declares every region once; run(d, s) enqueues the work on d = the staged buffer.  The copies
// go region by region in declaration order on idx->stream.  Two calls differ, and say so:
struct KdbTurnOpt {
    bool lane = true;               // false: the kernel needs no scratch -- no lane, and run() is called OUTSIDE idx->mu (consensus)
    bool launch_first = false;      // nothing to copy in: run() before idx->mu is first dropped (filter_eval); with a lane only
    size_t slack = 0;               // bytes kept free behind the last region
    const char *drop_who = nullptr; // set: KDB_SEARCH_FAIL_ON_DROP, reported under this name
};
template <typename Declare, typename Run>
static int kdb_turn_call(kdb_index *idx, const KdbTurnOpt &opt, Declare declare, Run run) {
    HostTurn turn(idx);
    KdbStage st;
    int rc = declare(st);
    if (rc) return rc;
    if (st.overflow || (opt.launch_first && !opt.lane)) { // (launch_first launches under idx->mu: it goes with a lane only)
        kdb_set_error("turn call: %s", st.overflow ? "more staged regions than KdbStage::CAP" : "launch_first without a lane");
        return KDB_ERR_INVALID;
    }
    unsigned char *const d = turn.stage(st.total() + opt.slack);
    if (!d) return turn.rc;
    hipStream_t s = idx->stream;
    if (!opt.launch_first) {
        turn.lk.unlock();
        rc = st.copy_in(d, [&](void *dst, const void *src, size_t n) -> int { KDB_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s)); return KDB_OK; });
        if (rc) return rc;
        if (opt.lane) turn.lk.lock();
    }
    DropWatch drops;
    if (opt.lane) {
        KdbLaneGuard lane(idx, s);
        if (lane.rc) return lane.rc;
        rc = run(d, s);
        if (opt.drop_who) drops.note(idx);
    } else {
        rc = run(d, s);
    }
    if (turn.lk.owns_lock()) turn.lk.unlock();
    if (rc) return rc;
    rc = st.copy_out(d, [&](void *dst, const void *src, size_t n) -> int { KDB_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s)); return KDB_OK; });
    if (rc) return rc;
    KDB_HIP(hipStreamSynchronize(s));
    return opt.drop_who ? drops.check(idx, opt.drop_who) : KDB_OK;
}

// A search or an exact scan of queries on a turn: run(d_q, d_allow, d_ids, d_dist, d_cnt, stream, B, d_k, d_ef) as for staged_slot_call.
template <typename F>
static int staged_big_call(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, const uint64_t *allow_bits, uint32_t *out_ids, void *out_dist,
                           uint32_t *out_count, size_t dist_bytes, bool fail_on_drop, F run, const HostKeys *hk = nullptr) {
    KdbRegion q, kq, efq, allow, ids, dist, cnt;
    KdbTurnOpt opt;
    opt.slack = 1024;
    opt.drop_who = fail_on_drop ? "search" : nullptr;
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) {
            q = st.in(queries, (size_t)B * idx->desc.dim * 4);
            kq = st.in(hk ? hk->k : nullptr, (size_t)B * 4);
            efq = st.in(hk ? hk->ef : nullptr, (size_t)B * 4);
            allow = st.in(allow_bits, kdb_bits_bytes(idx->count));
            ids = st.out(out_ids, (size_t)B * k * 4);
            dist = st.out(out_dist, (size_t)B * k * dist_bytes);
            cnt = st.out(out_count, (size_t)B * 4);
            return KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return run(q.at<float>(d), allow.at<uint64_t>(d), ids.at<uint32_t>(d), dist.at<float>(d), cnt.at<uint32_t>(d), s, B, kq.at<uint32_t>(d), efq.at<uint32_t>(d));
        });
}

// One host-pointer call through a slot, alone: exact scans, filtered searches, searches of more than KDB_COMBINE_MAX_B queries.
// run(d_q, d_allow, d_ids, d_dist, d_cnt, stream, B, d_k, d_ef) enqueues the work (under idx->mu; d_k, d_ef: the staged arrays of a
// mixed call, else null).  Page-locked staging: one memcpy in, one copy of queries | allow list, ONE device-to-host copy of
// ids | distances | counts, one memcpy out -- or, for a graph search of a few queries, none: the kernel writes its answers straight
// into the page-locked buffer (posted writes over PCIe; the end of the kernel makes them visible).
template <typename F>
static int staged_slot_call(kdb_index *idx, const float *queries, uint32_t B, uint32_t k, const uint64_t *allow_bits, uint32_t *out_ids, void *out_dist,
                            uint32_t *out_count, size_t dist_bytes, bool direct_out, F run, const HostKeys *hk = nullptr) {
    constexpr size_t direct_max = (size_t)64 << 10;
    std::unique_lock<std::mutex> lk(idx->mu);
    kdb_close_expired_session(idx);
    int si = -1;
    idx->slot_waiters++;
    idx->slot_cv.wait(lk, [&] { return idx->writers_waiting == 0 && (si = kdb_slot_find_free(idx)) >= 0; });
    idx->slot_waiters--;
    kdb_slot &sl = idx->slots[si];
    sl.busy = true;
    idx->inflight++;
    idx->n_groups++;
    idx->n_group_members++;
    const StagedLayout L = kdb_staged_layout(idx, B, k, allow_bits != nullptr, dist_bytes, hk != nullptr);
    int rc = kdb_slot_ensure(idx, sl, L.total);
    unsigned char *const h = reinterpret_cast<unsigned char *>(sl.h_pin), *const d = reinterpret_cast<unsigned char *>(sl.d_io);
    bool queued = false;
    if (rc == KDB_OK) {
        lk.unlock(); // stage in outside the lock (inflight > 0 keeps writers out: count and capacity cannot move)
        memcpy(h, queries, L.qbytes);
        if (hk) {
            memcpy(h + L.o_keys, hk->k, (size_t)B * 4);
            memcpy(h + L.o_keys + (size_t)B * 4, hk->ef, (size_t)B * 4);
        }
        if (allow_bits) memcpy(h + L.o_allow, allow_bits, L.aw);
        lk.lock();
        const bool direct = direct_out && L.out_span <= direct_max;
        unsigned char *const o_base = direct ? h : d;
        {
            KdbLaneGuard lane(idx, sl.stream);
            rc = lane.rc;
            // queries and allow list sit side by side on both sides: one copy
            if (rc == KDB_OK && hipMemcpyAsync(d, h, L.in_span(), hipMemcpyHostToDevice, sl.stream) != hipSuccess) {
                kdb_set_error("staging copy to the device failed");
                rc = KDB_ERR_HIP;
            }
            queued = rc == KDB_OK;
            if (rc == KDB_OK) {
                const uint32_t *const d_k = hk ? reinterpret_cast<uint32_t *>(d + L.o_keys) : nullptr;
                rc = run(reinterpret_cast<float *>(d), allow_bits ? reinterpret_cast<uint64_t *>(d + L.o_allow) : nullptr,
                         reinterpret_cast<uint32_t *>(o_base + L.o_ids), reinterpret_cast<float *>(o_base + L.o_dist),
                         reinterpret_cast<uint32_t *>(o_base + L.o_cnt), sl.stream, B, d_k, hk ? d_k + B : nullptr);
            }
        }
        if (rc == KDB_OK && !direct && hipMemcpyAsync(h + L.o_ids, d + L.o_ids, L.out_span, hipMemcpyDeviceToHost, sl.stream) != hipSuccess) {
            kdb_set_error("staging copy from the device failed");
            rc = KDB_ERR_HIP;
        }
        lk.unlock();
        if (queued && hipStreamSynchronize(sl.stream) != hipSuccess && rc == KDB_OK) { // (queued copies read the slot's buffer: wait on errors too)
            kdb_set_error("hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
            rc = KDB_ERR_HIP;
        }
        if (rc == KDB_OK) {
            memcpy(out_ids, h + L.o_ids, (size_t)B * k * 4);
            memcpy(out_dist, h + L.o_dist, (size_t)B * k * dist_bytes);
            memcpy(out_count, h + L.o_cnt, (size_t)B * 4);
        }
        lk.lock();
    }
    sl.busy = false;
    idx->inflight--;
    kdb_launch_forming(idx, lk);
    idx->slot_cv.notify_all();
    return rc;
}
