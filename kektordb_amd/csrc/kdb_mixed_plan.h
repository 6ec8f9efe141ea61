// kdb_mixed_plan.h -- the rules of a search launch whose queries differ in k and efSearch (kdb_search_batch_mixed[_dev]):
// a query's effective ef, the capacity a launch needs for its largest one, when a query is valid in a launch, when a late caller
// may join a running open launch, and the output stride of a launch that stays open.
//
// ONE function states each rule: the host plans with them (kdb_api_calls.hip, kdb_api_query.hip), the kernels apply them per query (search_kernel.cuh,
// search_heap.hip), so the two cannot disagree.  Plain C++, no HIP header: host and device under hipcc, and
// tests/cpp/mixed_plan_test.cpp builds it alone.
#ifndef KDB_MIXED_PLAN_H
#define KDB_MIXED_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/kektor_hip.h"

#if defined(__HIPCC__)
#define KDB_MIXED_HD __host__ __device__
#else
#define KDB_MIXED_HD
#endif

constexpr uint32_t KDB_MIXED_GROUP_CAP = 256u;             // queries one combined launch may carry (= KDB_GROUP_CAP, kdb_internal.h)
constexpr size_t KDB_MIXED_PIN_DEFAULT = (size_t)4 << 20;  // what a slot's page-locked buffer may hold (KDB_HOST_PIN_MAX's default)
constexpr uint32_t KDB_MIXED_STRIDE_STEP = 16u;            // an open launch's stride: whole steps of this many results
// Concurrent callers combine across keys up to this effective ef; a caller above it combines with callers of its own key only, as
// before: one caller's ef must not decide whether the launch of all the others still fits LDS (1024: inside the large visited hash)
constexpr uint32_t KDB_MIXED_COMBINE_EF_MAX = 1024u;

// efSearch after the KDB_SEARCH_NEEDS_REFINE boost (hnsw_index.go:387-399): twice the ef, at least 80, at most 200, never less
// than the ef asked for
KDB_MIXED_HD constexpr uint32_t kdb_mixed_boosted_ef(uint32_t ef, bool needs_refine) {
    if (!needs_refine) return ef;
    uint32_t boosted = ef > 0x7fffffffu ? 0xffffffffu : 2u * ef;
    if (boosted < 80u) boosted = 80u;
    if (boosted > 200u) boosted = 200u;
    return boosted > ef ? boosted : ef;
}

// The ef a query is walked with: the boost first, then ef = max(efSearch, k) (hnsw_index.go:2377-2380)
KDB_MIXED_HD constexpr uint32_t kdb_mixed_effective_ef(uint32_t ef, uint32_t k, bool needs_refine) {
    const uint32_t e = kdb_mixed_boosted_ef(ef, needs_refine);
    return e < k ? k : e;
}

// Beam storage for an effective ef: 1, 2 or 4 register slots of 64 entries, 0 = the beam lives in LDS (kdb_beam_slots' rule:
// kdb_search_core.cuh checks the two against each other)
KDB_MIXED_HD constexpr int kdb_mixed_beam_class(uint32_t eff) { return eff <= 64u ? 1 : eff <= 128u ? 2 : eff <= 256u ? 4 : 0; }

// Capacity of a launch from its largest effective ef: the top of the register class (a smaller ef inside the class costs the same
// LDS and registers), the value itself for the LDS beam
KDB_MIXED_HD constexpr uint32_t kdb_mixed_ef_cap(uint32_t eff_max) {
    const int c = kdb_mixed_beam_class(eff_max);
    return c ? 64u * (uint32_t)c : eff_max;
}

// The predicate the kernels apply to every query of a mixed launch: k results fit the query's row of the output, its beam fits the
// launch's.  A query that fails it is answered with count 0 | KDB_MIXED_BAD_QUERY and never walked.
KDB_MIXED_HD constexpr bool kdb_mixed_query_valid(uint32_t k, uint32_t eff, uint32_t stride, uint32_t ef_cap) {
    return k != 0u && k <= stride && eff <= ef_cap;
}

// A late caller joins a RUNNING open launch (whose layout is never changed) if its answers fit the launch's rows, its walk the
// launch's beam, and the launch reads and writes what the caller expects (flags, bytes per distance)
KDB_MIXED_HD constexpr bool kdb_mixed_admit(uint32_t k, uint32_t eff, uint32_t flags, uint32_t dist_bytes, uint32_t stride, uint32_t ef_cap,
                                            uint32_t launch_flags, uint32_t launch_dist_bytes) {
    return kdb_mixed_query_valid(k, eff, stride, ef_cap) && flags == launch_flags && dist_bytes == launch_dist_bytes;
}

// What a slot's buffer holds for `cap_q` queries at this stride: queries | k and ef of every query | ids | distances | counts, every
// region rounded to 256 bytes, and the slack staged_layout keeps
KDB_MIXED_HD constexpr size_t kdb_mixed_slot_bytes(uint32_t cap_q, uint32_t dim, uint32_t stride, uint32_t dist_bytes) {
    return (size_t)cap_q * dim * 4u + (size_t)cap_q * 8u + (size_t)cap_q * stride * (4u + dist_bytes) + (size_t)cap_q * 4u + 4096u;
}

// Stride of a launch that will stay open, fixed when it is launched: the founders' largest k rounded up to whole steps of 16 (room for
// late callers that ask for a few more), never above ef_cap (no admitted query has a larger k: k <= effective ef <= ef_cap) -- and
// without the rounding when the buffer of KDB_MIXED_GROUP_CAP queries would then pass the pin limit.  0: not even the founders' own
// stride fits; such a launch is not kept open.
KDB_MIXED_HD constexpr uint32_t kdb_mixed_open_stride(uint32_t k_max, uint32_t ef_cap, uint32_t dim, uint32_t dist_bytes, size_t pin_max) {
    if (k_max == 0u || k_max > ef_cap) return 0u;
    uint32_t stride = (k_max + KDB_MIXED_STRIDE_STEP - 1u) / KDB_MIXED_STRIDE_STEP * KDB_MIXED_STRIDE_STEP;
    if (stride > ef_cap) stride = ef_cap;
    if (kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, dim, stride, dist_bytes) <= pin_max) return stride;
    return kdb_mixed_slot_bytes(KDB_MIXED_GROUP_CAP, dim, k_max, dist_bytes) <= pin_max ? k_max : 0u;
}

#endif
