// kdb_walk_lds.h -- the LDS of one walking wave of graph construction, and of a workgroup that scores ids against a stored row.
//
// ONE function cuts the walk's LDS: the host sizes the launch from it and the kernel takes its pointers from it, so the two
// cannot disagree by a word.  Plain C++, no HIP header: host and device under hipcc, and tests/cpp/walk_plan_test.cpp builds it
// alone.
#ifndef KDB_WALK_LDS_H
#define KDB_WALK_LDS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define KDB_WALK_HD __host__ __device__
#else
#define KDB_WALK_HD
#endif

#define KDB_WALK_MARKS 256u // un-mark list of the upper layers (KDB_UP_MARK_CAP)

// NrList: a walk can never hold more of them than the index has deleted nodes (+ the entry point when a filter excludes it), so
// up to 2047 deleted nodes the list cannot overflow; beyond that it holds the 2048 nearest pending ones and counts what it drops
// (kdb_counters.n_dropped)
KDB_WALK_HD static inline uint32_t kdb_nr_cap(uint32_t n_deleted) {
    return ((n_deleted < 2047u ? n_deleted : 2047u) + 1u + 3u) & ~3u; // traversal-only candidates (deleted nodes)
}

// register slots of 64 beam entries for efConstruction, 0 = the beam lives in LDS: kdb_beam_slots' rule with one slot promoted to
// two (kdb_graph_build.cuh asserts the agreement at every boundary; this header takes no HIP include and cannot call it)
KDB_WALK_HD constexpr uint32_t kdb_walk_bs(uint32_t efc) { return efc <= 128 ? 2u : efc <= 256 ? 4u : 0u; }

// Byte offsets, in this order: query row | beam_d | beam_id | beam_lo | nr_d | nr_id | nr_lo | nb_id | nb_d | nb_lo | marks.
// A region the walk does not have is empty and shares its offset with the one behind it: the beam is in LDS only when bs == 0
// (efConstruction above 256; up to there it lives in 2 or 4 register slots of 64 entries -- kdb_beam_slots' rule, one slot
// promoted to two), the *_lo arrays (low words of the 64-bit distance keys) are int8's.
struct KdbWalkLds {
    uint32_t beam_cap, bs, nr_cap;
    uint32_t q, beam_d, beam_id, beam_lo, nr_d, nr_id, nr_lo, nb_id, nb_d, nb_lo, marks;
    uint32_t bytes;
};

// the cut for given capacities.  The kernels call this half themselves, with (bs, beam_cap, nr_cap) as the host's plan has them:
// i8 and bs are template constants there, so the offsets stay expressions of ld and the two capacities (a plan passed whole as
// a kernel argument costs the walk kernels 3 to 10 VGPRs: a dozen more scalars live across the walk, spilled into vector lanes)
KDB_WALK_HD static inline KdbWalkLds kdb_walk_lds_cut(bool i8, uint32_t ld, uint32_t bs, uint32_t beam_cap, uint32_t nr_cap) {
    KdbWalkLds w;
    w.beam_cap = beam_cap;
    w.bs = bs;
    w.nr_cap = nr_cap;
    const uint32_t beam = w.bs == 0 ? w.beam_cap * 4 : 0, nr = w.nr_cap * 4, lo = i8 ? 1 : 0;
    uint32_t off = 0;
    auto take = [&off](uint32_t bytes) { const uint32_t o = off; off += bytes; return o; };
    w.q = take(i8 ? ld : ld * 4);
    w.beam_d = take(beam);
    w.beam_id = take(beam);
    w.beam_lo = take(beam * lo);
    w.nr_d = take(nr);
    w.nr_id = take(nr);
    w.nr_lo = take(nr * lo);
    w.nb_id = take(64 * 4);
    w.nb_d = take(64 * 4);
    w.nb_lo = take(64 * 4 * lo);
    w.marks = take(KDB_WALK_MARKS * 4);
    w.bytes = off;
    return w;
}

// the plan of a walk: ld columns per stored row (int8: a multiple of 16, the packed row itself is the query; else f32 values),
// efConstruction, deleted nodes in the index
KDB_WALK_HD static inline KdbWalkLds kdb_walk_lds(bool i8, uint32_t ld, uint32_t efc, uint32_t n_deleted) {
    const uint32_t beam_cap = ((efc + 64 + 1) + 63) / 64 * 64;
    return kdb_walk_lds_cut(i8, ld, kdb_walk_bs(efc), beam_cap, kdb_nr_cap(n_deleted));
}

// Behind the prune tiles of a workgroup that scores ids against a stored row (four waves, a chunk of 64 ids each):
// w_d[4][64] distances | w_lo[4][64] their low words (int8) | the row as the query (packed int8, else f32) + 64 bytes of slack
struct KdbScoreTail {
    uint32_t w_d, w_lo, tq, bytes;
};
KDB_WALK_HD static inline KdbScoreTail kdb_score_tail(bool i8, uint32_t ld) {
    return KdbScoreTail{0u, 4u * 64u * 4u, 2u * 4u * 64u * 4u, 2048u + (i8 ? ld : ld * 4u) + 64u};
}
#endif
