// kdb_search_plan.h -- the launch decision of hnsw_search_kernel (search_kernel.cuh) as arithmetic: the class rules of a walk (beam
// storage, visited hash, un-mark list), the LDS bytes of a workgroup, and the ladder of kernel cells a launch tries in order.
//
// ONE function states each rule: the search launcher, the heap-order walk's plan (kdb_heap_plan.h), a mixed launch's capacity
// (kdb_mixed_plan.h) and the construction walks (kdb_walk_lds.h) all take them from here.  What needs the device -- the occupancy of
// a kernel at a footprint, the walk planes, the launch itself -- stays in search_kernel.cuh and search.hip.  Plain C++, no HIP
// header: tests/cpp/search_plan_test.cpp builds it alone and checks the footprint against a restatement of the kernel's own carve.
#ifndef KDB_SEARCH_PLAN_H
#define KDB_SEARCH_PLAN_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KDB_PLAN_HD __host__ __device__
#else
#define KDB_PLAN_HD
#endif

#define KDB_UP_MARK_CAP 256u               // upper-layer visited un-mark list (per wave, LDS); overflow -> full clear
#define KDB_SEARCH_LDS_LIMIT (160u * 1024u) // LDS of a CU: a footprint whose bytes + 16 pass it is refused

// beam slots needed for ef (the beam never holds more than ef entries); 0 = use the LDS beam
KDB_PLAN_HD constexpr int kdb_beam_slots(uint32_t ef) {
    if (ef <= 64) return 1; // one entry per lane: every beam operation stays inside one register
    if (ef <= 128) return 2;
    if (ef <= 256) return 4;
    return 0; // (six register slots, ef 257..384, lost to the LDS beam's one merge per hop: 1M x 768, k=100, 1024 queries, ef 384: 3.63 ms
              //  against 2.89 ms at ef 400 -- scripts/ef_probe.py, round 4; the slot count 6 is gone)
}

// LDS hash-set size (words) for ef; 0 = use the HBM bitset
KDB_PLAN_HD constexpr uint32_t kdb_vis_hash_size(uint32_t ef) {
    if (ef <= 100) return 2048; // the set holds the ~9*ef ids a query evaluates
    if (ef <= 260) return 4096;
    return 0;
}

// ... and for walks whose batch leaves LDS free (one round of waves at this footprint): ef 261 .. 1040
KDB_PLAN_HD constexpr uint32_t kdb_vis_hash_size_large(uint32_t ef) {
    if (ef <= 260) return 0;
    if (ef <= 520) return 8192;   // 32 KB: four waves per CU
    if (ef <= 1040) return 16384; // 64 KB: two waves per CU
    return 0;
}

// entries of the LDS beam (BS == 0) for an effective ef
KDB_PLAN_HD constexpr uint32_t kdb_search_beam_cap(uint32_t eff) { return ((eff + 2) + 63) / 64 * 64; }

// LDS bytes of one workgroup of hnsw_search_kernel, region by region in the order the kernel cuts them (the three-wave planes kernel
// puts the hash ahead of the pending list: the same sum).  wk: 64-bit distance keys (int8) -- one more word per beam / neighbour /
// pending entry; bs: register slots of the beam, 0 = the beam's three arrays of beam_cap entries live here; vis_words: words of the
// visited hash, 0 = the HBM bitset (the region is then its un-mark list); waves: per query (above 1: a latency mode)
KDB_PLAN_HD constexpr size_t kdb_search_lds_bytes(bool wk, uint32_t ld, int bs, uint32_t beam_cap, uint32_t nr_cap, uint32_t vis_words, uint32_t waves) {
    const size_t entry = wk ? 12 : 8;
    size_t off = 0;
    off += wk ? ((size_t)ld + 15) / 16 * 16 : (size_t)ld * 4;                       // the query: the packed int8 row, else float32 values
    if (bs == 0) off += (size_t)beam_cap * entry;                                   // beam_d, beam_id (, beam_lo)
    off += 64 * entry;                                                              // nb_id, nb_d (, nb_lo)
    if (waves > 1) off += 64;                                                       // ctl: what the waves of a query tell each other
    if (waves > 1 || bs >= 2) off += (size_t)64 * (size_t)(bs >= 2 ? bs : 1) * 8;   // ins_d, ins_id: scatter scratch of the one-pass insertion
    off += (size_t)nr_cap * entry;                                                  // nr_d, nr_id (, nr_lo): the pending list
    off += (size_t)(vis_words ? vis_words : KDB_UP_MARK_CAP) * 4;                   // marks: the hash table, or the un-mark list
    return off;
}
KDB_PLAN_HD constexpr bool kdb_search_lds_fits(size_t bytes) { return bytes + 16 <= KDB_SEARCH_LDS_LIMIT; }

// The latency modes of a multi-slot register beam have always been launched with 512 bytes more than the kernel cuts (the scatter
// scratch was counted once for the slots and once for the mode).  Kept: a byte less can move a batch-size threshold between two
// geometries at some row width.
#define KDB_SEARCH_WIDE_SLACK 512u

// One kernel cell a launch may take.  bounded: taken only by a batch of at most n_cu x resident workgroups of that kernel at that
// footprint (every query its own workgroup); the last rung of a ladder takes whatever is left.
struct KdbSearchRung {
    uint32_t hash;      // 1: visited set in LDS (migrating to the HBM bitset if it fills), 0: the HBM bitset
    uint32_t waves;     // per query: 4 / 2 = the latency modes (search_layer_wide), 1 = the throughput kernel
    uint32_t vis_words; // words of the hash, 0 with the bitset
    uint32_t lds;       // bytes of LDS per workgroup
    bool bounded;
    bool planes;        // this rung may run the planes kernel where the index has walk planes (kdb_planes_kernel)
};
#define KDB_SEARCH_RUNGS_MAX 6
struct KdbSearchLadder {
    int bs;            // kdb_beam_slots(eff)
    uint32_t beam_cap; // kdb_search_beam_cap(eff)
    uint32_t n;        // rungs; 0: refused -- the one-wave footprint (lds1) does not fit a CU's LDS
    size_t lds1;
    KdbSearchRung rung[KDB_SEARCH_RUNGS_MAX];
};

// The cells of a launch in the order they are tried, for (64-bit keys, columns of a stored row, effective ef, pending-list entries).
//   register beams (ef <= 256): the LDS hash with four waves per query, two, one.
//     Latency mode: a batch that leaves most of the chip idle gives every query four waves: wave 0 walks, the other three evaluate a
//     hop's rows (one HBM round trip per hop instead of three), wave 1 prepares the next node while wave 0 inserts
//     (search_layer_wide); same walk, same results, same counters -- as long as every query gets its own resident workgroup (512 at
//     768-d float32).  Twice as many queries than that: two waves per query -- the walker and one wave that prepares nodes and
//     evaluates rows.  The latency modes take a four times larger hash set (LDS is plentiful with one or two workgroups per CU): the
//     visited test is a compare-and-swap probe loop that ends when the slowest of 32 lanes has found its slot -- at a load below 7 %
//     that is two rounds, not three.  Round 5: the four-slot beam (ef 129 .. 256) too -- with the hash at its ordinary size there (the
//     enlarged one would leave two workgroups per CU).
//   LDS beam, ef 261 .. 1040: the visited set of a walk (~9 ef ids) still fits LDS when the batch leaves LDS free -- 32 KB (64 KB
//     above ef 520) per wave, four (two) waves per CU.  A batch that fits ONE round of such waves takes the LDS hash and loses the HBM
//     bitset's dependent round trip per hop (atomicOr at the device's coherence point); larger batches keep the bitset, whose eight
//     waves per CU hide more latency than the hash saves.  (The hash still migrates to the bitset if a walk outgrows it.)  Round 5:
//     the latency mode for the LDS beam as well (k = 100 / ef = 400 on 1024 queries: every query its own four waves -- the rows of a
//     hop in one round trip, the visit of the next node beside the one-merge insertion).
//   beyond the large hash (ef > 1040, or a batch too large for it): the latency mode over the HBM bitset -- wave 1 owns the bitset,
//     the walker never waits for its atomics -- then the one-wave bitset kernel.
// A bounded rung whose footprint does not fit a CU's LDS is left out.
// (Round 6 built "two queries per wave" for short rows -- docs/probes/r06_search_pair.cuh: one walk per 32-lane half, every
// wave-uniform value of this walk kept per half, ballots split, cross-lane reads inside the half; bit-exact at the first run -- and
// measured it on the GloVe-100 shape, 8192 queries: efS 20 0.450 ms against 0.455 here, efS 100 1.27 ms against 0.93: what is scalar
// bookkeeping for one query per wave becomes vector work per half (a half-ballot is five instructions, not one), and a four-slot
// beam per half triples the insertion: more instructions per QUERY, not fewer.  Not shipped: no rung for it.)
KDB_PLAN_HD static inline KdbSearchLadder kdb_search_ladder(bool wk, uint32_t ld, uint32_t eff, uint32_t nr_cap) {
    KdbSearchLadder l{};
    l.bs = kdb_beam_slots(eff);
    l.beam_cap = kdb_search_beam_cap(eff);
    const uint32_t hsize = l.bs ? kdb_vis_hash_size(eff) : 0u; // (never 0 for a register beam: ef <= 256)
    l.lds1 = kdb_search_lds_bytes(wk, ld, l.bs, l.beam_cap, nr_cap, hsize, 1u);
    if (!kdb_search_lds_fits(l.lds1)) return l;
    auto rung = [&](uint32_t words, uint32_t waves, bool last) {
        const size_t b = kdb_search_lds_bytes(wk, ld, l.bs, l.beam_cap, nr_cap, words, waves) + (l.bs >= 2 && waves > 1u ? KDB_SEARCH_WIDE_SLACK : 0u);
        if (last || kdb_search_lds_fits(b)) l.rung[l.n++] = KdbSearchRung{words ? 1u : 0u, waves, words, (uint32_t)b, !last, last && l.bs != 0};
    };
    if (l.bs) {
        const uint32_t hw = l.bs == 4 ? hsize : (hsize * 4u > 16384u ? 16384u : hsize * 4u);
        rung(hw, 4u, false), rung(hw, 2u, false), rung(hsize, 1u, true);
        return l;
    }
    const uint32_t hbig = kdb_vis_hash_size_large(eff);
    if (hbig) rung(hbig, 4u, false), rung(hbig, 2u, false), rung(hbig, 1u, false);
    rung(0u, 4u, false), rung(0u, 2u, false), rung(0u, 1u, true);
    return l;
}

#endif
