// kdb_heap_plan.h -- what one wave of the heap-order walk (heap_walk_kernel, search_heap.hip) keeps in LDS and how much of its
// candidate heap spills to HBM: the visited hash, whether the result heap lives in registers, the candidate heap's capacity
// (cap_c), the part of it kept on chip (nl_c) and the LDS bytes per workgroup.
//
// The arithmetic of kdb_heap_walk_plan and nothing else: the occupancy query, the grid and the scratch of the tails stay in
// search_heap.hip.  Plain C++, no HIP header: host code under hipcc, and tests/cpp/heap_plan_test.cpp builds it alone and
// checks the footprint against a restatement of the kernel's own carve.
#ifndef KDB_HEAP_PLAN_H
#define KDB_HEAP_PLAN_H
#include <initializer_list>
#include <stddef.h>
#include <stdint.h>

#define KDB_HEAP_MARKS 256u              // un-mark list of the upper layers when the visited set is the HBM bitset (KDB_UP_MARK_CAP)
#define KDB_HEAP_LDS_LIMIT (160u * 1024u) // LDS of a CU: a plan whose lds + 16 passes it is refused

struct KdbHeapPlan {
    uint32_t hsize;    // words of the LDS visited hash (0: the HBM bitset)
    uint32_t nl_c;     // candidate-heap entries in LDS
    uint32_t cap_c;    // ... and in all (the rest in HBM scratch, per workgroup)
    uint32_t grid;     // workgroups (one wave each)
    uint32_t reg_results; // the result heap lives in registers (ef + 2 <= 64)
    size_t lds;        // bytes of LDS per workgroup
    size_t tail_bytes; // HBM scratch of all workgroups' candidate-heap tails
};

// words of the LDS visited hash for an effective ef, 0 = the HBM bitset alone: kdb_vis_hash_size's rule (kdb_search_core.cuh;
// search_heap.hip asserts the agreement at every boundary -- this header takes no HIP include and cannot call it)
constexpr uint32_t kdb_heap_hash_words(uint32_t eff) { return eff <= 100u ? 2048u : eff <= 260u ? 4096u : 0u; }

// bytes of one heap entry: id, key, and the low word of a 64-bit key (int8)
constexpr size_t kdb_heap_entry_bytes(bool wk) { return wk ? 12 : 8; }

// LDS of everything but the candidate heap: the query | nb_id, nb_d (, nb_lo) of 64 entries | the hash or the un-mark list | the
// result heap (ef + 2 entries) unless it is in registers | the drain arrays (ef + 2 entries)
inline size_t kdb_heap_fixed_lds(bool wk, uint32_t ld, uint32_t eff, uint32_t hsize, bool reg_results) {
    const size_t ew = kdb_heap_entry_bytes(wk);
    return (wk ? ((size_t)ld + 15) / 16 * 16 : (size_t)ld * 4) + 64 * (wk ? 12 : 8) + (hsize ? (size_t)hsize * 4 : KDB_HEAP_MARKS * 4) +
           (reg_results ? 1 : 2) * (size_t)(eff + 2u) * ew;
}

// HBM scratch of `grid` workgroups' candidate-heap tails
inline size_t kdb_heap_tail_bytes(uint32_t grid, uint32_t cap_c, uint32_t nl_c) { return (size_t)grid * (size_t)(cap_c - nl_c) * 12u; }

// LDS per wave sized FROM ef -- the visited hash of the fast walk, the result heap (ef + 2), and as much of the candidate heap as
// lets eight waves share a CU (about 8 ef entries; it holds every accepted neighbour of a layer search minus one pop per hop: a few
// ef at its largest) -- so that a few thousand tied queries all walk at once; the rest of the candidate heap (up to cap_c entries:
// 16 ef, at least 2048) in HBM scratch, per workgroup.
// wk: 64-bit keys (int8); ld: columns of a stored row; count: nodes of the index; eff: the effective ef (max(ef, k)).
// Fills hsize, reg_results, cap_c, nl_c and lds (grid and tail_bytes: 0).  false: the footprint does not fit a CU's LDS.
inline bool kdb_heap_plan_lds(bool wk, uint32_t ld, uint32_t count, uint32_t eff, KdbHeapPlan *out) {
    const size_t ew = kdb_heap_entry_bytes(wk);
    KdbHeapPlan p{};
    p.hsize = kdb_heap_hash_words(eff); // 2048 / 4096 words up to ef 260, beyond: the HBM bitset
    p.reg_results = p.hsize != 0 && eff + 2u <= 64u; // the result heap in registers (entry i in lane i)
    const size_t fixed = kdb_heap_fixed_lds(wk, ld, eff, p.hsize, p.reg_results != 0);
    const uint64_t cap64 = (uint64_t)16u * eff > 2048u ? (uint64_t)16u * eff : 2048u;
    p.cap_c = (uint32_t)(cap64 < (uint64_t)count + 2u ? cap64 : (uint64_t)count + 2u); // (a heap never holds more entries than there are nodes)
    const size_t want = fixed + (size_t)(8u * eff > 64u ? 8u * eff : 64u) * ew;
    size_t tier = 0;
    for (size_t waves : {8, 6, 4, 3, 2}) {
        const size_t t = (160u * 1024u) / waves - 512u;
        if (t >= want) {
            tier = t;
            break;
        }
    }
    if (!tier) tier = fixed + 64 * ew + 64 < 158u * 1024u ? (want < 158u * 1024u ? want : 158u * 1024u) : fixed + 64 * ew;
    size_t n = tier > fixed ? (tier - fixed) / ew : 64;
    if (n > 4095) n = 4095; // twelve levels of the heap on chip
    if (n < 64) n = 64;
    if (n > p.cap_c) n = p.cap_c;
    p.nl_c = (uint32_t)n;
    p.lds = fixed + (size_t)p.nl_c * ew;
    *out = p;
    return p.lds + 16 <= KDB_HEAP_LDS_LIMIT;
}

#endif
