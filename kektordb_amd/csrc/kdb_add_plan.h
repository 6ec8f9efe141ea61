// kdb_add_plan.h -- what every node of a kdb_index_add call finds, computed on the host before the first launch.
//
// The sequential Add (pkg/core/hnsw/hnsw_index.go:472-809) reads three things that earlier Adds of the same call changed: the
// level it may take (randomLevel caps at maxLevel + 1, :2620-2623), the entry point and maxLevel (:657-670 for the first node of
// an empty graph, :793-801 for a node above the top).  All three are a pure function of (entry, max_level, first_id, levels[]):
// no walk decides them.  So the chain of inserts needs no host synchronisation per node -- the host knows every launch's
// arguments up front.  Plain C++, no HIP: tests/cpp/add_plan_test.cpp checks it against the oracle on the CPU.
#ifndef KDB_ADD_PLAN_H
#define KDB_ADD_PLAN_H
#include <stdint.h>

struct KdbAddStep {
    uint8_t level;     // len(Connections)-1 of the node after the cap
    uint32_t entry;    // entry point the node finds (0: the graph is empty)
    int32_t max_level; // maxLevel the node finds (-1: the graph is empty -- the node becomes the entry point, no links)
};

// steps[i] for node first_id + i; *entry / *max_level: in = the index before the call, out = after it
static inline void kdb_add_plan(uint32_t *entry, int32_t *max_level, uint32_t first_id, const uint8_t *levels, uint32_t n, KdbAddStep *steps) {
    uint32_t ep = *entry;
    int32_t top = *max_level;
    for (uint32_t i = 0; i < n; i++) {
        int32_t lv = (int32_t)levels[i];
        if (lv > top + 1) lv = top + 1; // :2620-2623
        steps[i].level = (uint8_t)lv;
        steps[i].entry = top < 0 ? 0u : ep;
        steps[i].max_level = top;
        if (lv > top) { // :657-670 (empty graph), :793-801
            top = lv;
            ep = first_id + i;
        }
    }
    *entry = ep;
    *max_level = top;
}

// (node, level) lists the call writes: a node links on levels 0 .. min(its level, the maxLevel it finds); none on an empty graph
static inline uint64_t kdb_add_plan_lists(const KdbAddStep *steps, uint32_t n) {
    uint64_t lists = 0;
    for (uint32_t i = 0; i < n; i++)
        if (steps[i].max_level >= 0) lists += (uint64_t)((int32_t)steps[i].level < steps[i].max_level ? (int32_t)steps[i].level : steps[i].max_level) + 1u;
    return lists;
}
#endif
