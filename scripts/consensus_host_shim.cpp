// The CPU leg of scripts/consensus_probe.py: consensus_host (include/kektor_hip.hpp) over B lists of n decoded rows each, on
// `threads` threads, behind one C symbol so that the probe can call it from the process that runs the device legs.
#include <thread>
#include <vector>

#include "kektor_hip.hpp"

extern "C" int consensus_host_many(const float *rows, const uint32_t *counts, uint32_t B, uint32_t n, uint32_t dim, const float *queries,
                                   uint32_t threads, kdb_consensus *out, double *similarity) {
    auto work = [&](uint32_t t) {
        for (uint32_t b = t; b < B; b += threads) {
            const kektor::ConsensusResult r = kektor::consensus_host(rows + (size_t)b * n * dim, counts[b], dim, queries + (size_t)b * dim);
            out[b] = r.rec;
            for (uint32_t i = 0; i < counts[b]; i++) similarity[(size_t)b * n + i] = r.similarity[i];
        }
    };
    if (threads <= 1) {
        threads = 1;
        work(0);
        return 0;
    }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < threads; t++) th.emplace_back(work, t);
    for (auto &x : th) x.join();
    return 0;
}
