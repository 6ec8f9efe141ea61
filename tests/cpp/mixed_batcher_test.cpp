// MicroBatcher and requests that differ in k and efSearch (include/kektor_hip.hpp).
//   * no GPU needed: over a test double WITHOUT SearchMixed the batcher keeps its (k, efSearch, allow list) keying -- every call the
//     double sees carries one k and one efSearch; over a double WITH SearchMixed the callers of one allow list share a group whatever
//     they ask for, every caller still gets the answer computed from ITS query with ITS k and efSearch, and a list that routes to the
//     exact scan keeps the old keying (the scan has one k per call);
//   * built with -DMIXED_BATCHER_GPU and run on a GPU: the same over a real index -- callers with one shared allow list and three
//     keys; every answer equals SearchWithScores for that caller alone, ids and scores bit for bit, in fewer launches than calls.
// Exit 0 = pass, 77 = no GPU (GPU build only).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "kektor_hip.hpp"

namespace {
using Results = std::vector<std::vector<kektor::SearchResult>>;
struct PlainDouble { // today's test double: no SearchMixed
    std::atomic<int> calls{0}, flat_calls{0};
    uint32_t Dim() const { return 8; }
    uint32_t Count() const { return 1000; }
    Results answer(const float *q, uint32_t B, int k, int tag) {
        std::this_thread::sleep_for(std::chrono::microseconds(300)); // a GPU call
        Results out(B);
        for (uint32_t b = 0; b < B; b++)
            for (int i = 0; i < k; i++) out[b].push_back({(uint32_t)q[(size_t)b * 8] * 10u + (uint32_t)i, (double)tag});
        return out;
    }
    Results SearchBatch(const float *q, uint32_t B, int k, const kektor::AllowList *, int ef) {
        calls++;
        return answer(q, B, k, ef);
    }
    Results FlatScanBatch(const float *q, uint32_t B, int k, const kektor::AllowList *) {
        flat_calls++;
        return answer(q, B, k, -1);
    }
};
struct MixingDouble : PlainDouble {
    std::atomic<int> mixed_calls{0}, mixed_with_two_keys{0};
    Results SearchMixed(const float *q, uint32_t B, const std::vector<int> &ks, const std::vector<int> &efs, const kektor::AllowList *) {
        mixed_calls++;
        std::this_thread::sleep_for(std::chrono::microseconds(300));
        Results out(B);
        bool two = false;
        for (uint32_t b = 0; b < B; b++) {
            if (ks[b] != ks[0] || efs[b] != efs[0]) two = true;
            for (int i = 0; i < ks[b]; i++) out[b].push_back({(uint32_t)q[(size_t)b * 8] * 10u + (uint32_t)i, (double)efs[b]});
        }
        if (two) mixed_with_two_keys++;
        return out;
    }
};

// 24 threads x 40 one-query calls, three keys, one shared list (wide), now and then the selective one; returns the number of wrong answers
template <class IndexT>
int run_callers(kektor::hnsw::BasicMicroBatcher<IndexT> &mb, const kektor::AllowList &wide, const kektor::AllowList &narrow) {
    static const int keys[3][2] = {{5, 20}, {10, 64}, {3, 130}};
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 24; t++)
        th.emplace_back([&, t] {
            for (int it = 0; it < 40; it++) {
                const int me = t * 100 + it;
                std::vector<float> q(8, 0.f);
                q[0] = (float)me;
                const int *key = keys[(t + it) % 3];
                const kektor::AllowList *al = it % 9 == 4 ? &narrow : &wide;
                auto r = mb.SearchWithScores(q, key[0], al, key[1]);
                const double want_tag = al == &narrow ? -1.0 : (double)key[1];
                if ((int)r.size() != key[0]) { bad++; continue; }
                for (int i = 0; i < key[0]; i++)
                    if (r[i].DocID != (uint32_t)me * 10u + (uint32_t)i || r[i].Score != want_tag) bad++;
            }
        });
    for (auto &x : th) x.join();
    return bad.load();
}

int cpu_half() {
    int bad = 0;
    kektor::AllowList wide(1000), narrow(1000);
    for (uint32_t i = 1; i <= 1000; i += 2) wide.Add(i);
    for (uint32_t i = 1; i <= 1000; i += 100) narrow.Add(i); // 1 % of the ids: routed to the exact scan
    {   // the old keying: a double without SearchMixed sees one (k, ef) per call -- run_callers checks every answer against ITS key
        PlainDouble idx;
        kektor::hnsw::BasicMicroBatcher<PlainDouble> mb(idx);
        bad += run_callers(mb, wide, narrow);
        const auto st = mb.stats();
        if (st.calls != 24 * 40 || st.mixedBatches != 0 || st.batches >= st.calls || st.flatBatches == 0) bad++;
        if (idx.calls.load() + idx.flat_calls.load() != (int)st.batches) bad++;
    }
    {   // the new one: one group per allow list
        MixingDouble idx;
        kektor::hnsw::BasicMicroBatcher<MixingDouble> mb(idx);
        bad += run_callers(mb, wide, narrow);
        const auto st = mb.stats();
        if (st.calls != 24 * 40 || st.mixedBatches == 0 || st.batches >= st.calls || st.flatBatches == 0) bad++;
        if (idx.mixed_calls.load() != (int)st.mixedBatches || idx.mixed_with_two_keys.load() == 0) bad++;
        if (idx.calls.load() != 0) bad++; // every walk of the shared list went out through SearchMixed
        if (idx.mixed_calls.load() + idx.flat_calls.load() != (int)st.batches) bad++;
    }
    return bad;
}

#ifdef MIXED_BATCHER_GPU
int gpu_half() {
    const uint32_t n = 3000, dim = 32;
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::vector<float> X((size_t)n * dim);
    for (float &x : X) x = u(rng);
    for (uint32_t c = 0; c < dim; c++) X[(size_t)40 * dim + c] = X[(size_t)7 * dim + c]; // (a duplicate row: a tie for the heap-order pass)
    kektor::hnsw::Index idx(dim, KDB_METRIC_L2, KDB_PREC_F32, 16, 100, n);
    idx.UploadRows(1, n, X.data());
    idx.Build(n, 3);
    kektor::AllowList half(n);
    for (uint32_t i = 1; i <= n; i++)
        if (i % 2 == 0 || i % 7 == 0) half.Add(i);
    static const int keys[3][2] = {{5, 20}, {10, 64}, {3, 130}};
    const int T = 16, IT = 30;
    std::vector<std::vector<float>> Q((size_t)T * IT, std::vector<float>(dim));
    for (auto &q : Q)
        for (float &x : q) x = u(rng);
    for (uint32_t c = 0; c < dim; c++) Q[3][c] = X[(size_t)7 * dim + c];
    std::vector<std::vector<kektor::SearchResult>> want(Q.size());
    for (size_t i = 0; i < Q.size(); i++) want[i] = idx.SearchWithScores(Q[i], keys[i % 3][0], &half, keys[i % 3][1]); // one by one
    uint64_t s0[10], s1[10], m0[4], m1[4];
    if (kdb_index_caller_stats(idx.handle(), s0) || kdb_index_mixed_stats(idx.handle(), m0)) return 1;
    kektor::hnsw::MicroBatcher mb(idx);
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            for (int it = 0; it < IT; it++) {
                const size_t i = (size_t)t * IT + it;
                auto r = mb.SearchWithScores(Q[i], keys[i % 3][0], &half, keys[i % 3][1]);
                if (r.size() != want[i].size() || r.empty()) { bad++; continue; }
                for (size_t j = 0; j < r.size(); j++)
                    if (r[j].DocID != want[i][j].DocID || r[j].Score != want[i][j].Score) bad++;
            }
        });
    for (auto &x : th) x.join();
    if (kdb_index_caller_stats(idx.handle(), s1) || kdb_index_mixed_stats(idx.handle(), m1)) return 1;
    const auto st = mb.stats();
    const uint64_t launches = s1[0] - s0[0];
    std::printf("gpu: calls %llu batches %llu mixed batches %llu launches %llu launches with two keys %llu bad %d\n", (unsigned long long)st.calls,
                (unsigned long long)st.batches, (unsigned long long)st.mixedBatches, (unsigned long long)launches, (unsigned long long)(m1[0] - m0[0]), bad.load());
    if (st.calls != (uint64_t)T * IT || st.mixedBatches == 0 || st.mixedBatches != st.batches) bad++;
    if (launches >= st.calls || launches != st.batches) bad++; // fewer launches than calls: one per batch
    if (m1[0] - m0[0] == 0) bad++;                             // ... and some of them carried more than one key
    return bad.load();
}
#endif
} // namespace

int main() {
    int bad = cpu_half();
#ifdef MIXED_BATCHER_GPU
    if (kdb_hip_device_count() == 0) {
        std::printf("no device\n");
        return 77;
    }
    bad += gpu_half();
#endif
    std::printf(bad ? "FAIL %d\n" : "ok %d\n", bad);
    return bad ? 1 : 0;
}
