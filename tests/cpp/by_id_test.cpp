// Index::GetVectors / Index::SearchSimilar (include/kektor_hip.hpp) against the calls they replace: one page of the loop of
// Gardener.findRedundantClusters (pkg/cognitive/gardener.go:803-869) -- VGetMany, then VSearchWithScores with every vector read --
// must give what the single by-id call gives.  Exit code 0 = pass, 77 = no GPU.
#include <cstdio>
#include <random>
#include <vector>

#include "kektor_hip.hpp"

static bool same(const std::vector<kektor::SearchResult> &a, const std::vector<kektor::SearchResult> &b) {
    if (a.size() != b.size()) return false;
    for (size_t j = 0; j < a.size(); j++)
        if (a[j].DocID != b[j].DocID || a[j].Score != b[j].Score) return false;
    return true;
}

int main() {
    if (kdb_hip_device_count() == 0) {
        try {
            kektor::hnsw::Index idx(16, KDB_METRIC_L2, KDB_PREC_F32, 8, 20, 100);
            std::printf("FAIL: index created without a device\n");
            return 1;
        } catch (const kektor::Error &e) {
            std::printf("no device: %s\n", e.what());
            return 77;
        }
    }
    const uint32_t n = 2000, dim = 16;
    const int k = 5;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::vector<float> X((size_t)n * dim);
    for (auto &x : X) x = U(rng);
    kektor::hnsw::Index idx(dim, KDB_METRIC_L2, KDB_PREC_F32, 8, 20, n);
    idx.UploadRows(1, n, X.data());
    idx.Build(n, 3, 256);
    int bad = 0;
    std::vector<uint32_t> ids;
    for (uint32_t i = 1; i <= 50; i++) ids.push_back(i); // (the corpus, graph and ids of host_mirror_test.cpp's self-match check)
    std::vector<uint8_t> found;
    const std::vector<float> V = idx.GetVectors(ids, &found);
    for (uint32_t i = 0; i < ids.size(); i++) {
        if (!found[i]) bad++;
        for (uint32_t j = 0; j < dim; j++)
            if (V[(size_t)i * dim + j] != X[(size_t)(ids[i] - 1) * dim + j]) bad++; // float32 rows come back as stored
    }
    for (int ef : {12, 100}) {
        const auto sim = idx.SearchSimilar(ids, k, ef);
        const auto sim_drop = idx.SearchSimilar(ids, k, ef, nullptr, true);
        for (uint32_t i = 0; i < ids.size(); i++) {
            const std::vector<float> q(V.begin() + (size_t)i * dim, V.begin() + (size_t)(i + 1) * dim);
            if (!same(sim[i], idx.SearchWithScores(q, k, nullptr, ef))) bad++;
            if (sim[i].size() != (size_t)k || sim[i][0].DocID != ids[i] || sim[i][0].Score != 0.0) bad++; // self ranks first
            const auto wide = idx.SearchWithScores(q, k + 1, nullptr, ef);                              // ... and is absent with dropSelf
            std::vector<kektor::SearchResult> want;
            for (const auto &r : wide)
                if (r.DocID != ids[i] && want.size() < (size_t)k) want.push_back(r);
            if (!same(sim_drop[i], want)) bad++;
            for (const auto &r : sim_drop[i])
                if (r.DocID == ids[i]) bad++;
        }
    }
    // ids that name no live node: zero rows, found 0, no results; the others of the same call are unaffected
    idx.Delete({777, 1999});
    {
        const std::vector<uint32_t> mixed = {0, 777, ids[0], n + 1, 0xffffffffu, 1999, ids[1]};
        std::vector<uint8_t> f;
        const std::vector<float> W = idx.GetVectors(mixed, &f);
        const auto sim = idx.SearchSimilar(mixed, k, 50);
        const auto alone = idx.SearchSimilar({ids[0], ids[1]}, k, 50);
        for (size_t i = 0; i < mixed.size(); i++) {
            const bool live = i == 2 || i == 6;
            if ((f[i] != 0) != live) bad++;
            if (!live) {
                if (!sim[i].empty()) bad++;
                for (uint32_t j = 0; j < dim; j++)
                    if (W[i * dim + j] != 0.f) bad++;
            }
        }
        if (!same(sim[2], alone[0]) || !same(sim[6], alone[1])) bad++;
    }
    idx.Close();
    if (!idx.SearchSimilar(ids, k, 50)[0].empty()) bad++; // closed index returns []
    std::printf(bad ? "FAIL %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
