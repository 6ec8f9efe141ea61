// consensus_host / Index::Consensus / Index::BeliefState (include/kektor_hip.hpp).
//   consensus_test host IN OUT   no device needed: consensus_host on every case of IN, the raw results to OUT for
//                                tests/test_consensus_host.py to compare with its numpy restatement bit for bit.
//                                IN:  u32 cases, then per case u32 n, u32 dim, u32 has_query, n * dim floats[, dim floats]
//                                OUT: per case kdb_consensus (32 bytes), dim floats (centroid)[, n doubles (similarity)],
//                                     (n + 1)^2 doubles (gram)
//   consensus_test               on the device: Index::Consensus on id lists must equal consensus_host on the vectors GetVectors reads
//                                for those ids -- Engine.VBeliefState's own order of work (pkg/engine/epistemic.go:45-124) -- and
//                                Index::BeliefState must equal SearchWithScores followed by that.  Exit 0 = pass, 77 = no GPU.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kektor_hip.hpp"

static_assert(sizeof(kdb_consensus) == 32, "kdb_consensus is 32 bytes");

static int host_mode(const char *in, const char *out) {
    FILE *f = std::fopen(in, "rb"), *g = std::fopen(out, "wb");
    if (!f || !g) return 2;
    uint32_t cases = 0;
    if (std::fread(&cases, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t h[3];
        if (std::fread(h, 4, 3, f) != 3) return 2;
        std::vector<float> rows((size_t)h[0] * h[1]), q(h[1]);
        if (!rows.empty() && std::fread(rows.data(), 4, rows.size(), f) != rows.size()) return 2;
        if (h[2] && std::fread(q.data(), 4, q.size(), f) != q.size()) return 2;
        const kektor::ConsensusResult r = kektor::consensus_host(rows.data(), h[0], h[1], h[2] ? q.data() : nullptr, true);
        std::fwrite(&r.rec, sizeof r.rec, 1, g);
        std::fwrite(r.centroid.data(), 4, r.centroid.size(), g);
        if (h[2]) std::fwrite(r.similarity.data(), 8, r.similarity.size(), g);
        std::fwrite(r.gram.data(), 8, r.gram.size(), g);
    }
    std::fclose(f);
    return std::fclose(g) ? 2 : 0;
}

static bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }
// The float64 sums are the same on both sides; behind them lie one sqrt product, one divide and a sum of at most 64 squares, so 2^-46
// covers a device sqrt or divide that is one ulp off.  The score divides by max_pair^2 (>= 0.05^2 asserted): 1e-10.
static const double TOL = 1.0 / 70368744177664.0;
static bool near(double a, double b, double tol = TOL) { return a == b || std::fabs(a - b) <= tol; }
static bool near_rec(const kdb_consensus &a, const kdb_consensus &b) {
    if (a.n_active > 1 && !(b.max_pair >= 0.05)) return false;
    return near(a.score, b.score, 1e-10) && near(a.variance, b.variance) && near(a.max_pair, b.max_pair) && a.n_found == b.n_found && a.n_active == b.n_active;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::strcmp(argv[1], "host") == 0) return host_mode(argv[2], argv[3]);
    if (kdb_hip_device_count() == 0) {
        try {
            kektor::hnsw::Index idx(16, KDB_METRIC_COSINE, KDB_PREC_F32, 8, 20, 100);
            std::printf("FAIL: index created without a device\n");
            return 1;
        } catch (const kektor::Error &e) {
            std::printf("no device: %s\n", e.what());
            return 77;
        }
    }
    const uint32_t n = 2000, dim = 40, stride = 12;
    std::mt19937 rng(11);
    std::normal_distribution<float> N(0.f, 1.f);
    std::vector<float> X((size_t)n * dim);
    for (auto &x : X) x = N(rng);
    for (uint32_t i = 0; i < n; i++) { // stored form of a cosine index: unit rows
        double s = 0;
        for (uint32_t j = 0; j < dim; j++) s += (double)X[(size_t)i * dim + j] * X[(size_t)i * dim + j];
        for (uint32_t j = 0; j < dim; j++) X[(size_t)i * dim + j] = (float)(X[(size_t)i * dim + j] / std::sqrt(s));
    }
    kektor::hnsw::Index idx(dim, KDB_METRIC_COSINE, KDB_PREC_F32, 8, 20, n);
    idx.UploadRows(1, n, X.data());
    idx.Build(n, 3, 256);
    idx.Delete({5, 1500});
    int bad = 0;
    // 1. id lists: live ids, a deleted one, 0, an id above count, a repeat
    const uint32_t B = 9;
    std::vector<uint32_t> ids((size_t)B * stride), counts(B);
    std::vector<float> Q((size_t)B * dim);
    for (auto &x : Q) x = N(rng);
    for (uint32_t b = 0; b < B; b++) {
        counts[b] = b == 0 ? 0 : (b == 1 ? 1 : 2 + (b * 5) % (stride - 1));
        for (uint32_t i = 0; i < stride; i++) ids[(size_t)b * stride + i] = 1 + (uint32_t)(rng() % n);
        if (b >= 3) ids[(size_t)b * stride] = b == 3 ? 5u : b == 4 ? 0u : b == 5 ? n + 1 : ids[(size_t)b * stride + 1];
    }
    std::vector<double> sim;
    std::vector<float> cen;
    const std::vector<kdb_consensus> got = idx.Consensus(ids.data(), B, stride, counts.data(), Q.data(), nullptr, &sim, &cen);
    for (uint32_t b = 0; b < B; b++) {
        std::vector<uint32_t> lst(ids.begin() + (size_t)b * stride, ids.begin() + (size_t)b * stride + counts[b]);
        std::vector<uint8_t> found;
        const std::vector<float> V = idx.GetVectors(lst, &found); // VGet per candidate ...
        std::vector<float> rows;
        std::vector<uint32_t> pos;
        for (uint32_t i = 0; i < lst.size(); i++)
            if (found[i]) { // ... `continue` for the ones that are gone (epistemic.go:56)
                rows.insert(rows.end(), V.begin() + (size_t)i * dim, V.begin() + (size_t)(i + 1) * dim);
                pos.push_back(i);
            }
        const kektor::ConsensusResult want = kektor::consensus_host(rows.data(), (uint32_t)pos.size(), dim, Q.data() + (size_t)b * dim);
        if (got[b].n_found != pos.size() || got[b].n_active != pos.size()) bad++;
        if (!near_rec(got[b], want.rec)) bad++;
        if (!same_bits(cen.data() + (size_t)b * dim, want.centroid.data(), (size_t)dim * 4)) bad++;
        for (uint32_t i = 0, p = 0; i < stride; i++) {
            const bool live = p < pos.size() && pos[p] == i;
            const double w = live ? want.similarity[p] : -1.0;
            if (!near(sim[(size_t)b * stride + i], w)) bad++;
            if (live) p++;
        }
    }
    if (got[0].score != 0.0 || got[1].score != 1.0 || got[1].variance != 0.0) bad++;
    // 2. BeliefState = SearchWithScores, then the consensus of the results
    for (int k : {1, 10, 70}) {
        const std::vector<float> q(Q.begin(), Q.begin() + dim);
        const auto bs = idx.BeliefState(q, k);
        const int kk = k > 50 ? 50 : k; // "Safety cap" (epistemic.go:30-32)
        const auto res = idx.SearchWithScores(q, kk, nullptr, 100);
        if (!bs.ok || bs.nodes.size() != res.size()) bad++;
        std::vector<uint32_t> lst;
        for (size_t i = 0; i < res.size() && i < bs.nodes.size(); i++) {
            if (res[i].DocID != bs.nodes[i].DocID || res[i].Score != bs.nodes[i].Score) bad++;
            lst.push_back(res[i].DocID);
        }
        const std::vector<float> V = idx.GetVectors(lst);
        const kektor::ConsensusResult want = kektor::consensus_host(V.data(), (uint32_t)lst.size(), dim, q.data());
        if (!near_rec(bs.consensus, want.rec)) bad++;
        if (bs.similarities.size() != want.similarity.size()) bad++;
        else
            for (size_t i = 0; i < want.similarity.size(); i++)
                if (!near(bs.similarities[i], want.similarity[i])) bad++;
    }
    idx.Close();
    if (idx.BeliefState(std::vector<float>(dim, 1.f), 10).ok) bad++; // closed index
    std::printf(bad ? "FAIL %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
