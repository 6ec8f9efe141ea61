// Index::CompileFilter / EvalFilters / SearchFiltered (include/kektor_hip.hpp) on the documents of the reference's own filter tests
// (tests/golden/filter_kats.json; tests/test_cpp_filter.py writes them, the schema a mirror would keep and the ids the plain-Python
// FindIDsByFilter expects into the case file):  filter_mirror_test CASES.  CompileFilter needs no device and is checked first;
// exit code 0 = pass, 77 = no GPU (after the host half passed).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "kektor_hip.hpp"

using kektor::hnsw::Index;

struct Case {
    std::string filter;
    std::set<uint32_t> want;
};

static std::string line(std::ifstream &f) {
    std::string s;
    std::getline(f, s);
    return s;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    // n | slots: "kind slot" + n values | keys: "f64slot codeslot ndict" + key + (code, string) pairs | cases: filter + "m id ..."
    const uint32_t n = (uint32_t)std::stoul(line(f));
    const uint32_t n_slots = (uint32_t)std::stoul(line(f));
    struct Col {
        uint32_t kind, slot;
        std::vector<double> f64;
        std::vector<uint32_t> code;
    };
    std::vector<Col> cols(n_slots);
    for (Col &c : cols) {
        std::istringstream h(line(f)), v(line(f));
        h >> c.kind >> c.slot;
        for (uint32_t i = 0; i < n; i++) {
            std::string tok;
            v >> tok;
            if (c.kind == KDB_COL_F64) c.f64.push_back(tok == "nan" ? std::nan("") : std::stod(tok));
            else c.code.push_back((uint32_t)std::stoul(tok));
        }
    }
    Index::FilterSchema schema;
    const uint32_t n_keys = (uint32_t)std::stoul(line(f));
    for (uint32_t i = 0; i < n_keys; i++) {
        std::istringstream h(line(f));
        Index::FilterKey key;
        uint32_t nd = 0;
        h >> key.f64Slot >> key.codeSlot >> nd;
        const std::string name = line(f);
        for (uint32_t j = 0; j < nd; j++) {
            const uint32_t code = (uint32_t)std::stoul(line(f));
            key.dict[line(f)] = code;
        }
        schema[name] = key;
    }
    std::vector<Case> cases((size_t)std::stoul(line(f)));
    for (Case &c : cases) {
        c.filter = line(f);
        std::istringstream v(line(f));
        uint32_t m = 0, id = 0;
        v >> m;
        for (uint32_t j = 0; j < m; j++) {
            v >> id;
            c.want.insert(id);
        }
    }
    int bad = 0;
    // ---- the host half: every filter compiles to a well-formed program; the reference's errors throw
    std::vector<Index::FilterProgram> progs;
    for (const Case &c : cases) {
        progs.push_back(Index::CompileFilter(c.filter, schema));
        if (progs.back().empty() || !(progs.back().back().flags & KDB_FT_END_BLOCK)) bad++;
    }
    for (const char *broken : {"", "no-operator-here", "year < abc", "year = nan"}) {
        try {
            (void)Index::CompileFilter(broken, schema);
            bad++;
        } catch (const kektor::Error &) {
        }
    }
    {   // age = "10" on a key with both columns: two alternatives, the lenient union
        Index::FilterSchema s2;
        s2["age"].f64Slot = 1, s2["age"].codeSlot = 2, s2["age"].dict["10"] = 4;
        const auto p = Index::CompileFilter("age != \"10\"", s2);
        if (p.size() != 2 || p[0].op != KDB_FOP_F64_EQ || p[0].flags != (KDB_FT_OR_NEXT | KDB_FT_NOT) || p[0].value != 10.0 || p[1].op != KDB_FOP_CODE_EQ ||
            p[1].code != 4 || p[1].col != 2 || p[1].flags != KDB_FT_END_BLOCK)
            bad++;
        const auto q = Index::CompileFilter("nokey<3 OR age='x'", s2);
        if (q.size() != 2 || q[0].op != KDB_FOP_NEVER || q[0].flags != KDB_FT_END_BLOCK || q[1].op != KDB_FOP_NEVER) bad++;
    }
    if (bad) {
        std::printf("FAILED (host half): %d\n", bad);
        return 1;
    }
    if (kdb_hip_device_count() == 0) {
        try {
            Index idx(16, KDB_METRIC_L2, KDB_PREC_F32, 8, 20, 100);
            std::printf("FAIL: index created without a device\n");
            return 1;
        } catch (const kektor::Error &e) {
            std::printf("no device: %s\n", e.what());
            return 77;
        }
    }
    // ---- the device half: the documents as an index of n distinct rows, built by the sequential Add
    const uint32_t dim = 16;
    const int k = 16;
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::vector<float> X((size_t)n * dim);
    for (auto &x : X) x = U(rng);
    Index idx(dim, KDB_METRIC_L2, KDB_PREC_F32, 8, 20, n + 4);
    idx.UploadRows(1, n, X.data());
    const std::vector<uint8_t> levels(n, 0);
    idx.Add(1, levels.data(), n);
    for (const Col &c : cols) idx.SetColumn(c.slot, c.kind, 1, n, c.kind == KDB_COL_F64 ? (const void *)c.f64.data() : (const void *)c.code.data());
    std::vector<uint32_t> cards;
    const std::vector<kektor::AllowList> lists = idx.EvalFilters(progs, &cards);
    for (size_t p = 0; p < cases.size(); p++) {
        if (cards[p] != cases[p].want.size()) bad++;
        for (uint32_t id = 0; id <= n; id++)
            if (lists[p].Contains(id) != (cases[p].want.count(id) != 0)) bad++;
    }
    // one query per program plus one without a filter; every allowed document fits k, so the answer IS the set
    const uint32_t B = (uint32_t)cases.size() + 1;
    std::vector<float> Q((size_t)B * dim);
    for (auto &x : Q) x = U(rng);
    std::vector<uint32_t> poq;
    for (uint32_t b = 0; b + 1 < B; b++) poq.push_back(b);
    poq.push_back(KDB_NO_FILTER);
    std::vector<uint8_t> routes;
    const auto res = idx.SearchFiltered(Q.data(), B, k, 100, progs, poq, 0.1, &routes, &cards);
    for (uint32_t b = 0; b < B; b++) {
        std::set<uint32_t> got;
        for (const auto &r : res[b]) got.insert(r.DocID);
        if (got.size() != res[b].size()) bad++;
        if (b + 1 == B) {
            if (got.size() != n || routes[b] != 0) bad++;
            continue;
        }
        const Case &c = cases[b];
        if (got != c.want) {
            std::printf("filter %s: %zu ids, expected %zu\n", c.filter.c_str(), got.size(), c.want.size());
            bad++;
        }
        const uint8_t want_route = c.want.empty() ? 2 : ((double)c.want.size() < 0.1 * n ? 1 : 0);
        if (routes[b] != want_route || cards[b] != c.want.size()) bad++;
        // ... and bit for bit the single-list calls' answers
        const std::vector<float> q(Q.begin() + (size_t)b * dim, Q.begin() + (size_t)(b + 1) * dim);
        if (want_route == 2) continue;
        const auto alone = want_route == 1 ? idx.FlatScanBatch(q.data(), 1, k, &lists[b])[0] : idx.SearchWithScores(q, k, &lists[b], 100);
        if (alone.size() != res[b].size()) bad++;
        for (size_t j = 0; j < alone.size() && j < res[b].size(); j++)
            if (alone[j].DocID != res[b][j].DocID || alone[j].Score != res[b][j].Score) bad++;
    }
    if (bad) {
        std::printf("FAILED: %d\n", bad);
        return 1;
    }
    std::printf("ok: %zu filters\n", cases.size());
    return 0;
}
