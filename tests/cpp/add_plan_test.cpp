// The plan of kdb_index_add (kektordb_amd/csrc/kdb_add_plan.h) against cases recorded from the oracle's sequential Add: the capped
// level of every node and the entry point / maxLevel after it.  Stand-alone (the header only), built with -fsanitize=address,undefined.
// Case file (text): n_cases, then per case: entry max_level first_id n, then n lines: level_asked level_kept entry_after max_after.
#include "kdb_add_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("FAIL case %d: ", c);     \
            std::printf(__VA_ARGS__);             \
            std::printf("\n");                    \
            return 1;                             \
        }                                         \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_cases = 0;
    if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
    long nodes = 0;
    for (int c = 0; c < n_cases; c++) {
        unsigned entry0, first, n;
        int max0;
        if (std::fscanf(f, "%u %d %u %u", &entry0, &max0, &first, &n) != 4) return 2;
        std::vector<uint8_t> asked(n);
        std::vector<unsigned> kept(n), entry_after(n);
        std::vector<int> max_after(n);
        for (unsigned i = 0; i < n; i++) {
            unsigned a;
            if (std::fscanf(f, "%u %u %u %d", &a, &kept[i], &entry_after[i], &max_after[i]) != 4) return 2;
            asked[i] = (uint8_t)a;
        }
        // the whole call at once
        std::vector<KdbAddStep> steps(n);
        uint32_t entry = entry0;
        int32_t max_level = max0;
        kdb_add_plan(&entry, &max_level, first, asked.data(), n, steps.data());
        uint64_t lists = 0;
        for (unsigned i = 0; i < n; i++) {
            CHECK(steps[i].level == kept[i], "node %u keeps level %u, the oracle %u", first + i, (unsigned)steps[i].level, kept[i]);
            const unsigned e_before = i ? entry_after[i - 1] : (max0 < 0 ? 0u : entry0);
            const int m_before = i ? max_after[i - 1] : max0;
            CHECK(steps[i].entry == e_before && steps[i].max_level == m_before, "node %u finds (%u, %d), the oracle left (%u, %d)", first + i,
                  steps[i].entry, steps[i].max_level, e_before, m_before);
            if (m_before >= 0) lists += (uint64_t)((int)kept[i] < m_before ? (int)kept[i] : m_before) + 1u;
        }
        if (n) CHECK(entry == entry_after[n - 1] && max_level == max_after[n - 1], "after the call (%u, %d), the oracle (%u, %d)", entry, max_level,
                     entry_after[n - 1], max_after[n - 1]);
        else CHECK(entry == entry0 && max_level == max0, "an empty call changed the state");
        CHECK(kdb_add_plan_lists(steps.data(), n) == lists, "list count");
        // ... and one node per call: the same trajectory
        entry = entry0;
        max_level = max0;
        for (unsigned i = 0; i < n; i++) {
            KdbAddStep s1;
            kdb_add_plan(&entry, &max_level, first + i, &asked[i], 1, &s1);
            CHECK(s1.level == steps[i].level && s1.entry == steps[i].entry && s1.max_level == steps[i].max_level, "one call per node differs at node %u", first + i);
            CHECK(entry == entry_after[i] && max_level == max_after[i], "one call per node: after node %u", first + i);
        }
        nodes += n;
    }
    std::fclose(f);
    std::printf("ok %d cases, %ld nodes\n", n_cases, nodes);
    return 0;
}
