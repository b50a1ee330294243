// Prints the host plan of the weighted histogram kernel: bins of two 4-byte words
// (tests/test_wquantiles_host.py compiles this file with densityflows.jl_amd/csrc/df_hist_plan.cpp,
// no device and no HIP header needed).
//   whist_plan_check <file>
// file: "d teams n_tables n_points", then d bin counts, then n_tables pairs "a b".
// Output: that of hist_plan_check.cpp, from whist_check_tables and hist_plan_width at width 2;
// lds_off counts bins, table_words 4-byte words.
#include <cstdio>
#include <vector>

#include "densityflows_hip.h"
#include "df_hist_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int d = 0, teams = 0, n_tables = 0;
    long long n_points = 0;
    if (std::fscanf(f, "%d %d %d %lld", &d, &teams, &n_tables, &n_points) != 4) return 2;
    std::vector<int32_t> bins(d > 0 ? d : 1), keep(2 * (n_tables > 0 ? n_tables : 1));
    for (int k = 0; k < d; ++k)
        if (std::fscanf(f, "%d", &bins[k]) != 1) return 2;
    for (int j = 0; j < 2 * n_tables; ++j)
        if (std::fscanf(f, "%d", &keep[j]) != 1) return 2;
    std::fclose(f);

    constexpr int kWidth = 2;
    int64_t T = 0;
    std::string msg;
    const int rc = df::whist_check_tables(d, bins.data(), keep.data(), n_tables, n_points, &T, &msg);
    std::printf("check %d %lld\n", rc, (long long)T);
    if (rc != DF_OK) {
        std::printf("message %s\n", msg.c_str());
        return 0;
    }
    df::HistPlan plan;
    const bool ok = df::hist_plan_width(d, bins.data(), keep.data(), n_tables, teams, kWidth, &plan);
    std::printf("plan %d %zu %lld\n", ok ? 1 : 0, plan.groups.size(), (long long)plan.block_words);
    std::printf("budget %d %d %d %d\n", df::kHsLdsWords, df::kHsTableWords, df::kHsGroupDims, df::kHsGroupTables);
    if (!ok) return 0;
    for (const df::HistGroup& g : plan.groups) {
        std::printf("group %d %d %d %d %d\n", g.n_dims, g.n_tables, g.edge_words, g.table_words,
                    df::hs_lds_words(g.n_dims, g.edge_words, g.table_words, teams));
        for (int s = 0; s < g.n_dims; ++s) std::printf("dim %d %d %d %d\n", g.dim[s], g.bins[s], g.edge_src[s], g.edge_lds[s]);
        for (int t = 0; t < g.n_tables; ++t)
            std::printf("table %d %d %d %d\n", g.dim[g.ta[t]], g.tb[t] == df::kHs1D ? -1 : g.dim[g.tb[t]], g.out_off[t],
                        g.lds_off[t]);
    }
    return 0;
}
