// df_hist_plan.h — the host plan of the histogram kernel (df_hist.hip): the argument rules of the
// tables and the groups of tables one launch counts at once.  Host-only code: df_hist_plan.cpp
// builds with g++ and tests/hist_plan_check.cpp prints its output without a device.
//
// A group is what one launch holds in LDS: up to kHsGroupDims kept dimensions (their edges, and
// a column each in every wave's tile of 64 draws) and up to kHsGroupTables tables over them.
// LDS of a workgroup, in 4-byte words:
//   [slot of every dimension: 64 | edges: Σ (L + 1), rounded up to 4 |
//    teams · tables (table_words each) | 4 waves · tile: 64 · (n_dims | 1)]
// teams = 1 (a workgroup per point) or 4 (a wave per point: four points per workgroup share the
// edges and hold a set of tables each).  A workgroup stays within kHsLdsWords (80 KiB: two
// workgroups fit a CU's 160 KiB) and its tables within kHsTableWords (64 KiB).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace df {

constexpr int kHsGroupDims = 16;
constexpr int kHsGroupTables = 64;
constexpr int kHsWaves = 4;
constexpr int kHsRows = 64;
constexpr int kHsLdsWords = 20480;    // 80 KiB
constexpr int kHsTableWords = 16384;  // 64 KiB: one 128 x 128 table

// Passed to the kernel by value; every index into it is uniform over the workgroup.
struct HistGroup {
    int32_t n_dims, n_tables;
    int32_t edge_words;                // Σ (L + 1) over the group's dimensions
    int32_t table_words;               // Σ table sizes · the bin width in words, rounded up to a multiple of 4
    int16_t dim[kHsGroupDims];         // slot s: the dimension,
    int16_t bins[kHsGroupDims];        //         its L,
    int32_t edge_src[kHsGroupDims];    //         its first edge in the caller's edges array,
    int16_t edge_lds[kHsGroupDims];    //         and in the group's LDS edges
    uint8_t ta[kHsGroupTables];        // table t: slot of the lower dimension (runs fastest),
    uint8_t tb[kHsGroupTables];        //          slot of the higher one, kHs1D: a 1-D table
    int32_t out_off[kHsGroupTables];   //          its offset in a point's block (request order)
    int32_t lds_off[kHsGroupTables];   //          its offset in a team's tables, in bins
};
constexpr uint8_t kHs1D = 0xFF;

constexpr int hs_round4(int v) { return (v + 3) & ~3; }
constexpr int hs_tile_words(int n_dims) { return kHsRows * (n_dims | 1); }
constexpr int hs_lds_words(int n_dims, int edge_words, int table_words, int teams) {
    return 64 + hs_round4(edge_words) + teams * table_words + kHsWaves * hs_tile_words(n_dims);
}

struct HistPlan {
    std::vector<HistGroup> groups;
    int64_t block_words = 0;  // T
};

// Rules 5-8 of df_draw_histograms on HOST arrays (non-null): n_tables, bins, the requests, and
// T (*block_words) within int32, T·n_points within int64.  DF_OK, or the status with *msg.
int hist_check_tables(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int64_t n_points,
                      int64_t* block_words, std::string* msg);

// The groups of checked tables for `teams` teams per workgroup.  Every table lands in exactly
// one group; tables over the same block of dimensions share a group, so that a group of
// |A| x |B| tables costs |A| + |B| bin searches per draw.  false: a table does not fit a team's
// share of the LDS (teams = 4 only: every checked table fits a workgroup's).
bool hist_plan(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int teams, HistPlan* plan);

// The weighted tables (df_whist.hip): bins of `width` 4-byte words — 1: hist_plan, 2: uint64 sums of
// quantised weights, where table_words doubles within the same budgets (lds_off stays in bins).
// whist_check_tables: hist_check_tables' rules, then every table within DF_WHIST_MAX_TABLE_BINS
// (DF_ERR_UNSUPPORTED, the message names the request), then T·n_points 8-byte words within int64.
int whist_check_tables(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int64_t n_points,
                       int64_t* block_words, std::string* msg);
bool hist_plan_width(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int teams, int width,
                     HistPlan* plan);

}  // namespace df
