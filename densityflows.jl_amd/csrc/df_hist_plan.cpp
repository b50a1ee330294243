// df_hist_plan.cpp — see df_hist_plan.h.  Host-only: no HIP header, built with g++.
#include "df_hist_plan.h"

#include <algorithm>
#include <map>
#include <set>
#include <utility>

#include "densityflows_hip.h"

namespace df {
namespace {

int fail(int code, std::string* msg, const std::string& text) {
    if (msg) *msg = text;
    return code;
}

int64_t table_size(const int32_t* bins, int a, int b) {
    return b < 0 ? (int64_t)bins[a] : (int64_t)bins[a] * bins[b];
}

// A group under construction: the slots of its dimensions and the running LDS sizes.
struct Builder {
    const int32_t* bins;
    const std::vector<int32_t>* edge_src;
    int teams;
    int width = 1;  // 4-byte words of a bin
    HistGroup g = {};
    int raw_table_words = 0;  // the tables' bins

    int slot(int dim) const {
        for (int s = 0; s < g.n_dims; ++s)
            if (g.dim[s] == dim) return s;
        return -1;
    }
    bool add(int a, int b, int32_t out_off) {
        Builder next = *this;
        int sa = next.slot(a), sb = -1;
        if (sa < 0 && (sa = next.add_dim(a)) < 0) return false;
        if (b >= 0 && (sb = next.slot(b)) < 0 && (sb = next.add_dim(b)) < 0) return false;
        HistGroup& n = next.g;
        if (n.n_tables == kHsGroupTables) return false;
        const int t = n.n_tables++;
        n.ta[t] = (uint8_t)sa;
        n.tb[t] = b >= 0 ? (uint8_t)sb : kHs1D;
        n.out_off[t] = out_off;
        n.lds_off[t] = next.raw_table_words;
        next.raw_table_words += (int)table_size(bins, a, b);
        n.table_words = hs_round4(width * next.raw_table_words);
        if ((int64_t)teams * n.table_words > kHsTableWords ||
            hs_lds_words(n.n_dims, n.edge_words, n.table_words, teams) > kHsLdsWords)
            return false;
        g = next.g;
        raw_table_words = next.raw_table_words;
        return true;
    }

private:
    int add_dim(int dim) {
        if (g.n_dims == kHsGroupDims) return -1;
        const int s = g.n_dims++;
        g.dim[s] = (int16_t)dim;
        g.bins[s] = (int16_t)bins[dim];
        g.edge_src[s] = (*edge_src)[dim];
        g.edge_lds[s] = (int16_t)g.edge_words;
        g.edge_words += bins[dim] + 1;
        return s;
    }
};

}  // namespace

int hist_check_tables(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int64_t n_points,
                      int64_t* block_words, std::string* msg) {
    if (n_tables < 1 || n_tables > DF_HIST_MAX_TABLES)
        return fail(DF_ERR_UNSUPPORTED, msg, "n_tables must be in 1 .. DF_HIST_MAX_TABLES (2080)");
    for (int k = 0; k < d; ++k) {
        if (bins[k] < 0) return fail(DF_ERR_INVALID, msg, "bins[" + std::to_string(k) + "] is negative");
        if (bins[k] > DF_HIST_MAX_BINS)
            return fail(DF_ERR_UNSUPPORTED, msg,
                        "bins[" + std::to_string(k) + "] = " + std::to_string(bins[k]) + " is above DF_HIST_MAX_BINS (128)");
    }
    std::set<std::pair<int, int>> seen;
    int64_t T = 0;
    for (int j = 0; j < n_tables; ++j) {
        const int a = keep[2 * j], b = keep[2 * j + 1];
        const std::string who = "keep[" + std::to_string(j) + "] = {" + std::to_string(a) + ", " + std::to_string(b) + "}";
        if (a < 0 || a >= d) return fail(DF_ERR_INVALID, msg, who + ": the first dimension is outside [0, d)");
        if (b != -1 && (b <= a || b >= d))
            return fail(DF_ERR_INVALID, msg, who + ": the second dimension is neither -1 nor in (first, d)");
        if (bins[a] == 0 || (b >= 0 && bins[b] == 0))
            return fail(DF_ERR_INVALID, msg, who + " keeps a dimension without bins (bins = 0)");
        if (!seen.insert({a, b}).second) return fail(DF_ERR_INVALID, msg, who + " repeats an earlier request");
        T += table_size(bins, a, b);
    }
    if (T > INT32_MAX) return fail(DF_ERR_SHAPE, msg, "the tables of a point (T) are past int32");
    if (n_points > 0 && n_points > (INT64_MAX / 4) / T) return fail(DF_ERR_SHAPE, msg, "T · n_points past int64");
    if (block_words) *block_words = T;
    return DF_OK;
}

int whist_check_tables(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int64_t n_points,
                       int64_t* block_words, std::string* msg) {
    int64_t T = 0;
    const int rc = hist_check_tables(d, bins, keep, n_tables, 0, &T, msg);
    if (rc != DF_OK) return rc;
    for (int j = 0; j < n_tables; ++j) {
        const int a = keep[2 * j], b = keep[2 * j + 1];
        if (table_size(bins, a, b) > DF_WHIST_MAX_TABLE_BINS)
            return fail(DF_ERR_UNSUPPORTED, msg,
                        "keep[" + std::to_string(j) + "] = {" + std::to_string(a) + ", " + std::to_string(b) + "}: a table of " +
                            std::to_string(table_size(bins, a, b)) + " bins is above DF_WHIST_MAX_TABLE_BINS (8192)");
    }
    if (n_points > 0 && n_points > (INT64_MAX / 8) / T) return fail(DF_ERR_SHAPE, msg, "T · n_points past int64");
    if (block_words) *block_words = T;
    return DF_OK;
}

bool hist_plan(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int teams, HistPlan* plan) {
    return hist_plan_width(d, bins, keep, n_tables, teams, 1, plan);
}

bool hist_plan_width(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables, int teams, int width,
                     HistPlan* plan) {
    plan->groups.clear();
    std::vector<int32_t> edge_src(d, 0), out_off(n_tables, 0);
    int32_t at = 0;
    for (int k = 0; k < d; ++k) {
        edge_src[k] = at;
        if (bins[k] > 0) at += bins[k] + 1;
    }
    std::vector<int> rank_of(d, -1);  // position of a kept dimension among the kept ones
    int64_t T = 0;
    int lmax = 1;
    for (int j = 0; j < n_tables; ++j) {
        const int a = keep[2 * j], b = keep[2 * j + 1];
        out_off[j] = (int32_t)T;
        T += table_size(bins, a, b);
        rank_of[a] = 0;
        lmax = std::max(lmax, bins[a]);
        if (b >= 0) {
            rank_of[b] = 0;
            lmax = std::max(lmax, bins[b]);
        }
    }
    plan->block_words = T;
    int n_kept = 0;
    for (int k = 0; k < d; ++k)
        if (rank_of[k] == 0) rank_of[k] = n_kept++;

    // kept dimensions in blocks of g: the largest g whose full block pair (g x g tables of
    // lmax x lmax bins over 2g dimensions) fits
    int g = 1;
    for (int c = kHsGroupDims / 2; c > 1; --c) {
        const int tw = hs_round4(width * c * c * lmax * lmax);
        if (c * c <= kHsGroupTables && (int64_t)teams * tw <= kHsTableWords &&
            hs_lds_words(2 * c, 2 * c * (lmax + 1), tw, teams) <= kHsLdsWords) {
            g = c;
            break;
        }
    }
    std::map<std::pair<int, int>, std::vector<int>> buckets;  // (block of a, block of b) → requests
    for (int j = 0; j < n_tables; ++j) {
        const int a = keep[2 * j], b = keep[2 * j + 1];
        buckets[{rank_of[a] / g, rank_of[b >= 0 ? b : a] / g}].push_back(j);
    }

    Builder cur{bins, &edge_src, teams, width};
    auto close = [&]() {
        if (cur.g.n_tables > 0) plan->groups.push_back(cur.g);
        cur = Builder{bins, &edge_src, teams, width};
    };
    for (const auto& kv : buckets) {
        // the whole bucket beside what the group holds, or a group of its own
        Builder whole = cur;
        bool fits = true;
        for (int j : kv.second)
            if (!(fits = whole.add(keep[2 * j], keep[2 * j + 1], out_off[j]))) break;
        if (fits) {
            cur = whole;
            continue;
        }
        close();
        for (int j : kv.second) {
            if (cur.add(keep[2 * j], keep[2 * j + 1], out_off[j])) continue;
            close();
            if (!cur.add(keep[2 * j], keep[2 * j + 1], out_off[j])) return false;  // one table past a team's share
        }
    }
    close();
    return true;
}

}  // namespace df
