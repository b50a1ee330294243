// df_whist.hip — 1-D and 2-D marginal histograms of per-point draws under importance weights, on
// the device:
//   df_draw_weighted_histograms   the requested tables of every point of a caller-owned
//                                 (d, n_points · n_draws) array of draws; a bin holds the sum of the
//                                 quantised weights (df_wscale.h) of the draws df_draw_histograms
//                                 would have counted there, as uint64
// The bin rule, the edge search, the groups of tables and the three mappings are df_hist.hip's;
// the planner runs with bins of two 4-byte words (df_hist_plan.h: hist_plan_width).  A bin is at
// most T = Σ q < 2^56: it cannot overflow.
//
// draw_whist_kernel: draw_hist_kernel with uint64 tables.  After the search, lane = row reads its
// own weight (the tile's 64 weights: one coalesced read), quantises it with the point's e
// (scale_out, written by weight_scale_kernel earlier on the stream) and, when q > 0, adds q per
// table with one 64-bit LDS add.  The Wave and Block maps store every bin of a table plainly; the
// Split map adds its non-zero bins with 64-bit integer global atomic adds into blocks the call
// has zeroed on the stream.  All sums are integers: every mapping, and every order of the adds,
// gives the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>

#include "densityflows_hip.h"
#include "df_handle.h"
#include "df_hist_plan.h"
#include "df_wscale.h"

namespace df {
namespace {

constexpr int kWhThreads = 64 * kHsWaves;
constexpr int kWhWaveMax = 256;  // N up to which a point is one wave's
constexpr int64_t kWhDrawsMax = (int64_t)1 << 24;
constexpr int kWhWidth = 2;  // 4-byte words of a bin

enum WhMap { kWhWave = 0, kWhBlock = 1, kWhSplit = 2 };

static_assert(kWhWidth * DF_WHIST_MAX_TABLE_BINS == kHsTableWords, "the largest table is the tables' budget");
static_assert(hs_lds_words(2, 2 * (DF_HIST_MAX_BINS + 1), kWhWidth * DF_WHIST_MAX_TABLE_BINS, 1) <= kHsLdsWords,
              "the largest table, its edges and the tiles fit a workgroup");
static_assert(DF_HIST_MAX_BINS <= 128, "the search has 8 steps: 129 edges at most");
static_assert(DF_HIST_SPLIT_DRAWS % (kHsRows * kHsWaves) == 0 && DF_HIST_SPLIT_DRAWS > kWhWaveMax,
              "a workgroup of the split path takes whole trips");
static_assert(kWhDrawsMax * 64 < ((int64_t)1 << 31), "element indices of a point (N·d) are int32");

template <int MAP>
__device__ __forceinline__ void wh_team_sync() {
    if (MAP != kWhWave) {
        __syncthreads();
    } else {
        // a wave's own LDS instructions are served in order: this keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// df_hist.hip's hs_bin: #{edges found <= v} − 1 with the last-edge rule, an index in [-1, L − 1]
// for any edge content
__device__ __forceinline__ int wh_bin(const float* e, int L, float v) {
    int pos = 0;
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1) {
        const int nxt = pos + step;
        const int at = nxt - 1 < L ? nxt - 1 : L;  // in [0, L]
        const bool take = (nxt <= L + 1) & (e[at] <= v);
        pos = take ? nxt : pos;
    }
    const int bin = pos - 1;
    return bin < L ? bin : (v == e[L] ? L - 1 : -1);
}

// xs (d, points · N): draw j of point i at xs + d·(i·N + j); w (points · N); scale: {e, T} per
// point; sums: blocks of T 8-byte words.  MAP == kWhSplit: workgroup b takes draws
// [s·split, min(N, (s + 1)·split)) of point b / nsplit, s = b % nsplit, and adds them to a zeroed
// block.
template <int MAP>
__global__ void __launch_bounds__(kWhThreads) draw_whist_kernel(const float* __restrict__ xs, const float* __restrict__ w,
                                                                int d, int N, int64_t points,
                                                                const float* __restrict__ edges, HistGroup g, int64_t T,
                                                                int split, int nsplit, const int64_t* __restrict__ scale,
                                                                unsigned long long* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wh_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int TT = MAP == kWhWave ? 64 : kWhThreads;   // threads of a team
    constexpr int W = MAP == kWhWave ? 1 : kHsWaves;       // its waves
    constexpr int teams = MAP == kWhWave ? kHsWaves : 1;   // teams of a workgroup
    const int t = MAP == kWhWave ? lane : tid;             // this thread in its team
    const int ndp = g.n_dims | 1;
    int* slot = reinterpret_cast<int*>(wh_lds);
    float* ed = reinterpret_cast<float*>(slot + 64);
    uint32_t* all_tabs = reinterpret_cast<uint32_t*>(ed + hs_round4(g.edge_words));  // 16-byte aligned
    unsigned long long* tabs =
        reinterpret_cast<unsigned long long*>(all_tabs + (MAP == kWhWave ? wave : 0) * g.table_words);
    int* tile = reinterpret_cast<int*>(all_tabs + teams * g.table_words) + wave * hs_tile_words(g.n_dims);

    // the workgroup's: slots and edges
    if (tid < 64) {
        int s_of = -1;
        for (int s = 0; s < g.n_dims; ++s) s_of = g.dim[s] == tid ? s : s_of;
        slot[tid] = s_of;
    }
    for (int s = 0; s < g.n_dims; ++s) {
        const float* src = edges + g.edge_src[s];
        float* dst = ed + g.edge_lds[s];
        for (int j = tid; j <= g.bins[s]; j += kWhThreads) dst[j] = src[j];
    }
    __syncthreads();

    int64_t i;
    int r_lo = 0, r_hi = N;
    if (MAP == kWhWave) {
        i = (int64_t)blockIdx.x * kHsWaves + wave;
        if (i >= points) return;  // the whole wave; this mapping has no workgroup barrier below
    } else if (MAP == kWhBlock) {
        i = blockIdx.x;
    } else {
        i = blockIdx.x / (unsigned)nsplit;
        r_lo = (int)(blockIdx.x % (unsigned)nsplit) * split;
        r_hi = N - r_lo < split ? N : r_lo + split;
    }
    const int e = (int)scale[2 * i];

    for (int v = t; v < g.table_words / 4; v += TT) reinterpret_cast<uint4*>(tabs)[v] = make_uint4(0u, 0u, 0u, 0u);
    wh_team_sync<MAP>();

    for (int r0 = r_lo + (MAP == kWhWave ? 0 : wave) * kHsRows; r0 < r_hi; r0 += kHsRows * W) {
        const int R = r_hi - r0 < kHsRows ? r_hi - r0 : kHsRows;  // a multiple of 4
        const float4* src = reinterpret_cast<const float4*>(xs + (i * N + r0) * d);
        const int nv = R / 4 * d;
        wh_team_sync<kWhWave>();  // the last trip's adds before this trip's stage
        for (int v = lane; v < nv; v += 64) {
            const float4 f = src[v];
            int row = 4 * v / d, col = 4 * v - row * d;
            const float vals[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int el = 0; el < 4; ++el) {
                const int s = slot[col];
                if (s >= 0) tile[row * ndp + s] = __float_as_int(vals[el]);
                if (++col == d) {
                    col = 0;
                    ++row;
                }
            }
        }
        wh_team_sync<kWhWave>();
        if (lane < R) {
            const unsigned long long q = rs_quant(rs_key(w[i * N + r0 + lane]), e);
            if (q != 0) {
                int* mine = tile + lane * ndp;
                for (int s = 0; s < g.n_dims; ++s) mine[s] = wh_bin(ed + g.edge_lds[s], g.bins[s], __int_as_float(mine[s]));
                for (int k = 0; k < g.n_tables; ++k) {
                    const int sa = g.ta[k], sb = g.tb[k];
                    const int ia = mine[sa];
                    if (sb == kHs1D) {
                        if (ia >= 0) atomicAdd(&tabs[g.lds_off[k] + ia], q);
                    } else {
                        const int ib = mine[sb];
                        if ((ia | ib) >= 0) atomicAdd(&tabs[g.lds_off[k] + ia + g.bins[sa] * ib], q);
                    }
                }
            }
        }
    }
    wh_team_sync<MAP>();

    unsigned long long* block = sums + i * T;
    for (int k = 0; k < g.n_tables; ++k) {
        const int sb = g.tb[k];
        const int size = g.bins[g.ta[k]] * (sb == kHs1D ? 1 : g.bins[sb]);
        const unsigned long long* from = tabs + g.lds_off[k];
        unsigned long long* to = block + g.out_off[k];
        for (int v = t; v < size; v += TT) {
            const unsigned long long c = from[v];
            if (MAP == kWhSplit) {
                if (c != 0) atomicAdd(&to[v], c);
            } else {
                to[v] = c;
            }
        }
    }
}

// MaxDynamicSharedMemorySize of an instance = the largest request any launch of it has made in
// this process (the attribute belongs to the function, not to a call)
hipError_t raise_lds_limit(const void* k, int map, size_t lds) {
    static std::mutex mu;
    static size_t limit[3] = {};
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[map];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

template <int MAP>
hipError_t launch_group(const float* xs, const float* w, int d, int N, int64_t points, const float* edges,
                        const HistGroup& g, int64_t T, int split, int nsplit, const int64_t* scale, uint64_t* sums,
                        hipStream_t st) {
    const int teams = MAP == kWhWave ? kHsWaves : 1;
    const size_t lds = 4 * (size_t)hs_lds_words(g.n_dims, g.edge_words, g.table_words, teams);
    if (lds > 4 * (size_t)kHsLdsWords) return hipErrorInvalidValue;  // the planner's budget
    const void* k = reinterpret_cast<const void*>(&draw_whist_kernel<MAP>);
    const hipError_t e = raise_lds_limit(k, MAP, lds);
    if (e != hipSuccess) return e;
    const int64_t blocks = MAP == kWhWave ? (points + kHsWaves - 1) / kHsWaves : points * nsplit;
    hipLaunchKernelGGL((draw_whist_kernel<MAP>), dim3((unsigned)blocks), dim3(kWhThreads), lds, st, xs, w, d, N, points,
                       edges, g, T, split, nsplit, scale, reinterpret_cast<unsigned long long*>(sums));
    return hipGetLastError();
}

// DF_HIST_SPLIT_DRAWS, or the environment's value of that name, as df_draw_histograms reads it
// (a tuning aid: the sums do not depend on it)
int split_draws() {
    if (const char* s = std::getenv("DF_HIST_SPLIT_DRAWS")) {
        const long v = std::strtol(s, nullptr, 10);
        if (v > kWhWaveMax && v <= kWhDrawsMax && v % (kHsRows * kHsWaves) == 0) return (int)v;
    }
    return DF_HIST_SPLIT_DRAWS;
}

}  // namespace
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_draw_weighted_histograms(const float* xs, const float* w, int d, int64_t n_points, int64_t n_draws,
                                const float* edges, const int32_t* bins, const int32_t* keep, int32_t n_tables,
                                uint64_t* sums_out, int64_t* scale_out, void* stream) {
    if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0) return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kWhDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    if (!xs || !w) return set_err(DF_ERR_INVALID, "null xs or w array");
    if (!sums_out || !scale_out) return set_err(DF_ERR_INVALID, "null sums_out or scale_out array");
    if (!edges || !bins || !keep) return set_err(DF_ERR_INVALID, "null edges, bins or keep array");
    if (reinterpret_cast<uintptr_t>(xs) % 16 != 0) return set_err(DF_ERR_INVALID, "xs must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(w) % 16 != 0) return set_err(DF_ERR_INVALID, "w must be 16-byte aligned");
    std::string msg;
    // the count before bins is read: bins holds d words
    static const int32_t no_bins[1] = {0}, no_keep[2] = {0, -1};
    if (n_tables < 1 || n_tables > DF_HIST_MAX_TABLES)
        return set_err(hist_check_tables(1, no_bins, no_keep, n_tables, 0, nullptr, &msg), msg);
    int64_t T = 0;
    int rc = whist_check_tables(d, bins, keep, n_tables, n_points, &T, &msg);
    if (rc != DF_OK) return set_err(rc, msg);
    if (n_points > (INT64_MAX / 8) / n_draws / d) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    if (n_points == 0) return DF_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_draws;
    HistPlan wave, block;
    const bool wave_ok = hist_plan_width(d, bins, keep, n_tables, kHsWaves, kWhWidth, &wave);
    if (!hist_plan_width(d, bins, keep, n_tables, 1, kWhWidth, &block))  // not reached for checked tables
        return set_err(DF_ERR_UNSUPPORTED, "a histogram table does not fit the LDS");
    const int split = split_draws();
    const int map = N > split ? kWhSplit : (N <= kWhWaveMax && wave_ok ? kWhWave : kWhBlock);
    const int nsplit = map == kWhSplit ? (N + split - 1) / split : 1;
    if ((map == kWhWave ? (n_points + kHsWaves - 1) / kHsWaves : n_points * nsplit) > 0x7fffffff)
        return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    if ((rc = launch_weight_scale(w, n_points, N, scale_out, st)) != DF_OK) return rc;
    if (map == kWhSplit) {
        const hipError_t e = hipMemsetAsync(sums_out, 0, sizeof(uint64_t) * (size_t)T * (size_t)n_points, st);
        if (e != hipSuccess) return hip_err(e, "hipMemsetAsync(sums_out)");
    }
    for (const HistGroup& g : (map == kWhWave ? wave : block).groups) {
        const hipError_t e =
            map == kWhWave    ? launch_group<kWhWave>(xs, w, d, N, n_points, edges, g, T, split, 1, scale_out, sums_out, st)
            : map == kWhBlock ? launch_group<kWhBlock>(xs, w, d, N, n_points, edges, g, T, split, 1, scale_out, sums_out, st)
                              : launch_group<kWhSplit>(xs, w, d, N, n_points, edges, g, T, split, nsplit, scale_out, sums_out, st);
        if (e != hipSuccess) return hip_err(e, "weighted histogram kernel launch");
    }
    return DF_OK;
}

}  // extern "C"
