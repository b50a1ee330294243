// df_hist.hip — 1-D and 2-D marginal histograms of per-point draws, on the device:
//   df_draw_histograms         the requested tables of every point of a caller-owned
//                              (d, n_points · n_draws) array of draws
//   df_flow_point_histograms   df_flow_point_stats' chunk loop (df_pstats.hip: point_draw_chunks)
//                              with the counting at its end: the corner plot of one sampling
//                              pass, and on request the draws
//
// Bin rule (numpy's for explicit edges e_0 .. e_L): bin j holds e_j <= v < e_{j+1}, the last bin
// also v == e_L; Float32 comparisons.  A draw below e_0, above e_L or NaN is counted nowhere in
// the tables that keep its dimension.
//
// draw_hist_kernel.  The host plans groups of tables (df_hist_plan.cpp); a launch counts one
// group, which it receives by value.  The group's edges and the slot of every dimension sit in
// LDS, shared by the workgroup; every team (the unit that owns a point) has the group's tables
// there, and every wave a tile.  A wave and a tile of 64 draws (rows) at a time:
//   stage   the tile's 64·d contiguous floats with 16-byte loads; of each row only the group's
//           dimensions are kept, row stride n_dims | 1 (odd: the column reads are conflict-free).
//           The rows are N·d/4 whole float4 (N % 4 == 0): no lane reads past the point's last
//           draw, and a lane past the last vector stores nothing
//   search  lane = row.  Per kept dimension a branch-free binary search of 8 steps over the
//           L + 1 edges: pos = #{edges found <= v} in [0, L + 1] — a step is taken only while
//           pos + step <= L + 1 and the edge read is clamped to [0, L], so the walk is bounded
//           for any edge content.  bin = pos − 1; bin == L stays as L − 1 when v == e_L and is
//           dropped otherwise.  The bin (−1: outside) replaces the value in the tile
//   count   per table one ds_add_u32 at i_a + L_a·i_b (both >= 0), or at i_a (1-D)
// After the last tile the team's tables go to the point's block.
//
// With N = n_draws the mapping of points follows from N and the tables:
//   N <= 256            a wave per point, 4 points per workgroup, no workgroup barrier after
//                       the set-up (if a table does not fit a quarter of the LDS: as below)
//   N <= SPLIT_DRAWS    a workgroup per point: wave w takes tiles w, w + 4, ...
//   above               ceil(N / SPLIT_DRAWS) workgroups per point, SPLIT_DRAWS draws each
// The first two write every word of a table with plain stores, zero bins included: nothing is
// zeroed in global memory and there are no global atomics.  The third adds its non-zero bins
// with integer global atomic adds (consecutive lanes, consecutive words of a table) into blocks
// the call has zeroed on the stream.  Counts are integers: every mapping, and every order of
// the adds, gives the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>

#include "densityflows_hip.h"
#include "df_handle.h"
#include "df_hist_plan.h"

namespace df {
namespace {

constexpr int kHsThreads = 64 * kHsWaves;
constexpr int kHsWaveMax = 256;  // N up to which a point is one wave's
constexpr int64_t kHsDrawsMax = (int64_t)1 << 24;
constexpr size_t kHsLdsMax = 160 * 1024;

enum HsMap { kHsWave = 0, kHsBlock = 1, kHsSplit = 2 };

static_assert(2 * (size_t)kHsLdsWords * 4 <= kHsLdsMax, "two workgroups fit a CU");
static_assert(DF_HIST_MAX_BINS * DF_HIST_MAX_BINS <= kHsTableWords, "the largest table is one group");
static_assert(hs_lds_words(2, 2 * (DF_HIST_MAX_BINS + 1), DF_HIST_MAX_BINS * DF_HIST_MAX_BINS, 1) <= kHsLdsWords,
              "the largest table, its edges and the tiles fit a workgroup");
static_assert(DF_HIST_MAX_BINS <= 128, "the search has 8 steps: 129 edges at most");
static_assert(DF_HIST_SPLIT_DRAWS % (kHsRows * kHsWaves) == 0 && DF_HIST_SPLIT_DRAWS > kHsWaveMax,
              "a workgroup of the split path takes whole trips");
static_assert(kHsDrawsMax * 64 < ((int64_t)1 << 31), "element indices of a point (N·d) are int32");

template <int MAP>
__device__ __forceinline__ void hs_team_sync() {
    if (MAP != kHsWave) {
        __syncthreads();
    } else {
        // a wave's own LDS instructions are served in order: this keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// #{edges found <= v} − 1 with the last-edge rule: an index in [-1, L − 1] for any edge content
__device__ __forceinline__ int hs_bin(const float* e, int L, float v) {
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

// xs (d, points · N): draw j of point i at xs + d·(i·N + j); counts: blocks of T words.
// MAP == kHsSplit: workgroup b counts draws [s·split, min(N, (s + 1)·split)) of point b / nsplit,
// s = b % nsplit, and adds them to a zeroed block.
template <int MAP>
__global__ void __launch_bounds__(kHsThreads) draw_hist_kernel(const float* __restrict__ xs, int d, int N, int64_t points,
                                                               const float* __restrict__ edges, HistGroup g, int64_t T,
                                                               int split, int nsplit, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int TT = MAP == kHsWave ? 64 : kHsThreads;   // threads of a team
    constexpr int W = MAP == kHsWave ? 1 : kHsWaves;       // its waves
    constexpr int teams = MAP == kHsWave ? kHsWaves : 1;   // teams of a workgroup
    const int t = MAP == kHsWave ? lane : tid;             // this thread in its team
    const int ndp = g.n_dims | 1;
    int* slot = reinterpret_cast<int*>(hs_lds);
    float* ed = reinterpret_cast<float*>(slot + 64);
    uint32_t* all_tabs = reinterpret_cast<uint32_t*>(ed + hs_round4(g.edge_words));
    uint32_t* tabs = all_tabs + (MAP == kHsWave ? wave : 0) * g.table_words;
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
        for (int j = tid; j <= g.bins[s]; j += kHsThreads) dst[j] = src[j];
    }
    __syncthreads();

    int64_t i;
    int r_lo = 0, r_hi = N;
    if (MAP == kHsWave) {
        i = (int64_t)blockIdx.x * kHsWaves + wave;
        if (i >= points) return;  // the whole wave; this mapping has no workgroup barrier below
    } else if (MAP == kHsBlock) {
        i = blockIdx.x;
    } else {
        i = blockIdx.x / (unsigned)nsplit;
        r_lo = (int)(blockIdx.x % (unsigned)nsplit) * split;
        r_hi = N - r_lo < split ? N : r_lo + split;
    }

    for (int w = t; w < g.table_words / 4; w += TT) reinterpret_cast<uint4*>(tabs)[w] = make_uint4(0u, 0u, 0u, 0u);
    hs_team_sync<MAP>();

    for (int r0 = r_lo + (MAP == kHsWave ? 0 : wave) * kHsRows; r0 < r_hi; r0 += kHsRows * W) {
        const int R = r_hi - r0 < kHsRows ? r_hi - r0 : kHsRows;  // a multiple of 4
        const float4* src = reinterpret_cast<const float4*>(xs + (i * N + r0) * d);
        const int nv = R / 4 * d;
        hs_team_sync<kHsWave>();  // the last trip's counting before this trip's stage
        for (int v = lane; v < nv; v += 64) {
            const float4 f = src[v];
            int row = 4 * v / d, col = 4 * v - row * d;
            const float vals[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = slot[col];
                if (s >= 0) tile[row * ndp + s] = __float_as_int(vals[e]);
                if (++col == d) {
                    col = 0;
                    ++row;
                }
            }
        }
        hs_team_sync<kHsWave>();
        if (lane < R) {
            int* mine = tile + lane * ndp;
            for (int s = 0; s < g.n_dims; ++s) mine[s] = hs_bin(ed + g.edge_lds[s], g.bins[s], __int_as_float(mine[s]));
            for (int k = 0; k < g.n_tables; ++k) {
                const int sa = g.ta[k], sb = g.tb[k];
                const int ia = mine[sa];
                if (sb == kHs1D) {
                    if (ia >= 0) atomicAdd(&tabs[g.lds_off[k] + ia], 1u);
                } else {
                    const int ib = mine[sb];
                    if ((ia | ib) >= 0) atomicAdd(&tabs[g.lds_off[k] + ia + g.bins[sa] * ib], 1u);
                }
            }
        }
    }
    hs_team_sync<MAP>();

    int32_t* block = counts + i * T;
    for (int k = 0; k < g.n_tables; ++k) {
        const int sb = g.tb[k];
        const int size = g.bins[g.ta[k]] * (sb == kHs1D ? 1 : g.bins[sb]);
        const uint32_t* from = tabs + g.lds_off[k];
        int32_t* to = block + g.out_off[k];
        for (int w = t; w < size; w += TT) {
            const int32_t c = (int32_t)from[w];
            if (MAP == kHsSplit) {
                if (c != 0) atomicAdd(&to[w], c);
            } else {
                to[w] = c;
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
hipError_t launch_group(const float* xs, int d, int N, int64_t points, const float* edges, const HistGroup& g, int64_t T,
                        int split, int nsplit, int32_t* counts, hipStream_t st) {
    const int teams = MAP == kHsWave ? kHsWaves : 1;
    const size_t lds = 4 * (size_t)hs_lds_words(g.n_dims, g.edge_words, g.table_words, teams);
    if (lds > 4 * (size_t)kHsLdsWords) return hipErrorInvalidValue;  // the planner's budget
    const void* k = reinterpret_cast<const void*>(&draw_hist_kernel<MAP>);
    const hipError_t e = raise_lds_limit(k, MAP, lds);
    if (e != hipSuccess) return e;
    const int64_t blocks = MAP == kHsWave ? (points + kHsWaves - 1) / kHsWaves : points * nsplit;
    hipLaunchKernelGGL((draw_hist_kernel<MAP>), dim3((unsigned)blocks), dim3(kHsThreads), lds, st, xs, d, N, points, edges,
                       g, T, split, nsplit, counts);
    return hipGetLastError();
}

// DF_HIST_SPLIT_DRAWS, or the environment's value of that name while it is a multiple of a
// workgroup's trip above kHsWaveMax (a tuning aid: the counts do not depend on it)
int split_draws() {
    if (const char* s = std::getenv("DF_HIST_SPLIT_DRAWS")) {
        const long v = std::strtol(s, nullptr, 10);
        if (v > kHsWaveMax && v <= kHsDrawsMax && v % (kHsRows * kHsWaves) == 0) return (int)v;
    }
    return DF_HIST_SPLIT_DRAWS;
}

}  // namespace

namespace api {

struct HistTables {
    HistPlan wave, block;  // the groups of a wave-team (empty: some table needs a workgroup) and of a workgroup
    bool wave_ok = false;
};

int check_histogram_tables(const df_chain* c, int d, const float* edges, const int32_t* bins, const int32_t* keep,
                           int32_t n_tables, int64_t n_points, int64_t* block_words) {
    if (!edges || !bins || !keep) return set_err(DF_ERR_INVALID, "null edges, bins or keep array");
    std::string msg;
    // the count before the chain's d is read: bins holds d words
    static const int32_t no_bins[1] = {0}, no_keep[2] = {0, -1};
    if ((n_tables < 1 || n_tables > DF_HIST_MAX_TABLES))
        return set_err(hist_check_tables(1, no_bins, no_keep, n_tables, 0, nullptr, &msg), msg);
    if (c) d = c->plan.d;
    const int rc = hist_check_tables(d, bins, keep, n_tables, n_points, block_words, &msg);
    return rc == DF_OK ? DF_OK : set_err(rc, msg);
}

HistTables* plan_histograms(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables) {
    HistTables* h = new HistTables;
    h->wave_ok = hist_plan(d, bins, keep, n_tables, kHsWaves, &h->wave);
    if (!hist_plan(d, bins, keep, n_tables, 1, &h->block)) {  // not reached for checked tables
        delete h;
        return nullptr;
    }
    return h;
}

void free_histograms(HistTables* h) { delete h; }
int64_t histogram_block_words(const HistTables* h) { return h->block.block_words; }

int launch_draw_histograms(const float* xs, int d, int N, int64_t points, const float* edges, const HistTables* h,
                           int32_t* counts, hipStream_t st) {
    const int64_t T = h->block.block_words;
    const int split = split_draws();
    const int map = N > split ? kHsSplit : (N <= kHsWaveMax && h->wave_ok ? kHsWave : kHsBlock);
    const int nsplit = map == kHsSplit ? (N + split - 1) / split : 1;
    if ((map == kHsWave ? (points + kHsWaves - 1) / kHsWaves : points * nsplit) > 0x7fffffff)
        return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    if (map == kHsSplit) {
        const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)T * (size_t)points, st);
        if (e != hipSuccess) return hip_err(e, "hipMemsetAsync(counts)");
    }
    for (const HistGroup& g : (map == kHsWave ? h->wave : h->block).groups) {
        const hipError_t e = map == kHsWave    ? launch_group<kHsWave>(xs, d, N, points, edges, g, T, split, 1, counts, st)
                             : map == kHsBlock ? launch_group<kHsBlock>(xs, d, N, points, edges, g, T, split, 1, counts, st)
                                               : launch_group<kHsSplit>(xs, d, N, points, edges, g, T, split, nsplit, counts, st);
        if (e != hipSuccess) return hip_err(e, "histogram kernel launch");
    }
    return DF_OK;
}

}  // namespace api
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_draw_histograms(const float* xs, int d, int64_t n_points, int64_t n_draws, const float* edges,
                       const int32_t* bins, const int32_t* keep, int32_t n_tables, int32_t* counts_out, void* stream) {
    if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0) return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kHsDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    if (!xs || !counts_out) return set_err(DF_ERR_INVALID, "null xs or counts_out array");
    if (!edges || !bins || !keep) return set_err(DF_ERR_INVALID, "null edges, bins or keep array");
    if (reinterpret_cast<uintptr_t>(xs) % 16 != 0) return set_err(DF_ERR_INVALID, "xs must be 16-byte aligned");
    int64_t T = 0;
    const int rc = check_histogram_tables(nullptr, d, edges, bins, keep, n_tables, n_points, &T);
    if (rc != DF_OK) return rc;
    if (n_points == 0) return DF_OK;
    if (n_points > (INT64_MAX / 8) / n_draws / d) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    HistTables* h = plan_histograms(d, bins, keep, n_tables);
    if (!h) return set_err(DF_ERR_UNSUPPORTED, "a histogram table does not fit the LDS");
    const int out = launch_draw_histograms(xs, d, (int)n_draws, n_points, edges, h, counts_out,
                                           static_cast<hipStream_t>(stream));
    free_histograms(h);
    return out;
}

int df_flow_point_histograms(df_chain* c, const float* theta_raw, int64_t n_points, int64_t n_draws, int64_t chunk,
                             uint64_t seed, uint64_t offset, const float* edges, const int32_t* bins,
                             const int32_t* keep, int32_t n_tables, int32_t* counts_out, float* draws_out,
                             void* stream) {
    int rc = point_check_sizes(c, n_points, n_draws, chunk);
    if (rc != DF_OK) return rc;
    if (!counts_out && !draws_out) return set_err(DF_ERR_INVALID, "no output: counts_out and draws_out are both null");
    // the table rules past n_tables need d: a host word of the handle, no device work
    int64_t T = 0;
    if (counts_out && (rc = check_histogram_tables(c, 0, edges, bins, keep, n_tables, n_points, &T)) != DF_OK) return rc;
    if (n_points == 0) return DF_OK;
    PointOutputs out;
    out.draws = draws_out;
    HistTables* h = nullptr;
    if (counts_out) {
        if (!(h = plan_histograms(c->plan.d, bins, keep, n_tables)))
            return set_err(DF_ERR_UNSUPPORTED, "a histogram table does not fit the LDS");
        out.hist = h;
        out.edges = edges;
        out.counts = counts_out;
    }
    rc = point_draw_chunks(c, nullptr, theta_raw, n_points, n_draws, chunk, seed, offset, out, stream);
    free_histograms(h);
    return rc;
}

}  // extern "C"
