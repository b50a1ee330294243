// df_pstats.hip — the samples of a conditional flow reduced per condition, on the device:
//   df_flow_point_stats   for every point (x_i, θ_i): the SBC ranks #{j : draw_j[k] < x_i[k]} of
//                         n_draws samples of q(. | θ_i), one int32 per dimension, and the shifted
//                         sums behind the posterior mean and covariance, 2d + d(d+1)/2 doubles
//
// The call's size rules and its chunk loop are point_check_sizes and point_draw_chunks, shared with
// df_flow_point_quantiles (df_quant.hip) and df_flow_point_histograms (df_hist.hip) through
// df_handle.h: those calls add the selection of order statistics, or the counting of the marginal
// tables, at the end of every chunk; what PointOutputs does not ask for is not launched.
//
// Per chunk of whole points, as df_flow_hpd_ranks (df_calib.hip): the Philox draw, θ row i
// repeated over the draws of point i, df_flow_forward_inplace (the pass df_flow_sample runs: no
// ldj, no base term), and point_stats_kernel over the chunk's (d, points · N) array — d · N
// contiguous floats per point, draw j of a point in its floats [j·d, (j+1)·d).
//
// point_stats_kernel.  The unit of work is a wave and a tile of 64 draws (rows): the wave
// copies the tile's 64·d contiguous floats with 16-byte loads into its own part of LDS, row
// stride d | 1 (odd: the column reads below are conflict-free), and then reads it twice:
//   ranks  lane = row.  For every dimension k one compare, one ballot, one population count:
//          the wave's 64 draws of dimension k in 3 vector instructions.
//   sums   lane = entry.  The E = d + d(d+1)/2 entries of a point (S1[a], then S2[a, b], a >= b)
//          go to the lanes 64 at a time; a lane walks the tile's rows in increasing order with
//          one fp64 FMA per row: acc = fma(double(v_a) − c_a, double(v_b) − c_b, acc), and
//          acc + (double(v_a) − c_a) for S1.  One accumulator per lane at a time: d = 32 has
//          528 pairs, 9 passes of the lanes over the tile, and no per-lane array.
//          d <= 16 (configs 1-2): the wave first writes the tile once more as shifted doubles,
//          double(v_k) − c_k with a column of ones for S1, so that a row costs two 8-byte LDS
//          reads and the FMA instead of two conversions and two subtractions per entry (LDS:
//          8 · 64 · ((d + 1) | 1) bytes more per wave, which is why d stops at 16).  While
//          E <= 32 (d <= 6) the lanes would be half idle: F = 64 / E groups of lanes then share
//          a tile's rows, group g rows g, g + F, ..., and the F sums of an entry are added in
//          group order.  The terms are the same fp64 values on both paths.
// With N = n_draws the mapping of points follows from N alone:
//   N <= 64    packed: 64 / N points per wave, point s in rows [s·N, (s+1)·N) of the wave's
//              one tile; a rank is the ballot under the point's row mask, a sum walks the
//              point's N rows and is stored at once.  4 waves (256 / N points) per workgroup.
//   N <= 256   a wave per point, 4 points per workgroup, no workgroup barrier: tiles (trips)
//              of 64 rows in increasing order; lane k keeps the count of dimension k, the
//              sums of a trip are added to the wave's accumulators in LDS (E doubles)
//   above      a workgroup per point: wave w takes trips w, w + 4, ...; the 4 waves' counts
//              and sums are added in wave order, ((w0 + w1) + w2) + w3, behind one barrier
// Every (d, n_draws) takes the mapping of its N for every d <= 64; only the LDS a wave needs
// (64 · (d | 1) floats, and E doubles in the two mappings with trips) grows with d.
// Counts are integers.  The order of every fp64 sum is fixed by (d, N): rows in increasing
// order inside a trip (inside a group, then the groups in order, d <= 6), trips in increasing
// order inside a wave, waves in wave order.  It
// depends neither on the chunk, nor on the other points, nor on the grid: no atomics, no
// zeroing pass, one store per (point, dimension) and per (point, entry).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kPsThreads = 256;  // 4 waves
constexpr int kPsWaves = kPsThreads / 64;
constexpr int kPsRows = 64;            // draws of a tile: a lane per row
constexpr int kPsPackedMax = 64;       // N up to which several points share a wave
constexpr int kPsWaveMax = 256;        // N up to which a point is one wave's (four trips)
constexpr int kPsShiftMaxD = 16;       // d up to which the sums read a tile of shifted doubles
constexpr int64_t kChunkDefault = (int64_t)1 << 20, kChunkMax = (int64_t)1 << 24;
constexpr int64_t kDrawsMax = (int64_t)1 << 24;

enum PsMap { kPsPacked = 0, kPsWave = 1, kPsBlock = 2 };

__host__ __device__ constexpr int ps_entries(int d) { return d + d * (d + 1) / 2; }

// LDS of one wave, in bytes: [accumulators (E doubles) | group partials (64 doubles) and shifted
// tile (64 · ((d + 1) | 1) doubles), d <= kPsShiftMaxD | tile (64 · (d | 1) floats) | counts (64 int)]
__host__ __device__ constexpr int ps_acc_bytes(int d, bool sums, int map) {
    return sums && map != kPsPacked ? 8 * ps_entries(d) : 0;
}
__host__ __device__ constexpr int ps_shift_bytes(int d, bool sums) {
    return sums && d <= kPsShiftMaxD ? 8 * (64 + kPsRows * ((d + 1) | 1)) : 0;
}
__host__ __device__ constexpr int ps_tile_bytes(int d) { return (4 * kPsRows * (d | 1) + 7) & ~7; }
__host__ __device__ constexpr int ps_wave_bytes(int d, bool ranks, bool sums, int map) {
    return ps_acc_bytes(d, sums, map) + ps_shift_bytes(d, sums) + ps_tile_bytes(d) +
           (ranks && map == kPsBlock ? 4 * 64 : 0);
}

// Between a wave's LDS stores and its loads of words other lanes stored (and back): LDS serves
// one wave's instructions in order, so this only keeps the compiler from moving them.
__device__ __forceinline__ void ps_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows [0, R) of the tile from the R·d contiguous floats at src (16-byte aligned, R % 4 == 0)
__device__ __forceinline__ void ps_stage(float* tile, const float* __restrict__ src, int R, int d, int dp,
                                         int lane) {
    const int nv = R * d / 4;
    for (int v = lane; v < nv; v += 64) {
        const float4 f = *reinterpret_cast<const float4*>(src + 4 * v);
        int row = (4 * v) / d, col = 4 * v - row * d;
        const float vals[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            tile[row * dp + col] = vals[e];
            if (++col == d) {
                col = 0;
                ++row;
            }
        }
    }
}

// entry e of a point's block: S1[a] (one = true, b = a) for e < d, else S2[a, b] with
// e − d = a(a+1)/2 + b, a >= b
__device__ __forceinline__ void ps_decode(int e, int d, int& a, int& b, bool& one) {
    one = e < d;
    if (one) {
        a = b = e;
        return;
    }
    const int p = e - d;
    int t = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    while (t * (t + 1) / 2 > p) --t;
    a = t;
    b = p - t * (t + 1) / 2;
}

// Σ over rows [r0, r1) of the tile, in increasing order, of (v_a − c_a)·(v_b − c_b), or of
// (v_a − c_a) for S1; every value converted to double before the subtraction
__device__ __forceinline__ double ps_rows_sum(const float* tile, int dp, int r0, int r1, int a, int b,
                                              bool one, double ca, double cb) {
    double acc = 0.0;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        const double va = (double)tile[r * dp + a] - ca;
        const double vb = one ? 1.0 : (double)tile[r * dp + b] - cb;
        acc = fma(va, vb, acc);
    }
    return acc;
}

// d <= kPsShiftMaxD.  Row `lane` of the shifted tile: double(v_k) − double(c_k) for k < d and
// 1.0 in column d (S1[a] is the product of column a with it), c the lane's point's draw 0
__device__ __forceinline__ void ps_shift_row(double* dt, const float* tile, const float* __restrict__ c, int lane,
                                             int R, int d, int dp, int dpd) {
    if (lane < R) {
        for (int k = 0; k < d; ++k) dt[lane * dpd + k] = (double)tile[lane * dp + k] - (double)c[k];
        dt[lane * dpd + d] = 1.0;
    }
}

// Σ over rows r0, r0 + step, ... < r1 of the shifted tile of column a times column b
__device__ __forceinline__ double ps_rows_dot(const double* dt, int dpd, int r0, int r1, int step, int a, int b) {
    double acc = 0.0;
#pragma unroll 4
    for (int r = r0; r < r1; r += step) acc = fma(dt[r * dpd + a], dt[r * dpd + b], acc);
    return acc;
}

// xs (d, points · N): the chunk's draws; x (d, points): the chunk's points (RANKS).
// rank (d, points) and sums (points blocks of 2d + d(d+1)/2 doubles) are the chunk's.
template <bool RANKS, bool SUMS, int MAP>
__global__ void __launch_bounds__(kPsThreads) point_stats_kernel(const float* __restrict__ xs,
                                                                 const float* __restrict__ x, int d, int N,
                                                                 int64_t points, int32_t* __restrict__ rank,
                                                                 double* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ps_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dp = d | 1, E = ps_entries(d), S = E + d;
    const int wave_bytes = ps_wave_bytes(d, RANKS, SUMS, MAP);
    const int acc_bytes = ps_acc_bytes(d, SUMS, MAP);
    unsigned char* mine = ps_lds + wave * wave_bytes;
    const bool shifted = SUMS && d <= kPsShiftMaxD;
    const int dpd = (d + 1) | 1;
    double* acc = reinterpret_cast<double*>(mine);
    double* prt = reinterpret_cast<double*>(mine + acc_bytes);
    double* dt = prt + 64;
    float* tile = reinterpret_cast<float*>(mine + acc_bytes + ps_shift_bytes(d, SUMS));

    if (MAP == kPsPacked) {
        const int per = kPsRows / N;  // points of a wave
        const int64_t i0 = ((int64_t)blockIdx.x * kPsWaves + wave) * per;
        if (i0 >= points) return;  // the whole wave; nothing below waits for it
        const int np = (int)(points - i0 < per ? points - i0 : per);
        const int R = np * N;
        ps_stage(tile, xs + i0 * N * d, R, d, dp, lane);
        ps_wave_sync();
        if (RANKS) {
            const bool on = lane < R;
            const int seg = on ? lane / N : 0;
            const int64_t i = i0 + seg;
            const unsigned long long rows = N == 64 ? ~0ull : ((1ull << N) - 1ull) << (seg * N);
            for (int k = 0; k < d; ++k) {
                const bool below = on && tile[lane * dp + k] < x[i * d + k];
                const int cnt = __popcll(__ballot(below) & rows);
                if (on && lane == seg * N) rank[i * d + k] = cnt;
            }
        }
        if (SUMS) {
            if (shifted) {
                ps_shift_row(dt, tile, xs + (i0 + (lane < R ? lane / N : 0)) * N * d, lane, R, d, dp, dpd);
                ps_wave_sync();
            }
            const int total = np * E;
            for (int t = lane; t < total; t += 64) {
                const int s = t / E, e = t - s * E;
                int a, b;
                bool one;
                ps_decode(e, d, a, b, one);
                const float* first = xs + (i0 + s) * N * d;  // draw 0 of the point: the shift
                const double ca = (double)first[a], cb = (double)first[b];
                double* out = sums + (i0 + s) * S;
                out[d + e] = shifted ? ps_rows_dot(dt, dpd, s * N, s * N + N, 1, a, one ? d : b)
                                     : ps_rows_sum(tile, dp, s * N, s * N + N, a, b, one, ca, cb);
                if (one) out[e] = ca;
            }
        }
    } else {
        constexpr int W = MAP == kPsBlock ? kPsWaves : 1;  // waves of a point
        const int64_t i = MAP == kPsBlock ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kPsWaves + wave;
        if (MAP == kPsWave && i >= points) return;  // the whole wave; this mapping has no barrier
        const float* src = xs + i * N * d;
        int cnt = 0;  // lane k: dimension k
        bool first = true;
        for (int r0 = (MAP == kPsBlock ? wave : 0) * kPsRows; r0 < N; r0 += kPsRows * W) {
            const int R = N - r0 < kPsRows ? N - r0 : kPsRows;
            ps_wave_sync();
            ps_stage(tile, src + (int64_t)r0 * d, R, d, dp, lane);
            ps_wave_sync();
            if (RANKS) {
                const bool on = lane < R;
                for (int k = 0; k < d; ++k) {
                    const bool below = on && tile[lane * dp + k] < x[i * d + k];
                    const int pc = __popcll(__ballot(below));
                    cnt += lane == k ? pc : 0;
                }
            }
            if (SUMS && shifted) {
                ps_shift_row(dt, tile, src, lane, R, d, dp, dpd);
                ps_wave_sync();
                // E <= 32: F = 64 / E groups of lanes share the rows, group g rows g, g + F, ...;
                // the groups' sums meet in LDS and are added in group order by group 0
                const int F = E <= 32 ? 64 / E : 1;
                for (int eb = 0; eb < E; eb += 64) {
                    const int g = F > 1 ? lane / E : 0;
                    int e = F > 1 ? lane - g * E : eb + lane;
                    bool mine_e = F > 1 ? g < F : e < E;
                    double part = 0.0;
                    if (mine_e) {
                        int a, b;
                        bool one;
                        ps_decode(e, d, a, b, one);
                        part = ps_rows_dot(dt, dpd, g, R, F, a, one ? d : b);
                    }
                    if (F > 1) {
                        prt[lane] = part;  // lane = g·E + e
                        ps_wave_sync();
                        mine_e = lane < E;
                        e = lane;
                        if (mine_e)
                            for (int k = 1; k < F; ++k) part += prt[k * E + lane];
                    }
                    if (mine_e) acc[e] = first ? part : acc[e] + part;
                }
            } else if (SUMS) {
                for (int e = lane; e < E; e += 64) {
                    int a, b;
                    bool one;
                    ps_decode(e, d, a, b, one);
                    const double part = ps_rows_sum(tile, dp, 0, R, a, b, one, (double)src[a], (double)src[b]);
                    acc[e] = first ? part : acc[e] + part;
                }
            }
            first = false;
        }
        if (MAP == kPsWave) {
            if (RANKS && lane < d) rank[i * d + lane] = cnt;
            if (SUMS) {
                double* out = sums + i * S;
                for (int e = lane; e < E; e += 64) {
                    out[d + e] = acc[e];
                    if (e < d) out[e] = (double)src[e];
                }
            }
        } else {
            // every wave has had a trip (N > 256: at least 5 trips)
            const int rk_off = acc_bytes + ps_shift_bytes(d, SUMS) + ps_tile_bytes(d);
            if (RANKS) reinterpret_cast<int*>(mine + rk_off)[lane] = cnt;
            __syncthreads();
            if (RANKS && tid < d) {
                int sum = 0;
#pragma unroll
                for (int w = 0; w < kPsWaves; ++w)
                    sum += reinterpret_cast<const int*>(ps_lds + w * wave_bytes + rk_off)[tid];
                rank[i * d + tid] = sum;
            }
            if (SUMS) {
                double* out = sums + i * S;
                for (int e = tid; e < E; e += kPsThreads) {
                    double sum = reinterpret_cast<const double*>(ps_lds)[e];
#pragma unroll
                    for (int w = 1; w < kPsWaves; ++w) sum += reinterpret_cast<const double*>(ps_lds + w * wave_bytes)[e];
                    out[d + e] = sum;
                    if (e < d) out[e] = (double)src[e];
                }
            }
        }
    }
}

// MaxDynamicSharedMemorySize of an instance = the largest request any launch of it has made in
// this process (the attribute belongs to the function, not to a chain)
hipError_t raise_lds_limit(const void* k, int mode, int map, size_t lds) {
    static std::mutex mu;
    static size_t limit[3][3] = {};
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[mode][map];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

template <bool RANKS, bool SUMS, int MAP>
hipError_t launch_map(const float* xs, const float* x, int d, int N, int64_t points, int64_t per_wg, int32_t* rank,
                      double* sums, hipStream_t st) {
    const size_t lds = (size_t)kPsWaves * ps_wave_bytes(d, RANKS, SUMS, MAP);
    const void* k = reinterpret_cast<const void*>(&point_stats_kernel<RANKS, SUMS, MAP>);
    const hipError_t e = raise_lds_limit(k, (RANKS ? 0 : 2) + (SUMS ? 0 : 1), MAP, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((point_stats_kernel<RANKS, SUMS, MAP>), dim3((unsigned)((points + per_wg - 1) / per_wg)),
                       dim3(kPsThreads), lds, st, xs, x, d, N, points, rank, sums);
    return hipGetLastError();
}

template <bool RANKS, bool SUMS>
hipError_t launch_stats(const float* xs, const float* x, int d, int N, int64_t points, int32_t* rank, double* sums,
                        hipStream_t st) {
    if (N <= kPsPackedMax)
        return launch_map<RANKS, SUMS, kPsPacked>(xs, x, d, N, points, (int64_t)kPsWaves * (kPsRows / N), rank, sums, st);
    if (N <= kPsWaveMax) return launch_map<RANKS, SUMS, kPsWave>(xs, x, d, N, points, kPsWaves, rank, sums, st);
    return launch_map<RANKS, SUMS, kPsBlock>(xs, x, d, N, points, 1, rank, sums, st);
}

}  // namespace
}  // namespace df

using namespace df;
using namespace df::api;

namespace df {
namespace api {

int point_check_sizes(const df_chain* c, int64_t n_points, int64_t n_draws, int64_t chunk) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (chunk < 0) return set_err(DF_ERR_SHAPE, "negative chunk size");
    if (n_draws <= 0 || n_draws % 4 != 0)
        return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4 (a Philox counter boundary)");
    if (chunk > kChunkMax) return set_err(DF_ERR_UNSUPPORTED, "a chunk holds at most 2^24 samples");
    if (n_draws > kDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    return DF_OK;
}

int point_draw_chunks(df_chain* c, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                      int64_t chunk, uint64_t seed, uint64_t offset, const PointOutputs& out, void* stream) {
    int32_t* const rank_out = out.rank;
    double* const sums_out = out.sums;
    float* const draws_out = out.draws;
    float* const quant_out = out.quant;
    // (the first use of the handle)
    int rc = sample_check_theta(c, theta_raw);
    if (rc != DF_OK) return rc;
    const int d = c->plan.d, n = c->plan.n;
    if (n_points > (INT64_MAX / 8) / n_draws / std::max(d, std::max(n, 1)))
        return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);

    // whole points per chunk
    const int64_t G = std::min(n_points, std::max<int64_t>(1, (chunk == 0 ? kChunkDefault : chunk) / n_draws));
    const int64_t step = G * n_draws;  // samples; <= 2^24
    if ((rc = reserve(c->d_mom_x, c->mom_x_cap, (int64_t)sizeof(float) * d * step, st, "point statistics sample")) !=
            DF_OK ||
        (n > 0 && (rc = reserve(c->d_hpd_th, c->hpd_th_cap, (int64_t)sizeof(float) * n * step, st,
                                "point statistics θ")) != DF_OK))
        return rc;
    float* xs = c->d_mom_x.as<float>();
    float* th = n > 0 ? c->d_hpd_th.as<float>() : nullptr;

    const int N = (int)n_draws;
    const int64_t S = 2 * (int64_t)d + (int64_t)d * (d + 1) / 2;
    for (int64_t p0 = 0; p0 < n_points; p0 += G) {
        const int64_t pts = std::min(G, n_points - p0);
        const int64_t len = pts * n_draws;
        const float* unused = nullptr;
        rc = sample_draw(c, xs, nullptr, 0, len, seed, offset + (uint64_t)((int64_t)d * p0 * (n_draws / 4)), stream,
                         &unused);
        if (rc != DF_OK) return rc;
        if (n > 0 && (rc = launch_theta_repeat(th, theta_raw + (int64_t)n * p0, n, n_draws, (int64_t)n * len, st)) != DF_OK)
            return rc;
        if ((rc = df_flow_forward_inplace(c, xs, th, len, stream)) != DF_OK) return rc;
        hipError_t e = hipSuccess;
        if (draws_out) {
            // the chunk's samples as they stand; a copy has no alignment rule
            e = hipMemcpyAsync(draws_out + (int64_t)d * p0 * n_draws, xs, sizeof(float) * (size_t)d * (size_t)len,
                               hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return hip_err(e, "hipMemcpyAsync(draws)");
        }
        const float* xp = x ? x + (int64_t)d * p0 : nullptr;
        int32_t* rp = rank_out ? rank_out + (int64_t)d * p0 : nullptr;
        double* sp = sums_out ? sums_out + S * p0 : nullptr;
        if (rank_out && sums_out)
            e = launch_stats<true, true>(xs, xp, d, N, pts, rp, sp, st);
        else if (rank_out)
            e = launch_stats<true, false>(xs, xp, d, N, pts, rp, nullptr, st);
        else if (sums_out)
            e = launch_stats<false, true>(xs, nullptr, d, N, pts, nullptr, sp, st);
        if (e != hipSuccess) return hip_err(e, "point statistics kernel launch");
        // df_flow_point_quantiles: the selection reads the chunk the reduction has read
        if (quant_out && (rc = launch_order_statistics(xs, d, N, pts, out.orders, out.n_orders,
                                                       quant_out + (int64_t)d * p0 * out.n_orders, st)) != DF_OK)
            return rc;
        // df_flow_point_histograms: the tables of the chunk's points
        if (out.counts && (rc = launch_draw_histograms(xs, d, N, pts, out.edges, out.hist,
                                                       out.counts + histogram_block_words(out.hist) * p0, st)) != DF_OK)
            return rc;
    }
    return DF_OK;
}

}  // namespace api
}  // namespace df

extern "C" {

int df_flow_point_stats(df_chain* c, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                        int64_t chunk, uint64_t seed, uint64_t offset, int32_t* rank_out, double* sums_out,
                        float* draws_out, void* stream) {
    const int rc = point_check_sizes(c, n_points, n_draws, chunk);
    if (rc != DF_OK) return rc;
    if (!rank_out && !sums_out && !draws_out)
        return set_err(DF_ERR_INVALID, "no output: rank_out, sums_out and draws_out are all null");
    if (rank_out && !x) return set_err(DF_ERR_INVALID, "rank_out needs the points x (null input array)");
    if (n_points == 0) return DF_OK;
    PointOutputs out;
    out.rank = rank_out;
    out.sums = sums_out;
    out.draws = draws_out;
    return point_draw_chunks(c, x, theta_raw, n_points, n_draws, chunk, seed, offset, out, stream);
}

}  // extern "C"
