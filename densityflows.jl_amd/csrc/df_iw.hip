// df_iw.hip — importance weights of per-point draws, on the device:
//   df_importance_weights    per point the stabilised weights w_ij = expf(logw_ij − m_i), m_i the
//                            largest non-NaN log-weight, and {m, W1 = Σ w, W2 = Σ w², #{w > 0}}:
//                            the log-evidence and the effective sample size of every point
//   df_draw_weighted_stats   the weighted sibling of point_stats_kernel (df_pstats.hip) over a
//                            caller-owned (d, n_points · n_draws) array of draws and its weights:
//                            per dimension the weight below the point (the weighted SBC
//                            statistic) and the weighted shifted sums behind mean and covariance
// Both run on the current device on the caller's arrays, per point, in fp64, in a fixed order
// without atomics; nothing is zeroed, nothing synchronises.  With N = n_draws both take the
// point mapping of point_stats_kernel:
//   N <= 64    packed: 64 / N points per wave, point s in rows (lanes) [s·N, (s+1)·N); 4 waves
//              (256 / N points) per workgroup
//   N <= 256   a wave per point, 4 points per workgroup, no workgroup barrier
//   above      a workgroup per point
//
// importance_weights_kernel.  Two passes over a point's logw (N floats; the second pass finds
// them in the L2): the maximum (fmaxf from NaN, its identity: exact in any order), then
// w = expf(logw − m) — one Float32 subtraction, the library's expf — stored, converted to double
// and summed: W1 += w, W2 += w·w (the product of two floats is exact in fp64), n_pos += w > 0.
//   packed     lane = draw, 4-byte loads; the N terms of a point are added in draw order by the
//              point's first lane (through LDS)
//   wave       lane l holds draws 4l .. 4l + 3 (one 16-byte load, a 16-byte store where w_out is
//              16-byte aligned): its four terms in increasing order from 0, then the 64 lanes by
//              the butterfly tree (partner lane ^ 32, ^ 16, ..., ^ 1; a lane without draws adds 0)
//   workgroup  thread t holds the 16-byte vectors t, t + 256, ...: its terms in increasing order,
//              the lanes of a wave by the same tree, the 4 waves in wave order,
//              ((w0 + w1) + w2) + w3, behind one barrier (the maximum: a barrier of its own)
//
// draw_weighted_stats_kernel.  point_stats_kernel's unit of work — a wave and a tile of 64 draws
// (rows) staged with 16-byte loads into LDS at row stride d | 1 — with the tile's 64 weights
// beside it as doubles.  The sums: lane = entry, E = d + d(d+1)/2 entries (S1w[a], then
// S2w[a, b], a >= b); a lane walks the rows in increasing order with
//   acc = fma(w·(v_a − c_a), v_b − c_b, acc)      (S1w: v_b − c_b is 1.0)
// every value converted to double first, w·(v_a − c_a) one fp64 multiply.  d <= 16 reads the
// shifted-double tile (v_k − c_k, a column of ones), and while E <= 32 (d <= 6) F = 64 / E groups
// of lanes share a tile's rows, group g rows g, g + F, ..., added in group order — the paths of
// point_stats_kernel.  The order of every such sum is that kernel's: rows in increasing order
// inside a trip (inside a group, then the groups in order), trips in increasing order inside a
// wave (wave w of a workgroup takes trips w, w + 4, ...), waves in wave order.  With unit weights
// w·(v_a − c_a) is (v_a − c_a): entries [2, ..) of a block are df_flow_point_stats' block of the
// same draws bit for bit.
// The columns — wrank[k] = Σ w·[v_k < x_k] for k < d, W1 = Σ w, W2 = Σ w·w — have an order of
// their own: lane = column (d + 2 of them, 64 at a time); a lane walks the tile's rows in
// increasing order from 0, adding w where the Float32 comparison holds (nothing otherwise: a NaN
// weight reaches wrank[k] only through rows below the point); up to d = 16 the G = 64 / (d + 2)
// groups of lanes share the rows, group g rows g, g + G, ..., and the G sums are added in group
// order; a trip's sum is added to the wave's running value, trips in increasing order, and a
// workgroup's 4 waves in wave order behind the one barrier.  Packed: one walk over the point's N
// rows, no groups.
// No atomics, no zeroing pass, one store per (point, column) and per (point, entry); the order
// depends on (d, N) alone, neither on the other points nor on the grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kIwThreads = 256;  // 4 waves
constexpr int kIwWaves = kIwThreads / 64;
constexpr int kIwRows = 64;         // draws of a tile: a lane per row
constexpr int kIwPackedMax = 64;    // N up to which several points share a wave
constexpr int kIwWaveMax = 256;     // N up to which a point is one wave's
constexpr int kIwShiftMaxD = 16;    // d up to which the sums read a tile of shifted doubles
constexpr int64_t kIwDrawsMax = (int64_t)1 << 24;

enum IwMap { kIwPacked = 0, kIwWave = 1, kIwBlock = 2 };

// Between a wave's LDS stores and its loads of words other lanes stored (and back): LDS serves
// one wave's instructions in order, so this only keeps the compiler from moving them.
__device__ __forceinline__ void iw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float iw_wave_max(float m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    return m;
}

__device__ __forceinline__ double iw_wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// the weights of one 16-byte vector of logw, stored and added to the thread's sums in
// increasing order
__device__ __forceinline__ void iw_vector(const float4 f, float m, float* __restrict__ dst, bool vec, double& s1,
                                          double& s2, int& pos) {
    const float wv[4] = {expf(f.x - m), expf(f.y - m), expf(f.z - m), expf(f.w - m)};
    if (dst) {
        if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(wv[0], wv[1], wv[2], wv[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e] = wv[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double x = (double)wv[e];
        s1 += x;
        s2 += x * x;
        pos += wv[e] > 0.f ? 1 : 0;
    }
}

// logw, w_out (points · N); stats: 4 doubles per point.  vec: w_out is 16-byte aligned.
template <int MAP>
__global__ void __launch_bounds__(kIwThreads) importance_weights_kernel(const float* __restrict__ logw, int N,
                                                                        int64_t points, float* __restrict__ w_out,
                                                                        int vec, double* __restrict__ stats) {
    __shared__ double iw_lds[kIwWaves][kIwRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float none = __int_as_float(0x7fc00000);  // fmaxf's identity

    if (MAP == kIwPacked) {
        const int per = kIwRows / N;  // points of a wave
        const int64_t i0 = ((int64_t)blockIdx.x * kIwWaves + wave) * per;
        if (i0 >= points) return;  // the whole wave; nothing below waits for it
        const int np = (int)(points - i0 < per ? points - i0 : per);
        const int R = np * N;
        const bool on = lane < R;
        const int row0 = on ? lane / N * N : 0;  // the first lane of this lane's point
        const float lw = on ? logw[i0 * N + lane] : none;
        float* mine_f = reinterpret_cast<float*>(iw_lds[wave]);
        mine_f[lane] = lw;
        iw_wave_sync();
        float m = none;
        for (int j = 0; j < N; ++j) m = fmaxf(m, mine_f[row0 + j]);
        const float wv = expf(lw - m);
        if (on && w_out) w_out[i0 * N + lane] = wv;
        if (stats) {
            iw_wave_sync();  // the maxima are read
            iw_lds[wave][lane] = (double)wv;
            iw_wave_sync();
            if (on && lane == row0) {
                double s1 = 0.0, s2 = 0.0;
                int pos = 0;
                for (int j = 0; j < N; ++j) {
                    const double x = iw_lds[wave][row0 + j];
                    s1 += x;
                    s2 += x * x;
                    pos += x > 0.0 ? 1 : 0;
                }
                double* out = stats + 4 * (i0 + lane / N);
                out[0] = (double)m;
                out[1] = s1;
                out[2] = s2;
                out[3] = (double)pos;
            }
        }
    } else if (MAP == kIwWave) {
        const int64_t i = (int64_t)blockIdx.x * kIwWaves + wave;
        if (i >= points) return;  // the whole wave; this mapping has no barrier
        const bool on = lane < N / 4;
        float4 f = make_float4(none, none, none, none);
        if (on) f = *reinterpret_cast<const float4*>(logw + i * N + 4 * lane);
        const float m = iw_wave_max(fmaxf(fmaxf(fmaxf(f.x, f.y), f.z), f.w));
        double s1 = 0.0, s2 = 0.0;
        int pos = 0;
        if (on) iw_vector(f, m, w_out ? w_out + i * N + 4 * lane : nullptr, vec != 0, s1, s2, pos);
        if (stats) {
            s1 = iw_wave_sum(s1);
            s2 = iw_wave_sum(s2);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) pos += __shfl_xor(pos, off, 64);
            if (lane == 0) {
                double* out = stats + 4 * i;
                out[0] = (double)m;
                out[1] = s1;
                out[2] = s2;
                out[3] = (double)pos;
            }
        }
    } else {
        const int64_t i = blockIdx.x;
        const float* src = logw + i * N;
        const int nv = N / 4;
        float m = none;
        for (int v = tid; v < nv; v += kIwThreads) {
            const float4 f = *reinterpret_cast<const float4*>(src + 4 * v);
            m = fmaxf(fmaxf(fmaxf(fmaxf(m, f.x), f.y), f.z), f.w);
        }
        m = iw_wave_max(m);
        float* maxes = reinterpret_cast<float*>(iw_lds[0]);
        if (lane == 0) maxes[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(maxes[0], maxes[1]), fmaxf(maxes[2], maxes[3]));
        double s1 = 0.0, s2 = 0.0;
        int pos = 0;
        for (int v = tid; v < nv; v += kIwThreads) {
            const float4 f = *reinterpret_cast<const float4*>(src + 4 * v);
            iw_vector(f, m, w_out ? w_out + i * N + 4 * v : nullptr, vec != 0, s1, s2, pos);
        }
        if (stats) {
            s1 = iw_wave_sum(s1);
            s2 = iw_wave_sum(s2);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) pos += __shfl_xor(pos, off, 64);
            // (row 0 holds the maxima: the partial sums go to rows 1 .. 3 and a word apart)
            double* part = iw_lds[1];
            if (lane == 0) {
                part[3 * wave] = s1;
                part[3 * wave + 1] = s2;
                part[3 * wave + 2] = (double)pos;
            }
            __syncthreads();
            if (tid == 0) {
                double t1 = part[0], t2 = part[1], tp = part[2];
#pragma unroll
                for (int w = 1; w < kIwWaves; ++w) {
                    t1 += part[3 * w];
                    t2 += part[3 * w + 1];
                    tp += part[3 * w + 2];
                }
                double* out = stats + 4 * i;
                out[0] = (double)m;
                out[1] = t1;
                out[2] = t2;
                out[3] = tp;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------

__host__ __device__ constexpr int ws_entries(int d) { return d + d * (d + 1) / 2; }

// LDS of one wave, in bytes: [accumulators (E doubles) | group partials (64 doubles) and, with
// sums, shifted tile (64 · ((d + 1) | 1) doubles), d <= kIwShiftMaxD | weights (64 doubles) | tile
// (64 · (d | 1) floats, at least d + 2 doubles: a workgroup's waves leave their columns there
// after their last trip)].  d = 32: 13,440 bytes, three workgroups per CU as point_stats_kernel.
__host__ __device__ constexpr int ws_acc_bytes(int d, bool sums, int map) {
    return sums && map != kIwPacked ? 8 * ws_entries(d) : 0;
}
__host__ __device__ constexpr int ws_shift_bytes(int d, bool sums) {
    return d <= kIwShiftMaxD ? 8 * (64 + (sums ? kIwRows * ((d + 1) | 1) : 0)) : 0;
}
__host__ __device__ constexpr int ws_tile_bytes(int d) {
    return 4 * kIwRows * (d | 1) > 8 * (d + 2) ? (4 * kIwRows * (d | 1) + 15) & ~15 : (8 * (d + 2) + 15) & ~15;
}
__host__ __device__ constexpr int ws_wave_bytes(int d, bool sums, int map) {
    return ((ws_acc_bytes(d, sums, map) + 15) & ~15) + ws_shift_bytes(d, sums) + 8 * kIwRows + ws_tile_bytes(d);
}

// rows [0, R) of the tile from the R·d contiguous floats at src (16-byte aligned, R % 4 == 0)
__device__ __forceinline__ void ws_stage(float* tile, const float* __restrict__ src, int R, int d, int dp, int lane) {
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

// entry e of a point's block: S1w[a] (one = true, b = a) for e < d, else S2w[a, b] with
// e − d = a(a+1)/2 + b, a >= b
__device__ __forceinline__ void ws_decode(int e, int d, int& a, int& b, bool& one) {
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

// Σ over rows [r0, r1) of the tile, in increasing order, of w·(v_a − c_a)·(v_b − c_b), or of
// w·(v_a − c_a) for S1w; every value converted to double first.  wd: the weights of rows r0 ..
__device__ __forceinline__ double ws_rows_sum(const float* tile, const double* wd, int dp, int r0, int r1, int a, int b,
                                              bool one, double ca, double cb) {
    double acc = 0.0;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        const double va = (double)tile[r * dp + a] - ca;
        const double vb = one ? 1.0 : (double)tile[r * dp + b] - cb;
        acc = fma(wd[r] * va, vb, acc);
    }
    return acc;
}

// d <= kIwShiftMaxD.  Row `lane` of the shifted tile: double(v_k) − double(c_k) for k < d and
// 1.0 in column d, c the lane's point's draw 0
__device__ __forceinline__ void ws_shift_row(double* dt, const float* tile, const float* __restrict__ c, int lane, int R,
                                             int d, int dp, int dpd) {
    if (lane < R) {
        for (int k = 0; k < d; ++k) dt[lane * dpd + k] = (double)tile[lane * dp + k] - (double)c[k];
        dt[lane * dpd + d] = 1.0;
    }
}

// Σ over rows r0, r0 + step, ... < r1 of the shifted tile of w times column a times column b
__device__ __forceinline__ double ws_rows_dot(const double* dt, const double* wd, int dpd, int r0, int r1, int step,
                                              int a, int b) {
    double acc = 0.0;
#pragma unroll 4
    for (int r = r0; r < r1; r += step) acc = fma(wd[r] * dt[r * dpd + a], dt[r * dpd + b], acc);
    return acc;
}

// column t over rows r0, r0 + step, ... < r1 in increasing order: t < d the weight of the rows
// with v_t < xk, t == d Σ w, t == d + 1 Σ w·w
__device__ __forceinline__ double ws_col_sum(const float* tile, const double* wd, int dp, int r0, int r1, int step,
                                             int t, int d, float xk) {
    double acc = 0.0;
    if (t < d) {
        for (int r = r0; r < r1; r += step) {
            const double ww = wd[r];
            acc += tile[r * dp + t] < xk ? ww : 0.0;
        }
    } else if (t == d) {
        for (int r = r0; r < r1; r += step) acc += wd[r];
    } else {
        for (int r = r0; r < r1; r += step) acc += wd[r] * wd[r];
    }
    return acc;
}

// xs (d, points · N): the draws; w (points · N): their weights; x (d, points): the points
// (RANKS).  wrank (d, points) and sums (points blocks of 2 + 2d + d(d+1)/2 doubles).
template <bool RANKS, bool SUMS, int MAP>
__global__ void __launch_bounds__(kIwThreads) draw_weighted_stats_kernel(const float* __restrict__ xs,
                                                                         const float* __restrict__ w,
                                                                         const float* __restrict__ x, int d, int N,
                                                                         int64_t points, double* __restrict__ wrank,
                                                                         double* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dp = d | 1, E = ws_entries(d), S = 2 + E + d;
    const int wave_bytes = ws_wave_bytes(d, SUMS, MAP);
    const int acc_bytes = (ws_acc_bytes(d, SUMS, MAP) + 15) & ~15;
    const int shift_bytes = ws_shift_bytes(d, SUMS);
    const int tile_off = acc_bytes + shift_bytes + 8 * kIwRows;
    unsigned char* mine = ws_lds + wave * wave_bytes;
    const bool shifted = SUMS && d <= kIwShiftMaxD;
    const int dpd = (d + 1) | 1;
    double* acc = reinterpret_cast<double*>(mine);
    double* prt = reinterpret_cast<double*>(mine + acc_bytes);
    double* dt = prt + 64;
    double* wd = reinterpret_cast<double*>(mine + acc_bytes + shift_bytes);
    float* tile = reinterpret_cast<float*>(mine + tile_off);
    // the columns asked for: ranks [0, d), W1 and W2 [d, d + 2)
    const int t_lo = RANKS ? 0 : d, t_hi = SUMS ? d + 2 : d, nc = t_hi - t_lo;

    if (MAP == kIwPacked) {
        const int per = kIwRows / N;  // points of a wave
        const int64_t i0 = ((int64_t)blockIdx.x * kIwWaves + wave) * per;
        if (i0 >= points) return;  // the whole wave; nothing below waits for it
        const int np = (int)(points - i0 < per ? points - i0 : per);
        const int R = np * N;
        ws_stage(tile, xs + i0 * N * d, R, d, dp, lane);
        if (lane < R) wd[lane] = (double)w[i0 * N + lane];
        iw_wave_sync();
        for (int tt = lane; tt < np * nc; tt += 64) {
            const int s = tt / nc, t = t_lo + tt - s * nc;
            const float xk = t < d ? x[(i0 + s) * d + t] : 0.f;
            const double v = ws_col_sum(tile, wd, dp, s * N, s * N + N, 1, t, d, xk);
            if (t < d)
                wrank[(i0 + s) * d + t] = v;
            else
                sums[(i0 + s) * S + (t - d)] = v;
        }
        if (SUMS) {
            if (shifted) {
                ws_shift_row(dt, tile, xs + (i0 + (lane < R ? lane / N : 0)) * N * d, lane, R, d, dp, dpd);
                iw_wave_sync();
            }
            const int total = np * E;
            for (int t = lane; t < total; t += 64) {
                const int s = t / E, e = t - s * E;
                int a, b;
                bool one;
                ws_decode(e, d, a, b, one);
                const float* first = xs + (i0 + s) * N * d;  // draw 0 of the point: the shift
                const double ca = (double)first[a], cb = (double)first[b];
                double* out = sums + (i0 + s) * S + 2;
                out[d + e] = shifted ? ws_rows_dot(dt, wd, dpd, s * N, s * N + N, 1, a, one ? d : b)
                                     : ws_rows_sum(tile, wd, dp, s * N, s * N + N, a, b, one, ca, cb);
                if (one) out[e] = ca;
            }
        }
    } else {
        constexpr int W = MAP == kIwBlock ? kIwWaves : 1;  // waves of a point
        const int64_t i = MAP == kIwBlock ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kIwWaves + wave;
        if (MAP == kIwWave && i >= points) return;  // the whole wave; this mapping has no barrier
        const float* src = xs + i * N * d;
        const float* wsrc = w + i * N;
        // columns t_lo + lane and t_lo + lane + 64 (d + 2 <= 66 columns).  d <= kIwShiftMaxD (at
        // most 18 columns): G = 64 / (d + 2) groups of lanes share a tile's rows, group g rows g,
        // g + G, ...; the groups' sums meet in LDS and are added in group order by group 0.  G and
        // a column's lanes follow from d alone, not from the outputs asked for: the same bits
        const int ncw = d + 2;
        const int G = d <= kIwShiftMaxD ? 64 / ncw : 1;
        const int cg = G > 1 ? lane / ncw : 0;
        const int tc0 = G > 1 ? lane - cg * ncw : t_lo + lane, tc1 = tc0 + 64;
        const bool on0 = (G > 1 ? cg < G && tc0 >= t_lo : true) && tc0 < t_hi;    // this lane walks rows of column tc0
        const bool own0 = on0 && cg == 0;                // and keeps its running value
        const bool on1 = G == 1 && tc1 < t_hi;
        const float xk0 = on0 && tc0 < d ? x[i * d + tc0] : 0.f;
        const float xk1 = on1 && tc1 < d ? x[i * d + tc1] : 0.f;
        double c0 = 0.0, c1 = 0.0;
        bool first = true;
        for (int r0 = (MAP == kIwBlock ? wave : 0) * kIwRows; r0 < N; r0 += kIwRows * W) {
            const int R = N - r0 < kIwRows ? N - r0 : kIwRows;
            iw_wave_sync();
            ws_stage(tile, src + (int64_t)r0 * d, R, d, dp, lane);
            if (lane < R) wd[lane] = (double)wsrc[r0 + lane];
            iw_wave_sync();
            {
                double part = on0 ? ws_col_sum(tile, wd, dp, cg, R, G, tc0, d, xk0) : 0.0;
                if (G > 1) {
                    prt[lane] = part;  // lane = cg·(d + 2) + column
                    iw_wave_sync();
                    if (own0)
                        for (int k = 1; k < G; ++k) part += prt[k * ncw + lane];
                }
                if (own0) c0 = first ? part : c0 + part;
            }
            if (on1) {
                const double part = ws_col_sum(tile, wd, dp, 0, R, 1, tc1, d, xk1);
                c1 = first ? part : c1 + part;
            }
            if (SUMS && shifted) {
                ws_shift_row(dt, tile, src, lane, R, d, dp, dpd);
                iw_wave_sync();
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
                        ws_decode(e, d, a, b, one);
                        part = ws_rows_dot(dt, wd, dpd, g, R, F, a, one ? d : b);
                    }
                    if (F > 1) {
                        prt[lane] = part;  // lane = g·E + e
                        iw_wave_sync();
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
                    ws_decode(e, d, a, b, one);
                    const double part =
                        ws_rows_sum(tile, wd, dp, 0, R, a, b, one, (double)src[a], (double)src[b]);
                    acc[e] = first ? part : acc[e] + part;
                }
            }
            first = false;
        }
        if (MAP == kIwWave) {
            if (own0) {
                if (tc0 < d)
                    wrank[i * d + tc0] = c0;
                else
                    sums[i * S + (tc0 - d)] = c0;
            }
            if (on1) {
                if (tc1 < d)
                    wrank[i * d + tc1] = c1;
                else
                    sums[i * S + (tc1 - d)] = c1;
            }
            if (SUMS) {
                iw_wave_sync();
                double* out = sums + i * S + 2;
                for (int e = lane; e < E; e += 64) {
                    out[d + e] = acc[e];
                    if (e < d) out[e] = (double)src[e];
                }
            }
        } else {
            // every wave has had a trip (N > 256: at least 5 trips); its tile is read: the wave's
            // columns take the tile's place
            iw_wave_sync();
            double* col = reinterpret_cast<double*>(tile);
            if (own0) col[tc0 - t_lo] = c0;
            if (on1) col[tc1 - t_lo] = c1;
            __syncthreads();
            if (tid < nc) {
                double sum = reinterpret_cast<const double*>(ws_lds + tile_off)[tid];
#pragma unroll
                for (int wv = 1; wv < kIwWaves; ++wv)
                    sum += reinterpret_cast<const double*>(ws_lds + wv * wave_bytes + tile_off)[tid];
                const int t = t_lo + tid;
                if (t < d)
                    wrank[i * d + t] = sum;
                else
                    sums[i * S + (t - d)] = sum;
            }
            if (SUMS) {
                double* out = sums + i * S + 2;
                for (int e = tid; e < E; e += kIwThreads) {
                    double sum = reinterpret_cast<const double*>(ws_lds)[e];
#pragma unroll
                    for (int wv = 1; wv < kIwWaves; ++wv)
                        sum += reinterpret_cast<const double*>(ws_lds + wv * wave_bytes)[e];
                    out[d + e] = sum;
                    if (e < d) out[e] = (double)src[e];
                }
            }
        }
    }
}

// MaxDynamicSharedMemorySize of an instance = the largest request any launch of it has made on
// this device in this process (the attribute belongs to a device's copy of the function, not to
// a call, and these calls run on whichever device is current); past kIwDevices ordinals it is
// set at every launch
constexpr int kIwDevices = 64;
hipError_t raise_lds_limit(const void* k, int mode, int map, size_t lds) {
    static std::mutex mu;
    static size_t limit[kIwDevices][3][3] = {};
    int dev = 0;
    hipError_t e0 = hipGetDevice(&dev);
    if (e0 != hipSuccess) return e0;
    if (dev < 0 || dev >= kIwDevices) return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[dev][mode][map];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

int64_t map_blocks(int N, int64_t points) {
    const int64_t per_wg = N <= kIwPackedMax ? (int64_t)kIwWaves * (kIwRows / N) : N <= kIwWaveMax ? kIwWaves : 1;
    return (points + per_wg - 1) / per_wg;
}

template <bool RANKS, bool SUMS, int MAP>
hipError_t launch_ws_map(const float* xs, const float* w, const float* x, int d, int N, int64_t points, double* wrank,
                         double* sums, hipStream_t st) {
    const size_t lds = (size_t)kIwWaves * ws_wave_bytes(d, SUMS, MAP);
    const void* k = reinterpret_cast<const void*>(&draw_weighted_stats_kernel<RANKS, SUMS, MAP>);
    const hipError_t e = raise_lds_limit(k, (RANKS ? 0 : 2) + (SUMS ? 0 : 1), MAP, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((draw_weighted_stats_kernel<RANKS, SUMS, MAP>), dim3((unsigned)map_blocks(N, points)),
                       dim3(kIwThreads), lds, st, xs, w, x, d, N, points, wrank, sums);
    return hipGetLastError();
}

template <bool RANKS, bool SUMS>
hipError_t launch_ws(const float* xs, const float* w, const float* x, int d, int N, int64_t points, double* wrank,
                     double* sums, hipStream_t st) {
    if (N <= kIwPackedMax) return launch_ws_map<RANKS, SUMS, kIwPacked>(xs, w, x, d, N, points, wrank, sums, st);
    if (N <= kIwWaveMax) return launch_ws_map<RANKS, SUMS, kIwWave>(xs, w, x, d, N, points, wrank, sums, st);
    return launch_ws_map<RANKS, SUMS, kIwBlock>(xs, w, x, d, N, points, wrank, sums, st);
}

template <int MAP>
hipError_t launch_iw_map(const float* logw, int N, int64_t points, float* w_out, double* stats, hipStream_t st) {
    const int vec = reinterpret_cast<uintptr_t>(w_out) % 16 == 0 ? 1 : 0;
    hipLaunchKernelGGL((importance_weights_kernel<MAP>), dim3((unsigned)map_blocks(N, points)), dim3(kIwThreads), 0, st,
                       logw, N, points, w_out, vec, stats);
    return hipGetLastError();
}

// the rules both calls share on n_points and n_draws, in their order
int check_points_draws(int64_t n_points, int64_t n_draws) {
    if (n_points < 0) return api::set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0)
        return api::set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kIwDrawsMax) return api::set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    return DF_OK;
}

}  // namespace
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_importance_weights(const float* logw, int64_t n_points, int64_t n_draws, float* w_out, double* stats_out,
                          void* stream) {
    const int rc = check_points_draws(n_points, n_draws);
    if (rc != DF_OK) return rc;
    if (!logw) return set_err(DF_ERR_INVALID, "null logw array");
    if (reinterpret_cast<uintptr_t>(logw) % 16 != 0) return set_err(DF_ERR_INVALID, "logw must be 16-byte aligned");
    if (!w_out && !stats_out) return set_err(DF_ERR_INVALID, "no output: w_out and stats_out are both null");
    if (n_points > (INT64_MAX / 8) / n_draws) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    if (n_points == 0) return DF_OK;
    const int N = (int)n_draws;
    if (map_blocks(N, n_points) > 0x7fffffff) return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = N <= kIwPackedMax ? launch_iw_map<kIwPacked>(logw, N, n_points, w_out, stats_out, st)
                         : N <= kIwWaveMax ? launch_iw_map<kIwWave>(logw, N, n_points, w_out, stats_out, st)
                                           : launch_iw_map<kIwBlock>(logw, N, n_points, w_out, stats_out, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "importance weights kernel launch");
}

int df_draw_weighted_stats(const float* xs, const float* w, const float* x, int d, int64_t n_points, int64_t n_draws,
                           double* wrank_out, double* sums_out, void* stream) {
    if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
    const int rc = check_points_draws(n_points, n_draws);
    if (rc != DF_OK) return rc;
    if (!xs || !w) return set_err(DF_ERR_INVALID, "null xs or w array");
    if (reinterpret_cast<uintptr_t>(xs) % 16 != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0)
        return set_err(DF_ERR_INVALID, "xs and w must be 16-byte aligned");
    if (!wrank_out && !sums_out) return set_err(DF_ERR_INVALID, "no output: wrank_out and sums_out are both null");
    if (wrank_out && !x) return set_err(DF_ERR_INVALID, "wrank_out needs the points x (null input array)");
    // the draws' floats and the blocks' doubles (at most 2 + 2·64 + 2080 per point)
    const int64_t per_point = n_draws * d > 2 + 2 * d + d * (d + 1) / 2 ? n_draws * d : 2 + 2 * d + d * (d + 1) / 2;
    if (n_points > (INT64_MAX / 8) / per_point) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    if (n_points == 0) return DF_OK;
    const int N = (int)n_draws;
    if (map_blocks(N, n_points) > 0x7fffffff) return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (wrank_out && sums_out)
        e = launch_ws<true, true>(xs, w, x, d, N, n_points, wrank_out, sums_out, st);
    else if (wrank_out)
        e = launch_ws<true, false>(xs, w, x, d, N, n_points, wrank_out, nullptr, st);
    else
        e = launch_ws<false, true>(xs, w, nullptr, d, N, n_points, nullptr, sums_out, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "weighted statistics kernel launch");
}

}  // extern "C"
