// df_resample.hip — importance resampling of per-point draws, on the device:
//   df_draw_resample   per point n_out picks among its n_draws weighted draws (systematic,
//                      stratified or multinomial) and, gathered, the picked rows: equally
//                      weighted draws that every per-point call of the library takes unchanged
// Everything is integer arithmetic, so the picks are defined exactly (the header states the
// contract) and depend neither on the mapping nor on the grid nor on the other points:
//   quantise  a weight takes part when its bits lie in [1, 0x7f7fffff] (finite, > 0).  With the
//             largest such weight wmax = f·2^e, f in [0.5, 1), q_j = rint(w_j·2^(32 − e)) half
//             to even, formed from the weight's bits by shifts: no conversion, no rounding mode
//   scan      I_j = q_0 + ... + q_j (the inclusive sums: C_{j+1} of the header), T = I_{N−1}
//   pick      the number of j' in [0, N − 2] with I_j'·D <= num·T, by a branch-free binary search
//             of ceil(log2 N) steps; each step is one 8-byte read and one 128-bit comparison
//             (__umul64hi and the low product).  num < D makes num·T < I_{N−1}·D, so the count
//             over [0, N − 2] is the count over all: the result lies in [0, N − 1] for any
//             content of w, and I_j > I_{j−1} at the result, that is q_j > 0.
// With N = n_draws the scan lives
//   N <= 256    in the wave's 2 KiB slice of LDS: a wave per point, 4 points per workgroup, no
//               workgroup barrier; lane l holds draws 4l .. 4l + 3 (one 16-byte load)
//   N <= 4096   in 32 KiB of LDS: a workgroup per point, trips of 1024 draws with a carry
//   above       in the caller's cdf_ws: resample_scan_kernel, a workgroup per point, trips of 4096
//               draws (16 per thread, the next trip's loads under this trip's scan), then
//               resample_pick_kernel over (point, 256 picks), which searches global memory
// The picks: a wave takes a tile of 64 picks, lane = pick; every lane computes its own Philox
// block.  The gather: the tile's lanes walk its 64·d output floats in order (coalesced stores),
// float e reads column e % d of the row picked by lane e / d (a lane permute); a pick of −1
// writes NaN and reads nothing.  Nothing is zeroed, nothing synchronises, no atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "densityflows_hip.h"
#include "df_handle.h"
#include "df_philox.h"
#include "df_wscale.h"

namespace df {
namespace {

constexpr int kRsThreads = 256;  // 4 waves
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsWaveMax = 256;                   // N up to which a point is one wave's
constexpr int kRsLdsMax = DF_RESAMPLE_LDS_DRAWS;  // N up to which a workgroup keeps the scan in LDS
constexpr int kRsScanVectors = 4;                 // 16-byte vectors a thread of the streamed scan holds per trip
constexpr int64_t kRsDrawsMax = (int64_t)1 << 24;
constexpr int64_t kRsOutMax = (int64_t)1 << 24;

struct RsArgs {
    const float* xs;
    int d, N;
    int64_t K;
    int method;
    uint32_t key0, key1;
    uint64_t offset;
    float* xs_out;
    int32_t* idx_out;
};

// Between a wave's LDS stores and its loads of words other lanes stored: LDS serves one wave's
// instructions in order, so this only keeps the compiler from moving them.
__device__ __forceinline__ void rs_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rs_key, rs_max4, rs_wave_max, rs_exponent, rs_quant: df_wscale.h (the quantiser the weighted
// quantiles and tables share)

__device__ __forceinline__ uint64_t rs_shfl_up(uint64_t v, int off) {
    return (uint64_t)__shfl_up((unsigned long long)v, (unsigned)off, 64);
}

// The lanes' sums (lanes in draw order) into the sum of the lanes before this one; total: the
// wave's sum.
__device__ __forceinline__ uint64_t rs_wave_before(uint64_t mine, int lane, uint64_t& total) {
    uint64_t s = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = rs_shfl_up(s, off);
        if (lane >= off) s += t;
    }
    total = (uint64_t)__shfl((unsigned long long)s, 63, 64);
    return s - mine;
}

// the V consecutive 16-byte vectors of thread slot `slot` (zeros past the nv vectors of the point)
template <int V>
__device__ __forceinline__ void rs_load_slot(const float* __restrict__ w, int slot, int nv, float4 f[V]) {
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const int v = slot * V + u;
        f[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < nv) f[u] = *reinterpret_cast<const float4*>(w + 4 * (int64_t)v);
    }
}

// A workgroup scans the N weights at w into dst[0 .. N) (LDS or global) and returns T.  Two
// passes over w: the largest weight that takes part, then trips of 1024·V draws — thread t holds
// the V consecutive 16-byte vectors V·t .. V·t + V − 1 of the trip, loaded one trip ahead — with
// the carry of the trips before.  part: 3·kRsWaves words of LDS.  Every thread of the workgroup
// calls this; the caller puts a barrier (or a launch) between the stores to dst and their readers.
template <int V>
__device__ __forceinline__ uint64_t rs_block_scan(const float* __restrict__ w, int N, uint64_t* dst, uint64_t* part,
                                                  int tid) {
    const int lane = tid & 63, wave = tid >> 6, nv = N / 4;
    uint32_t mx = 0u;
#pragma unroll 4
    for (int v = tid; v < nv; v += kRsThreads) {
        const float4 f = *reinterpret_cast<const float4*>(w + 4 * (int64_t)v);
        const uint32_t k[4] = {rs_key(f.x), rs_key(f.y), rs_key(f.z), rs_key(f.w)};
        mx = rs_max4(mx, k);
    }
    mx = rs_wave_max(mx);
    if (lane == 0) part[2 * kRsWaves + wave] = mx;
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < kRsWaves; ++ww) {
        const uint32_t o = (uint32_t)part[2 * kRsWaves + ww];
        mx = mx > o ? mx : o;
    }
    const int e = rs_exponent(mx);
    const int slots = (nv + V - 1) / V;
    uint64_t carry = 0;
    int trip = 0;
    float4 f[V], fn[V];
    rs_load_slot<V>(w, tid, nv, f);
    for (int s0 = 0; s0 < slots; s0 += kRsThreads, ++trip) {
        const int slot = s0 + tid;
        rs_load_slot<V>(w, slot + kRsThreads, nv, fn);  // the next trip's, under this trip's scan
        uint64_t incl[4 * V];
        uint64_t run = 0;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float wv[4] = {f[u].x, f[u].y, f[u].z, f[u].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                run += rs_quant(rs_key(wv[c]), e);
                incl[4 * u + c] = run;
            }
        }
        uint64_t total;
        const uint64_t before = rs_wave_before(run, lane, total);
        // the waves' totals of even and odd trips in slots of their own: one barrier per trip
        uint64_t* tot = part + (trip & 1) * kRsWaves;
        if (lane == 0) tot[wave] = total;
        __syncthreads();
        uint64_t base = carry + before;
#pragma unroll
        for (int ww = 0; ww < kRsWaves; ++ww) {
            const uint64_t t = tot[ww];
            base += ww < wave ? t : 0;
            carry += t;
        }
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int v = slot * V + u;
            if (v < nv) {
#pragma unroll
                for (int c = 0; c < 4; ++c) dst[4 * (int64_t)v + c] = base + incl[4 * u + c];
            }
        }
#pragma unroll
        for (int u = 0; u < V; ++u) f[u] = fn[u];
    }
    return carry;
}

// A wave's tiles of 64 picks of point i: tiles tile0, tile0 + stride, ... below K.  cdf: the
// point's inclusive sums (LDS or global), T their last.  Every lane of the wave arrives here
// together and T is the same in all of them: the branches below are the wave's.
__device__ __forceinline__ void rs_tiles(const uint64_t* cdf, uint64_t T, int64_t i, int64_t tile0, int64_t stride,
                                         int lane, const RsArgs& a) {
    const int N = a.N, d = a.d;
    const int64_t K = a.K;
    const int steps = 32 - __clz(N - 1);  // 2^steps >= N (N >= 4)
    const uint64_t D = a.method == DF_RESAMPLE_MULTINOMIAL ? 1ull : (uint64_t)K << 32;
    uint32_t r_point = 0u;
    if (a.method == DF_RESAMPLE_SYSTEMATIC) {
        const uint64_t c = a.offset + (uint64_t)i;
        r_point = philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), 1u, 0u}, a.key0, a.key1).x;
    }
    for (int64_t k0 = tile0 * 64; k0 < K; k0 += stride * 64) {
        const int64_t k = k0 + lane;  // past K in the last tile: computed, bounded as any, not stored
        int j = -1;
        if (T != 0) {
            uint64_t xhi, xlo;  // num·T over D (multinomial: its high word over 1)
            if (a.method == DF_RESAMPLE_MULTINOMIAL) {
                const uint64_t c = a.offset + (uint64_t)i * (uint64_t)(K / 2) + (uint64_t)(k / 2);
                const U4 b = philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), 1u, 0u}, a.key0, a.key1);
                const uint64_t r = (k & 1) ? ((uint64_t)b.w << 32) | b.z : ((uint64_t)b.y << 32) | b.x;
                xhi = 0;
                xlo = __umul64hi(r, T);
            } else {
                uint32_t r = r_point;
                if (a.method == DF_RESAMPLE_STRATIFIED) {
                    const uint64_t c = a.offset + (uint64_t)i * (uint64_t)(K / 4) + (uint64_t)(k / 4);
                    const U4 b = philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), 1u, 0u}, a.key0, a.key1);
                    const int word = (int)(k & 3);
                    r = word == 0 ? b.x : word == 1 ? b.y : word == 2 ? b.z : b.w;
                }
                const uint64_t num = ((uint64_t)k << 32) | r;
                xhi = __umul64hi(num, T);
                xlo = num * T;
            }
            int pos = 0;
            for (int s = steps - 1; s >= 0; --s) {
                const int cand = pos + (1 << s);
                const int rd = (cand < N - 1 ? cand : N - 1) - 1;  // in [0, N − 2]
                const uint64_t c = cdf[rd];
                const uint64_t hi = __umul64hi(c, D), lo = c * D;
                const bool le = hi < xhi || (hi == xhi && lo <= xlo);
                pos = (cand <= N - 1 && le) ? cand : pos;
            }
            j = pos;
        }
        if (a.idx_out && k < K) a.idx_out[i * K + k] = j;
        if (a.xs_out) {
            const int R = K - k0 < 64 ? (int)(K - k0) : 64;
            float* dst = a.xs_out + (i * K + k0) * d;
            const float* src = a.xs + i * (int64_t)N * d;
            for (int t = 0; t < d; ++t) {
                const int e = t * 64 + lane, p = e / d, col = e - p * d;  // p < 64
                const int jj = __shfl(j, p, 64);
                if (p < R) dst[e] = jj < 0 ? __int_as_float(0x7fc00000) : src[(int64_t)jj * d + col];
            }
        }
    }
}

// N <= kRsWaveMax: a wave per point
__global__ void __launch_bounds__(kRsThreads) resample_wave_kernel(const float* __restrict__ w, int64_t points,
                                                                   RsArgs a) {
    __shared__ uint64_t cdf[kRsWaves][kRsWaveMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N;
    const int64_t i = (int64_t)blockIdx.x * kRsWaves + wave;
    if (i >= points) return;  // the whole wave; this kernel has no barrier
    const bool on = lane < N / 4;
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) f = *reinterpret_cast<const float4*>(w + i * N + 4 * lane);
    const uint32_t k[4] = {rs_key(f.x), rs_key(f.y), rs_key(f.z), rs_key(f.w)};
    const uint32_t mx = rs_wave_max(rs_max4(0u, k));
    const int e = rs_exponent(mx);
    const uint64_t q[4] = {rs_quant(k[0], e), rs_quant(k[1], e), rs_quant(k[2], e), rs_quant(k[3], e)};
    uint64_t T;
    uint64_t run = rs_wave_before(q[0] + q[1] + q[2] + q[3], lane, T);
    if (on) {
#pragma unroll
        for (int c = 0; c < 4; ++c) cdf[wave][4 * lane + c] = run += q[c];
    }
    rs_wave_sync();
    rs_tiles(cdf[wave], T, i, 0, 1, lane, a);
}

// kRsWaveMax < N <= kRsLdsMax: a workgroup per point
__global__ void __launch_bounds__(kRsThreads) resample_block_kernel(const float* __restrict__ w, RsArgs a) {
    __shared__ uint64_t cdf[kRsLdsMax];
    __shared__ uint64_t part[3 * kRsWaves];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const uint64_t T = rs_block_scan<1>(w + i * a.N, a.N, cdf, part, tid);
    __syncthreads();
    rs_tiles(cdf, T, i, tid >> 6, kRsWaves, tid & 63, a);
}

// N > kRsLdsMax: a workgroup per point writes the scan into ws (points · N words) ...
__global__ void __launch_bounds__(kRsThreads) resample_scan_kernel(const float* __restrict__ w, int N,
                                                                   uint64_t* __restrict__ ws) {
    __shared__ uint64_t part[3 * kRsWaves];
    const int64_t i = blockIdx.x;
    (void)rs_block_scan<kRsScanVectors>(w + i * N, N, ws + i * N, part, threadIdx.x);
}

// ... and a workgroup takes 4 tiles of 64 picks of one point: block = point · tpp + tile group
__global__ void __launch_bounds__(kRsThreads) resample_pick_kernel(const uint64_t* __restrict__ ws, int64_t tpp,
                                                                   RsArgs a) {
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x / tpp, g = (int64_t)blockIdx.x - i * tpp;
    const uint64_t* cdf = ws + i * a.N;
    const int64_t tile = g * kRsWaves + (tid >> 6);
    if (tile * 64 >= a.K) return;  // the whole wave; this kernel has no barrier
    rs_tiles(cdf, cdf[a.N - 1], i, tile, a.K, tid & 63, a);  // (stride K: this tile alone)
}

}  // namespace
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_draw_resample(const float* xs, const float* w, void* cdf_ws, int d, int64_t n_points, int64_t n_draws,
                     int64_t n_out, int method, uint64_t seed, uint64_t offset, float* xs_out, int32_t* idx_out,
                     void* stream) {
    if (method < DF_RESAMPLE_SYSTEMATIC || method > DF_RESAMPLE_MULTINOMIAL)
        return set_err(DF_ERR_INVALID, "method must be 0 (systematic), 1 (stratified) or 2 (multinomial)");
    // n_points and n_draws: the rules and messages of df_importance_weights
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0)
        return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kRsDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    if (n_out <= 0 || n_out % 4 != 0) return set_err(DF_ERR_INVALID, "n_out must be a positive multiple of 4");
    if (n_out > kRsOutMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 picks (n_out)");
    if (!w) return set_err(DF_ERR_INVALID, "null w array");
    if (reinterpret_cast<uintptr_t>(w) % 16 != 0) return set_err(DF_ERR_INVALID, "w must be 16-byte aligned");
    if (!xs_out && !idx_out) return set_err(DF_ERR_INVALID, "no output: xs_out and idx_out are both null");
    if (xs_out) {
        if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
        if (!xs) return set_err(DF_ERR_INVALID, "null xs array");
        if (reinterpret_cast<uintptr_t>(xs) % 16 != 0) return set_err(DF_ERR_INVALID, "xs must be 16-byte aligned");
    }
    const bool streamed = n_draws > kRsLdsMax;
    if (streamed && (!cdf_ws || reinterpret_cast<uintptr_t>(cdf_ws) % 8 != 0))
        return set_err(DF_ERR_INVALID, "n_draws above DF_RESAMPLE_LDS_DRAWS needs cdf_ws: n_points · n_draws "
                                       "8-byte aligned uint64 words");
    // the draws' and the picked rows' floats, the workspace's words
    const int64_t row = xs_out ? d : 1;
    const int64_t per_point = (n_draws > n_out ? n_draws : n_out) * (row > 2 ? row : 2);
    if (n_points > (INT64_MAX / 4) / per_point) return set_err(DF_ERR_SHAPE, "n_points · n_draws · d past int64");
    if (n_points == 0) return DF_OK;

    const int N = (int)n_draws;
    RsArgs a{xs_out ? xs : nullptr, xs_out ? d : 1, N, n_out, method, (uint32_t)seed, (uint32_t)(seed >> 32), offset,
             xs_out, idx_out};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t tpp = (n_out + 64 * kRsWaves - 1) / (64 * kRsWaves);  // tile groups of a point
    const int64_t blocks = N <= kRsWaveMax ? (n_points + kRsWaves - 1) / kRsWaves : n_points;
    if (blocks > 0x7fffffff || (streamed && n_points > 0x7fffffff / tpp))
        return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    if (N <= kRsWaveMax) {
        hipLaunchKernelGGL(resample_wave_kernel, dim3((unsigned)blocks), dim3(kRsThreads), 0, st, w, n_points, a);
    } else if (!streamed) {
        hipLaunchKernelGGL(resample_block_kernel, dim3((unsigned)blocks), dim3(kRsThreads), 0, st, w, a);
    } else {
        uint64_t* ws = static_cast<uint64_t*>(cdf_ws);
        hipLaunchKernelGGL(resample_scan_kernel, dim3((unsigned)blocks), dim3(kRsThreads), 0, st, w, N, ws);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_err(e, "resampling scan kernel launch");
        hipLaunchKernelGGL(resample_pick_kernel, dim3((unsigned)(n_points * tpp)), dim3(kRsThreads), 0, st, ws, tpp, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DF_OK : hip_err(e, "resampling kernel launch");
}

}  // extern "C"
