// df_calib.hip — calibration of the conditional density, reduced on the device:
//   df_flow_hpd_ranks   for every point (x_i, θ_i) the number of n_draws samples of q(. | θ_i)
//                       whose density exceeds the point's (the HPD rank of the expected-coverage
//                       test); one int32 per point leaves the call, not n_points · n_draws floats
//
// Per chunk of whole points: the Philox draw (df_sample.hip), θ row i repeated over the draws of
// point i (theta_repeat_kernel), the base term (base_logpdf_kernel of df_moments.hip),
// df_flow_forward in place with the ldj into a workspace, and hpd_count_kernel in the place of
// sub_ldj_kernel: lp = base − ldj (the same single Float32 subtraction), compared with the
// point's lp, counted.
//
// The count is a ballot and a population count per wave64 — no atomics, no zeroing pass, one
// store per point.  With L = n_draws / 4 (a lane holds 4 consecutive draws, 16-byte loads) the
// mapping of points follows from L:
//   L <= 32   packed: 64 / L points per wave, point s in lanes [s·L, (s+1)·L); a point's count
//             is the ballot under its segment's mask.  Small n_draws would otherwise leave
//             most of a wave idle (n_draws = 4: one lane of 64).
//   L <= 128  a wave per point, trips of 64 lanes; 4 points per workgroup, no barrier
//   above     a workgroup per point, trips of 256 lanes; the 4 waves' counts through LDS,
//             added in wave order by thread 0
// Counts are integers: every mapping and every order gives the same rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kHpdThreads = 256;  // 4 waves
constexpr int kHpdWaves = kHpdThreads / 64;
constexpr int kHpdPackedMax = 32;      // L up to which several points share a wave
constexpr int kHpdWaveMax = 128;       // L up to which a point is one wave's (two trips)
constexpr int64_t kChunkDefault = (int64_t)1 << 20, kChunkMax = (int64_t)1 << 24;
constexpr int64_t kDrawsMax = (int64_t)1 << 24;

enum HpdMap { kMapPacked = 0, kMapWave = 1, kMapBlock = 2 };

// dst (n, points · n_draws): column i·n_draws + k is column i of th (n, points)
__global__ void __launch_bounds__(256) theta_repeat_kernel(float* __restrict__ dst, const float* __restrict__ th, int n,
                                                           int64_t n_draws, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t j = e / n;
    dst[e] = th[(j / n_draws) * n + (e - j * n)];
}

// The 4 draws of float4 slot q: lp = base − ldj, stored when asked, compared with the point's
// lp.  Bit e of the result: draw e lies above the point (IEEE: false when either is NaN).
template <bool STORE>
__device__ __forceinline__ unsigned above4(const float* __restrict__ base, const float* __restrict__ ldj,
                                           float* __restrict__ lp_out, bool vec, int64_t q, float v) {
    const float4 b = *reinterpret_cast<const float4*>(base + 4 * q);
    const float4 l = *reinterpret_cast<const float4*>(ldj + 4 * q);
    const float4 lp = float4{b.x - l.x, b.y - l.y, b.z - l.z, b.w - l.w};
    if (STORE) {
        if (vec) {
            *reinterpret_cast<float4*>(lp_out + 4 * q) = lp;
        } else {
            lp_out[4 * q] = lp.x;
            lp_out[4 * q + 1] = lp.y;
            lp_out[4 * q + 2] = lp.z;
            lp_out[4 * q + 3] = lp.w;
        }
    }
    return (lp.x > v ? 1u : 0u) | (lp.y > v ? 2u : 0u) | (lp.z > v ? 4u : 0u) | (lp.w > v ? 8u : 0u);
}

// The lanes of `mask` whose draws lie above, over the 4 draws of a lane.
__device__ __forceinline__ int count4(unsigned above, unsigned long long mask) {
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) cnt += __popcll(__ballot((above >> e) & 1u) & mask);
    return cnt;
}

// rank[i] = #{k : base[i·N + k] − ldj[i·N + k] > lp_pts[i]} for the `points` points of a chunk,
// N = 4·L.  base, ldj (and lp_out unless it is odd-aligned, `vec` = 0) are 16-byte aligned.
template <bool STORE, int MAP>
__global__ void __launch_bounds__(kHpdThreads) hpd_count_kernel(const float* __restrict__ base,
                                                                const float* __restrict__ ldj,
                                                                const float* __restrict__ lp_pts, int L, int64_t points,
                                                                int32_t* __restrict__ rank, float* __restrict__ lp_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool vec = STORE && (reinterpret_cast<uintptr_t>(lp_out) & 15) == 0;
    if (MAP == kMapPacked) {
        const int per = 64 / L;  // points of a wave
        const int seg = lane / L, within = lane - seg * L;
        const int64_t i = ((int64_t)blockIdx.x * kHpdWaves + wave) * per + seg;
        const bool on = seg < per && i < points;
        unsigned above = 0;
        if (on) above = above4<STORE>(base, ldj, lp_out, vec, i * L + within, lp_pts[i]);
        const unsigned long long mask = ((1ull << L) - 1ull) << (seg < per ? seg * L : 0);
        const int cnt = count4(above, mask);
        if (on && within == 0) rank[i] = cnt;
    } else if (MAP == kMapWave) {
        const int64_t i = (int64_t)blockIdx.x * kHpdWaves + wave;
        if (i >= points) return;  // the whole wave; nothing below waits for it
        const float v = lp_pts[i];
        int cnt = 0;
        for (int t = 0; t < L; t += 64) {
            unsigned above = 0;
            if (t + lane < L) above = above4<STORE>(base, ldj, lp_out, vec, i * L + t + lane, v);
            cnt += count4(above, ~0ull);
        }
        if (lane == 0) rank[i] = cnt;
    } else {
        __shared__ int red[kHpdWaves];
        const int64_t i = blockIdx.x;
        const float v = lp_pts[i];
        int cnt = 0;
        for (int t = 0; t < L; t += kHpdThreads) {
            unsigned above = 0;
            if (t + tid < L) above = above4<STORE>(base, ldj, lp_out, vec, i * L + t + tid, v);
            cnt += count4(above, ~0ull);
        }
        if (lane == 0) red[wave] = cnt;
        __syncthreads();
        if (tid == 0) rank[i] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

template <bool STORE>
void launch_count(const float* base, const float* ldj, const float* lp_pts, int L, int64_t points, int32_t* rank,
                  float* lp_out, hipStream_t st) {
    if (L <= kHpdPackedMax) {
        const int64_t per_wg = (int64_t)kHpdWaves * (64 / L);
        hipLaunchKernelGGL((hpd_count_kernel<STORE, kMapPacked>), dim3((unsigned)((points + per_wg - 1) / per_wg)),
                           dim3(kHpdThreads), 0, st, base, ldj, lp_pts, L, points, rank, lp_out);
    } else if (L <= kHpdWaveMax) {
        hipLaunchKernelGGL((hpd_count_kernel<STORE, kMapWave>), dim3((unsigned)((points + kHpdWaves - 1) / kHpdWaves)),
                           dim3(kHpdThreads), 0, st, base, ldj, lp_pts, L, points, rank, lp_out);
    } else {
        hipLaunchKernelGGL((hpd_count_kernel<STORE, kMapBlock>), dim3((unsigned)points), dim3(kHpdThreads), 0, st, base,
                           ldj, lp_pts, L, points, rank, lp_out);
    }
}

}  // namespace

namespace api {

int launch_theta_repeat(float* dst, const float* th, int n, int64_t n_draws, int64_t total, hipStream_t st) {
    if ((total + 255) / 256 > 0x7fffffff) return set_err(DF_ERR_UNSUPPORTED, "chunk too large for one launch");
    hipLaunchKernelGGL(theta_repeat_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dst, th, n, n_draws,
                       total);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DF_OK : hip_err(e, "θ repeat kernel launch");
}

}  // namespace api
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_flow_hpd_ranks(df_chain* c, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                      int64_t chunk, uint64_t seed, uint64_t offset, int32_t* rank_out, float* logpdf_out,
                      float* draws_logpdf_out, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (chunk < 0) return set_err(DF_ERR_SHAPE, "negative chunk size");
    if (n_draws <= 0 || n_draws % 4 != 0)
        return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4 (a Philox counter boundary)");
    if (chunk > kChunkMax) return set_err(DF_ERR_UNSUPPORTED, "a chunk holds at most 2^24 samples");
    if (n_draws > kDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    if (!rank_out) return set_err(DF_ERR_INVALID, "null rank output");
    if (n_points == 0) return DF_OK;
    if (!x) return set_err(DF_ERR_INVALID, "null input array");
    // (the first use of the handle)
    int rc = sample_check_theta(c, theta_raw);
    if (rc != DF_OK) return rc;
    const int d = c->plan.d, n = c->plan.n;
    if (n_points > (INT64_MAX / 4) / n_draws / std::max(d, std::max(n, 1)))
        return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);

    // whole points per chunk
    const int64_t G = std::min(n_points, std::max<int64_t>(1, (chunk == 0 ? kChunkDefault : chunk) / n_draws));
    const int64_t step = G * n_draws;  // samples; <= 2^24
    if ((rc = reserve(c->d_mom_x, c->mom_x_cap, (int64_t)sizeof(float) * d * step, st, "calibration sample")) != DF_OK ||
        (rc = reserve(c->d_mom_lp, c->mom_lp_cap, (int64_t)sizeof(float) * step, st, "calibration base term")) != DF_OK ||
        (rc = reserve(c->d_slp_ldj, c->slp_ldj_cap, (int64_t)sizeof(float) * std::max<int64_t>(step, 1024), st,
                      "calibration ldj")) != DF_OK ||
        (n > 0 && (rc = reserve(c->d_hpd_th, c->hpd_th_cap, (int64_t)sizeof(float) * n * step, st,
                                "calibration θ")) != DF_OK) ||
        (!logpdf_out && (rc = reserve(c->d_hpd_lp, c->hpd_lp_cap,
                                      (int64_t)sizeof(float) * std::max<int64_t>(n_points, 1024), st,
                                      "calibration point density")) != DF_OK))
        return rc;
    float* xs = c->d_mom_x.as<float>();
    float* base = c->d_mom_lp.as<float>();
    float* ldj = c->d_slp_ldj.as<float>();
    float* th = n > 0 ? c->d_hpd_th.as<float>() : nullptr;
    float* lp_pts = logpdf_out ? logpdf_out : c->d_hpd_lp.as<float>();

    // the points' own density: one inverse pass over all of them
    if ((rc = df_flow_logpdf(c, x, theta_raw, lp_pts, n_points, stream)) != DF_OK) return rc;

    const int L = (int)(n_draws / 4);
    for (int64_t p0 = 0; p0 < n_points; p0 += G) {
        const int64_t pts = std::min(G, n_points - p0);
        const int64_t len = pts * n_draws;
        const float* unused = nullptr;
        rc = sample_draw(c, xs, nullptr, 0, len, seed, offset + (uint64_t)((int64_t)d * p0 * L), stream, &unused);
        if (rc != DF_OK) return rc;
        hipError_t e;
        if (n > 0 && (rc = launch_theta_repeat(th, theta_raw + (int64_t)n * p0, n, n_draws, (int64_t)n * len, st)) != DF_OK)
            return rc;
        if ((rc = launch_base_logpdf(xs, base, d, len, st)) != DF_OK) return rc;
        if ((rc = df_flow_forward(c, xs, th, xs, ldj, len, stream)) != DF_OK) return rc;
        if (draws_logpdf_out)
            launch_count<true>(base, ldj, lp_pts + p0, L, pts, rank_out + p0, draws_logpdf_out + p0 * n_draws, st);
        else
            launch_count<false>(base, ldj, lp_pts + p0, L, pts, rank_out + p0, nullptr, st);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "count kernel launch");
    }
    return DF_OK;
}

}  // extern "C"
