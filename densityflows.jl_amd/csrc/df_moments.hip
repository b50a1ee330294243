// df_moments.hip — expectations under the flow, reduced on the device:
//   df_flow_sample_logpdf          x ~ q together with log q(x), one forward pass per sample
//   df_flow_sample_logpdf_moments  {count, Σ lp, Σ lp²} of such draws, chunk by chunk (entropy)
//   df_train_score_moments         {count, Σ lp, Σ lp², Σ g, Σ g gᵀ} of df_train_logpdf_grad's
//                                  per-sample lp and g = ∂lp/∂θ on given points
//   df_train_fisher                the same sums over draws at one θ (the Fisher matrix)
// Nothing of the workload's size crosses to the host: a call returns 3 + m + m² doubles.
//
// The reduction is store-and-sum, without atomics: moments_partial_kernel writes one block of
// 3 + m + m² doubles per workgroup, moments_final_kernel adds the blocks in workgroup order.
// With T = kMomThreads, tiles = ceil(batch / T), trips = ceil(tiles / min(grid, tiles)),
// per = trips · T and G = ceil(tiles / trips) workgroups, workgroup b owns the samples
// [b·per, (b+1)·per) ∩ [0, batch) and walks them in trips of T: thread i adds sample b·per + trip·T + i to its own sums, trips in
// increasing order; a sample past the range adds nothing.  Then the fixed tree: lanes of a
// wave by __shfl_down with offsets 32, 16, 8, 4, 2, 1 (lane l takes l + offset), and the
// waves' sums ((w0 + w1) + w2) + w3.  Every term is a product or a sum in double of the
// floats converted to double.  The outer products are walked in 8 × 8 tiles (ta <= tb): the
// 64 sums of a tile pair live in registers, m <= 8 reads every sample once, a larger m reads
// the samples once per tile pair.  Entry (a, b) and entry (b, a) are the same sequence of
// double operations on commuted factors, so both triangles hold the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "densityflows_hip.h"
#include "df_trainer.h"

namespace df {
namespace {

constexpr int kMomThreads = 256;  // samples of one trip of a workgroup; 4 waves
constexpr int kMomWgPerCu = 2;    // workgroups per CU of grid_cus the grid is sized from (both resident)
constexpr int kMomTile = 8;       // rows (and columns) of one register tile of Σ g gᵀ
constexpr int kMomAcc = kMomTile * kMomTile + kMomTile + 2;
constexpr int64_t kChunkDefault = (int64_t)1 << 20, kChunkMax = (int64_t)1 << 24;

// The base term of df_flow_sample_logpdf, one thread per sample, every operation one Float32
// operation (the unit is built without contraction):
//   s = z_0·z_0;  s = s + z_k·z_k for k = 1 .. d-1;  lp = -(c + s) / 2,  c = (float)d · (float)log(2π)
__global__ void __launch_bounds__(256) base_logpdf_kernel(const float* __restrict__ z, float* __restrict__ lp,
                                                          int d, int64_t batch, float c) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= batch) return;
    const float* zj = z + (int64_t)d * j;
    float s = zj[0] * zj[0];
    for (int k = 1; k < d; ++k) s = s + zj[k] * zj[k];
    lp[j] = -(c + s) / 2.f;
}

// lp_j = lp_j - ldj_j: the density of a drawn point from the base term and the forward ldj
__global__ void __launch_bounds__(256) sub_ldj_kernel(float* __restrict__ lp, const float* __restrict__ ldj,
                                                      int64_t batch) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < batch) lp[j] = lp[j] - ldj[j];
}

// One workgroup's block of partial sums (layout of the output block; entry 0 is left to the
// final kernel).  part: [gridDim.x][3 + m + m²].
__global__ void __launch_bounds__(kMomThreads) moments_partial_kernel(const float* __restrict__ lp,
                                                                      const float* __restrict__ g, int m,
                                                                      int64_t batch, int64_t per,
                                                                      double* __restrict__ part) {
    __shared__ double red[kMomThreads / 64][kMomAcc];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t E = 3 + (int64_t)m + (int64_t)m * m;
    double* const mine = part + (int64_t)blockIdx.x * E;
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < batch ? lo + per : batch;
    const int T = (m + kMomTile - 1) / kMomTile;
    // tile pairs (ta, tb), ta <= tb; m == 0 still takes one pass for the lp sums
    for (int ta = 0; ta < (T > 0 ? T : 1); ++ta) {
        for (int tb = ta; tb < (T > 0 ? T : 1); ++tb) {
            const bool diag = ta == tb, first = ta == 0 && tb == 0;
            // rows and columns of this tile pair that exist (uniform: the unrolled loops keep
            // their static register indices and skip the rest)
            const int na = m - ta * kMomTile < kMomTile ? m - ta * kMomTile : kMomTile;
            const int nb = m - tb * kMomTile < kMomTile ? m - tb * kMomTile : kMomTile;
            double acc[kMomAcc];
#pragma unroll
            for (int k = 0; k < kMomAcc; ++k) acc[k] = 0.0;
            for (int64_t j = lo + tid; j < hi; j += kMomThreads) {
                double ga[kMomTile], gb[kMomTile];
#pragma unroll
                for (int k = 0; k < kMomTile; ++k) {
                    const int a = ta * kMomTile + k, b = tb * kMomTile + k;
                    ga[k] = a < m ? (double)g[(int64_t)m * j + a] : 0.0;
                    gb[k] = b < m ? (double)g[(int64_t)m * j + b] : 0.0;
                }
#pragma unroll
                for (int kb = 0; kb < kMomTile; ++kb) {
                    if (kb >= nb) continue;
#pragma unroll
                    for (int ka = 0; ka < kMomTile; ++ka)
                        if (ka < na) acc[ka + kMomTile * kb] = acc[ka + kMomTile * kb] + ga[ka] * gb[kb];
                }
                if (diag) {
#pragma unroll
                    for (int k = 0; k < kMomTile; ++k)
                        if (k < na) acc[kMomTile * kMomTile + k] = acc[kMomTile * kMomTile + k] + ga[k];
                }
                if (first) {
                    const double v = (double)lp[j];
                    acc[kMomAcc - 2] = acc[kMomAcc - 2] + v;
                    acc[kMomAcc - 1] = acc[kMomAcc - 1] + v * v;
                }
            }
            // the fixed tree: lanes, then waves in order
#pragma unroll
            for (int k = 0; k < kMomAcc; ++k) {
                // (sums nothing was added to are not stored below either)
                const bool used = k < kMomTile * kMomTile ? (k % kMomTile < na && k / kMomTile < nb)
                                  : k < kMomAcc - 2       ? (diag && k - kMomTile * kMomTile < na)
                                                          : first;
                if (!used) continue;
                double v = acc[k];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
                if (lane == 0) red[wave][k] = v;
            }
            __syncthreads();
            if (tid < kMomAcc) {
                double v = red[0][tid];
                for (int w = 1; w < kMomThreads / 64; ++w) v = v + red[w][tid];
                if (tid < kMomTile * kMomTile) {
                    const int a = ta * kMomTile + (tid % kMomTile), b = tb * kMomTile + (tid / kMomTile);
                    if (a < m && b < m) {
                        mine[3 + m + a + (int64_t)m * b] = v;
                        if (!diag) mine[3 + m + b + (int64_t)m * a] = v;
                    }
                } else if (tid < kMomTile * kMomTile + kMomTile) {
                    const int a = ta * kMomTile + (tid - kMomTile * kMomTile);
                    if (diag && a < m) mine[3 + a] = v;
                } else if (first) {
                    mine[1 + (tid - (kMomAcc - 2))] = v;
                }
            }
            __syncthreads();
        }
    }
}

// out[e] = (accumulate ? out[e] : 0) + Σ_b part[b][e], b in increasing order; out[0] counts.
// One workgroup per entry: its threads fetch the partials kMomFinal at a time into LDS, then
// thread 0 adds them in workgroup order (the order is the contract; the loads are what costs).
constexpr int kMomFinal = 1024;
__global__ void __launch_bounds__(256) moments_final_kernel(const double* __restrict__ part, int nblocks, int64_t E,
                                                            int64_t batch, int accumulate, double* __restrict__ out) {
    __shared__ double buf[kMomFinal];
    const int64_t e = blockIdx.x;
    double s = 0.0;
    for (int base = 0; base < nblocks; base += kMomFinal) {
        const int cnt = nblocks - base < kMomFinal ? nblocks - base : kMomFinal;
        for (int i = threadIdx.x; i < cnt; i += 256) buf[i] = part[(int64_t)(base + i) * E + e];
        __syncthreads();
        if (threadIdx.x == 0) {
            int i = 0;
            if (base == 0) s = buf[i++];
#pragma unroll 8
            for (; i < cnt; ++i) s = s + buf[i];  // (unrolled: the LDS reads run ahead of the add chain)
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (e == 0) s = (double)batch;
        out[e] = accumulate ? out[e] + s : s;
    }
}

inline unsigned blocks256(int64_t count) { return (unsigned)((count + 255) / 256); }

int64_t moments_entries(int m) { return 3 + (int64_t)m + (int64_t)m * m; }

// Workgroups of the partial kernel for this batch.
int moments_grid(const df_chain* c, int64_t batch) {
    const int64_t tiles = (batch + kMomThreads - 1) / kMomThreads;
    return (int)std::min<int64_t>((int64_t)std::max(1, c->grid_cus) * kMomWgPerCu, tiles);
}

}  // namespace

namespace api {

bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    return cap != hipStreamCaptureStatusNone;
}

// A handle's workspace holds `need` bytes after this.  It only grows, and not inside a capture;
// it belongs to the handle, not to a stream: an earlier call on any stream may still read it.
int reserve(DevBuf& buf, int64_t& cap, int64_t need, hipStream_t st, const char* what) {
    if (need <= cap) return DF_OK;
    if (capturing(st))
        return api::set_err(DF_ERR_INVALID, std::string("the ") + what + " workspace cannot grow during a stream capture");
    if (buf.get()) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return api::hip_err(e, "hipDeviceSynchronize");
    }
    cap = 0;
    if (buf.alloc((size_t)need) != hipSuccess)
        return api::set_err(DF_ERR_NOMEM, std::string("hipMalloc failed (") + what + " workspace)");
    cap = need;
    return DF_OK;
}

int launch_base_logpdf(const float* z, float* lp, int d, int64_t batch, hipStream_t st) {
    hipLaunchKernelGGL(base_logpdf_kernel, dim3(blocks256(batch)), dim3(256), 0, st, z, lp, d, batch,
                       (float)d * (float)kLog2Pi);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DF_OK : hip_err(e, "base logpdf kernel launch");
}

}  // namespace api

namespace {

// The reduction of (lp, g) over `batch` > 0 samples into out (3 + m + m² doubles), through
// the caller's partial buffer (reserved for this batch).
int reduce_moments(const df_chain* c, const float* lp, const float* g, int m, int64_t batch, double* part,
                   double* out, int accumulate, hipStream_t st) {
    const int64_t tiles = (batch + kMomThreads - 1) / kMomThreads;
    const int64_t trips = (tiles + moments_grid(c, batch) - 1) / moments_grid(c, batch);
    const int64_t per = trips * kMomThreads;
    const int G = (int)((tiles + trips - 1) / trips);  // no workgroup without a sample
    const int64_t E = moments_entries(m);
    hipLaunchKernelGGL(moments_partial_kernel, dim3((unsigned)G), dim3(kMomThreads), 0, st, lp, g, m, batch, per, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api::hip_err(e, "moments kernel launch");
    hipLaunchKernelGGL(moments_final_kernel, dim3((unsigned)E), dim3(256), 0, st, part, G, E, batch, accumulate, out);
    e = hipGetLastError();
    return e == hipSuccess ? DF_OK : api::hip_err(e, "moments sum kernel launch");
}

int64_t part_bytes(const df_chain* c, int m, int64_t batch) {
    return (int64_t)sizeof(double) * moments_grid(c, batch) * moments_entries(m);
}

// The chunk a call proceeds by: 0 is 2^20, rounded up to a multiple of 4 (a Philox counter
// boundary).  The caller has refused chunk < 0 and chunk > 2^24.
int64_t chunk_of(int64_t chunk) { return chunk == 0 ? kChunkDefault : (chunk + 3) / 4 * 4; }

int check_chunked(int64_t n_samples, int64_t chunk) {
    if (n_samples < 0) return api::set_err(DF_ERR_SHAPE, "negative sample count");
    if (chunk < 0) return api::set_err(DF_ERR_SHAPE, "negative chunk size");
    if (chunk > kChunkMax) return api::set_err(DF_ERR_UNSUPPORTED, "a chunk holds at most 2^24 samples");
    return DF_OK;
}

}  // namespace
}  // namespace df

using namespace df;
using namespace df::api;

// df_flow_sample_logpdf on a chain whose arguments df_flow_sample's checks have passed.
static int sample_logpdf(df_chain* c, float* x_out, float* logpdf_out, const float* theta_raw, int theta_broadcast,
                         int64_t batch, uint64_t seed, uint64_t offset, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (logpdf_out) {
        const int rc = reserve(c->d_slp_ldj, c->slp_ldj_cap, (int64_t)sizeof(float) * std::max<int64_t>(batch, 1024),
                               st, "sample density");
        if (rc != DF_OK) return rc;
    }
    const float* th = nullptr;
    int rc = sample_draw(c, x_out, theta_raw, theta_broadcast, batch, seed, offset, stream, &th);
    if (rc != DF_OK) return rc;
    if (!logpdf_out) return df_flow_forward(c, x_out, th, x_out, nullptr, batch, stream);
    if ((rc = launch_base_logpdf(x_out, logpdf_out, c->plan.d, batch, st)) != DF_OK) return rc;
    float* ldj = c->d_slp_ldj.as<float>();
    rc = df_flow_forward(c, x_out, th, x_out, ldj, batch, stream);
    if (rc != DF_OK) return rc;
    hipLaunchKernelGGL(sub_ldj_kernel, dim3(blocks256(batch)), dim3(256), 0, st, logpdf_out, ldj, batch);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DF_OK : hip_err(e, "density combine kernel launch");
}

extern "C" {

int df_flow_sample_logpdf(df_chain* c, float* x_out, float* logpdf_out, const float* theta_raw, int theta_broadcast,
                          int64_t batch, uint64_t seed, uint64_t offset, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (batch == 0) return DF_OK;
    if (!x_out) return set_err(DF_ERR_INVALID, "null output array");
    if ((batch + 255) / 256 > 0x7fffffff) return set_err(DF_ERR_UNSUPPORTED, "batch too large for one launch");
    const int rc = sample_check_theta(c, theta_raw);
    if (rc != DF_OK) return rc;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    return sample_logpdf(c, x_out, logpdf_out, theta_raw, theta_broadcast, batch, seed, offset, stream);
}

int df_flow_sample_logpdf_moments(df_chain* c, const float* theta_raw, int64_t n_samples, int64_t chunk,
                                  uint64_t seed, uint64_t offset, double* out3, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    int rc = check_chunked(n_samples, chunk);
    if (rc != DF_OK) return rc;
    if (!out3) return set_err(DF_ERR_INVALID, "null output block");
    const int d = c->plan.d;
    if (n_samples > 0 && (rc = sample_check_theta(c, theta_raw)) != DF_OK) return rc;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(out3, 0, 3 * sizeof(double), st);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    if (n_samples == 0) return DF_OK;
    const int64_t step = std::min(chunk_of(chunk), (n_samples + 3) / 4 * 4);
    if ((rc = reserve(c->d_mom_x, c->mom_x_cap, (int64_t)sizeof(float) * d * step, st, "moments sample")) != DF_OK ||
        (rc = reserve(c->d_mom_lp, c->mom_lp_cap, (int64_t)sizeof(float) * step, st, "moments density")) != DF_OK ||
        (rc = reserve(c->d_mom_part, c->mom_part_cap, part_bytes(c, 0, step), st, "moments partial")) != DF_OK)
        return rc;
    float* x = c->d_mom_x.as<float>();
    float* lp = c->d_mom_lp.as<float>();
    for (int64_t start = 0; start < n_samples; start += step) {
        const int64_t len = std::min(step, n_samples - start);
        rc = sample_logpdf(c, x, lp, theta_raw, 1, len, seed, offset + (uint64_t)((int64_t)d * (start / 4)), stream);
        if (rc != DF_OK) return rc;
        rc = reduce_moments(c, lp, nullptr, 0, len, c->d_mom_part.as<double>(), out3, 1, st);
        if (rc != DF_OK) return rc;
    }
    return DF_OK;
}

}  // extern "C"

static int unsupported_layerwise(const char* who) {
    return set_err(DF_ERR_UNSUPPORTED,
                   std::string(who) +
                       ": df_train_logpdf_grad needs a trainer on the fused sweep; this chain trains layer-wise "
                       "(a conditioner with hidden width > 64, more than one hidden Dense, or more than 4 "
                       "transformed dims in a layer)");
}

// The trainer's lp, gθ and partial workspaces for `batch` samples, and the sweep's own buffers
// (ensure_capacity inside score_sweep replaces them: not inside a capture either).
static int reserve_score(df_train* t, int64_t batch, hipStream_t st) {
    const df_chain* c = t->c;
    const int n = c->plan.n;
    if (n > 0 && batch > t->cap && capturing(st))
        return set_err(DF_ERR_INVALID, "the sweep's workspaces cannot grow during a stream capture");
    const int64_t cap = std::max<int64_t>(batch, 1024);
    int rc;
    if ((rc = reserve(t->d_mom_lp, t->mom_lp_cap, (int64_t)sizeof(float) * cap, st, "moments density")) != DF_OK ||
        (rc = reserve(t->d_mom_g, t->mom_g_cap, (int64_t)sizeof(float) * std::max(n, 1) * cap, st,
                      "moments score")) != DF_OK ||
        (rc = reserve(t->d_mom_part, t->mom_part_cap, part_bytes(c, n, cap), st, "moments partial")) != DF_OK)
        return rc;
    return DF_OK;
}

// lp and gθ of (x, θ) into the trainer's workspaces, then the reduction.  flow: -1 as the
// trainer's df_theta_input says, 1 raw θ.
static int score_moments(df_train* t, const float* x, const float* theta, int64_t batch, double* out, int accumulate,
                         int flow, hipStream_t st) {
    const int n = t->c->plan.n;
    int rc = reserve_score(t, batch, st);
    if (rc != DF_OK) return rc;
    float* lp = t->d_mom_lp.as<float>();
    float* g = n > 0 ? t->d_mom_g.as<float>() : nullptr;
    rc = score_sweep(t, x, theta, lp, nullptr, g, batch, flow, st);
    if (rc != DF_OK) return rc;
    return reduce_moments(t->c, lp, g, n, batch, t->d_mom_part.as<double>(), out, accumulate, st);
}

extern "C" {

int df_train_score_moments(df_train* t, const float* x, const float* theta, int64_t batch, double* out,
                           int accumulate, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (t->tp.layerwise) return unsupported_layerwise("df_train_score_moments");
    if (!out) return set_err(DF_ERR_INVALID, "null output block");
    df_chain* c = t->c;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        if (accumulate) return DF_OK;
        const hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * moments_entries(c->plan.n), st);
        return e == hipSuccess ? DF_OK : hip_err(e, "hipMemsetAsync");
    }
    if (!x) return set_err(DF_ERR_INVALID, "null input array");
    if (c->plan.n > 0 && !theta)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    return score_moments(t, x, theta, batch, out, accumulate != 0, -1, st);
}

int df_train_fisher(df_train* t, const float* theta_raw, int64_t n_samples, int64_t chunk, uint64_t seed,
                    uint64_t offset, double* out, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    int rc = check_chunked(n_samples, chunk);
    if (rc != DF_OK) return rc;
    if (t->tp.layerwise) return unsupported_layerwise("df_train_fisher");
    if (!out) return set_err(DF_ERR_INVALID, "null output block");
    df_chain* c = t->c;
    const int d = c->plan.d, n = c->plan.n;
    if (n_samples > 0 && (rc = sample_check_theta(c, theta_raw)) != DF_OK) return rc;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * moments_entries(n), st);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    if (n_samples == 0) return DF_OK;
    const int64_t step = std::min(chunk_of(chunk), (n_samples + 3) / 4 * 4);
    if ((rc = reserve(t->d_mom_x, t->mom_x_cap, (int64_t)sizeof(float) * d * step, st, "moments sample")) != DF_OK ||
        (rc = reserve(t->d_mom_th, t->mom_th_cap, (int64_t)sizeof(float) * std::max(n, 1) * step, st,
                      "moments θ")) != DF_OK ||
        (rc = reserve_score(t, step, st)) != DF_OK)
        return rc;
    float* x = t->d_mom_x.as<float>();
    float* th = n > 0 ? t->d_mom_th.as<float>() : nullptr;
    // one θ for every sample: the broadcast serves every chunk
    if (n > 0 && (rc = df_theta_broadcast(th, theta_raw, n, std::min(step, n_samples), stream)) != DF_OK) return rc;
    for (int64_t start = 0; start < n_samples; start += step) {
        const int64_t len = std::min(step, n_samples - start);
        rc = df_flow_sample(c, x, th, 0, len, seed, offset + (uint64_t)((int64_t)d * (start / 4)), stream);
        if (rc != DF_OK) return rc;
        rc = score_moments(t, x, th, len, out, 1, 1, st);
        if (rc != DF_OK) return rc;
    }
    return DF_OK;
}

}  // extern "C"
