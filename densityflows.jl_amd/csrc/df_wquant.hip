// df_wquant.hip — the fixed-point scale and the weighted quantiles of per-point draws under
// importance weights, on the device:
//   df_draw_weight_scale         per point {e, T}: the exponent of its largest weight that takes
//                                part and the sum of its quantised weights (df_wscale.h)
//   df_draw_weighted_quantiles   the requested weighted quantiles of every dimension of every
//                                point of a caller-owned (d, n_points · n_draws) array of draws
// Everything past the quantisation is integer arithmetic: with q_j the quantised weight of draw
// j, key_j its totalOrder key (df_quant.hip) in a dimension, C(k) = Σ {q_j : key_j <= k} and
// τ = max(1, ceil(num·T / 2^32)), the result is the draw with the smallest key k such that
// C(k) >= τ, returned with its own bits.  A point with T = 0 gives 0x7fc00000 in every slot.
//
// weight_scale_kernel: a wave per point up to N = 256 (lane l holds weights 4l .. 4l + 3, one
// 16-byte load; 4 points per workgroup, no workgroup barrier), a workgroup per point above (two
// walks of the point's weights in 16-byte loads: the largest key, then Σ q).  Two 8-byte stores
// per point.
//
// wquant_select_kernel: order_select_kernel's radix select (df_quant.hip) — 8-bit digits, most
// significant first, 4 passes over the point's d · N contiguous floats — with uint64 sums of
// quantised weights in place of counts.  A pair is a (dimension, probability).  Pass 0 sums the
// top digit once per dimension; passes 1-3 sum, per pair, the next digit of the draws whose
// higher digits equal the pair's prefix.  A draw's q is quantised on the fly from w[i·N + row]
// and the point's e (scale_out); a draw with q = 0 adds nothing.  Summing is a 64-bit LDS add
// on a 256-bin histogram (integer sums: any order gives the same words).  Each pair has a
// residual rem, initially its τ, computed here from T (scale_out) and the numerators.  After a
// pass a wave scans the pair's histogram — lane l holds bins 4l .. 4l + 3, an inclusive scan over
// the lanes — finds the one bin b with below(b) < rem <= below(b) + sum(b), appends b to the
// prefix and subtracts below(b) from rem.  1 <= rem <= (weight under the prefix) holds
// throughout, so exactly one bin answers and its sum is positive.  After pass 3 the prefix is the
// key.
//
// Teams follow N as in order_select_kernel: a wave per point up to N = 256, a workgroup above.
// LDS of one team, G dimensions and Q probabilities at a time (a group: G·Q pairs):
//   [histograms: G·Q · 256 uint64 | rem: G·Q uint64 | prefix: G·Q uint32 | 4·G·Q bytes unused]
// that is 2064 bytes per pair.  A workgroup-team takes G = min(d, max(1, 32 / Q)): at most 32
// pairs, 64.5 KiB, so that two workgroups fit a CU.  A wave-team takes G = min(d, max(1, 8 / Q))
// while Q <= 16: at most 16 pairs per wave, 129 KiB per workgroup.  Above Q = 16 four wave-teams
// would pass the CU's 160 KiB, and the points go to workgroup-teams whatever N.
// One store per (point, dimension, probability); nothing is zeroed in global memory, no global
// atomics: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>

#include "densityflows_hip.h"
#include "df_handle.h"
#include "df_wscale.h"

namespace df {
namespace {

constexpr int kWqThreads = 256;  // 4 waves
constexpr int kWqWaves = kWqThreads / 64;
constexpr int kWqWaveMax = 256;  // N up to which a point is one wave's
constexpr int kWqBins = 256;     // 8-bit digits
constexpr int kWqPasses = 4;
constexpr int kWqBlockPairs = 32;    // pairs of a group, workgroup-team: 64 KiB of histograms
constexpr int kWqWavePairs = 8;      // pairs of a group, wave-team, while Q <= 8 (else one dimension: Q pairs)
constexpr int kWqWaveMaxProbs = 16;  // Q up to which four wave-teams fit a CU
constexpr int kWqPairBytes = 8 * kWqBins + 16;  // histogram, rem, prefix, and 4 bytes that keep a team 16-byte aligned
constexpr size_t kWqLdsMax = 160 * 1024;
constexpr int64_t kWqDrawsMax = (int64_t)1 << 24;
constexpr uint64_t kWqOne = (uint64_t)1 << 32;  // the denominator of a probability

enum WqMap { kWqWave = 0, kWqBlock = 1 };

struct WqNums {
    uint64_t num[DF_WQUANT_MAX_PROBS];
};

__host__ __device__ constexpr int wq_group_dims(int d, int Q, int map) {
    const int cap = map == kWqBlock ? kWqBlockPairs : kWqWavePairs;
    const int g = cap / Q < 1 ? 1 : cap / Q;
    return g < d ? g : d;
}
__host__ __device__ constexpr int wq_team_bytes(int d, int Q, int map) { return wq_group_dims(d, Q, map) * Q * kWqPairBytes; }

static_assert(DF_WQUANT_MAX_PROBS <= kWqBlockPairs, "one dimension's probabilities are one group of a workgroup-team");
static_assert(2 * (size_t)kWqBlockPairs * kWqPairBytes <= kWqLdsMax, "two workgroup-teams fit a CU");
static_assert((size_t)kWqWaves * (kWqWavePairs > kWqWaveMaxProbs ? kWqWavePairs : kWqWaveMaxProbs) * kWqPairBytes <= kWqLdsMax,
              "four wave-team groups past 160 KiB");
static_assert(kWqPairBytes % 16 == 0, "a team's histograms are read and zeroed 16 bytes at a time");
static_assert(kWqDrawsMax * 64 < ((int64_t)1 << 31), "element indices of a point (N·d) are int32");

// df_quant.hip's totalOrder key and its inverse
__device__ __forceinline__ uint32_t wq_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float wq_value(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

template <int MAP>
__device__ __forceinline__ void wq_team_sync() {
    if (MAP == kWqBlock) {
        __syncthreads();
    } else {
        // a wave's own LDS instructions are served in order: this keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

__device__ __forceinline__ uint64_t wq_wave_sum(uint64_t s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, off, 64);
    return s;
}

// w (points · N) → scale: {e, T} per point
template <int MAP>
__global__ void __launch_bounds__(kWqThreads) weight_scale_kernel(const float* __restrict__ w, int N, int64_t points,
                                                                  int64_t* __restrict__ scale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t mx = 0u;
    uint64_t sum = 0;
    int64_t i;
    if (MAP == kWqWave) {
        i = (int64_t)blockIdx.x * kWqWaves + wave;
        if (i >= points) return;  // the whole wave; this mapping has no workgroup barrier
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < N / 4) f = *reinterpret_cast<const float4*>(w + i * N + 4 * lane);
        const uint32_t k[4] = {rs_key(f.x), rs_key(f.y), rs_key(f.z), rs_key(f.w)};
        mx = rs_wave_max(rs_max4(0u, k));
        const int e = rs_exponent(mx);
        sum = wq_wave_sum(rs_quant(k[0], e) + rs_quant(k[1], e) + rs_quant(k[2], e) + rs_quant(k[3], e));
    } else {
        __shared__ uint64_t part[2 * kWqWaves];
        i = blockIdx.x;
        const float4* src = reinterpret_cast<const float4*>(w + i * N);
        const int nv = N / 4;
#pragma unroll 4
        for (int v = tid; v < nv; v += kWqThreads) {
            const float4 f = src[v];
            const uint32_t k[4] = {rs_key(f.x), rs_key(f.y), rs_key(f.z), rs_key(f.w)};
            mx = rs_max4(mx, k);
        }
        mx = rs_wave_max(mx);
        if (lane == 0) part[wave] = mx;
        __syncthreads();
#pragma unroll
        for (int ww = 0; ww < kWqWaves; ++ww) {
            const uint32_t o = (uint32_t)part[ww];
            mx = mx > o ? mx : o;
        }
        const int e = rs_exponent(mx);
#pragma unroll 4
        for (int v = tid; v < nv; v += kWqThreads) {
            const float4 f = src[v];
            sum += rs_quant(rs_key(f.x), e) + rs_quant(rs_key(f.y), e) + rs_quant(rs_key(f.z), e) + rs_quant(rs_key(f.w), e);
        }
        sum = wq_wave_sum(sum);
        if (lane == 0) part[kWqWaves + wave] = sum;
        __syncthreads();
        sum = 0;
#pragma unroll
        for (int ww = 0; ww < kWqWaves; ++ww) sum += part[kWqWaves + ww];
    }
    if ((MAP == kWqWave ? lane : tid) == 0) {
        scale[2 * i] = mx ? rs_exponent(mx) : 0;
        scale[2 * i + 1] = (int64_t)sum;
    }
}

// One wave: the bin of h[0 .. 256) that holds the residual *rem (1 <= rem <= Σ h), and rem inside
// it.  The one lane that holds the bin appends it to *prefix at `shift` and writes the residual
// inside it to *rem.
__device__ __forceinline__ void wq_scan(const uint64_t* h, int lane, uint32_t* prefix, uint64_t* rem, int shift) {
    const ulonglong2 c01 = *reinterpret_cast<const ulonglong2*>(h + 4 * lane);
    const ulonglong2 c23 = *reinterpret_cast<const ulonglong2*>(h + 4 * lane + 2);
    const uint64_t c0 = c01.x, c1 = c01.y, c2 = c23.x;
    const uint64_t own = c0 + c1 + c2 + c23.y;
    uint64_t incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, (unsigned)s, 64);
        if (lane >= s) incl += up;
    }
    const uint64_t r = *rem;  // every lane reads the same word before any lane writes it
    uint64_t below = incl - own;
    wq_team_sync<kWqWave>();
    if (below < r && r <= incl) {  // one lane
        uint32_t bin = 4 * lane;
        if (r > below + c0) {
            below += c0;
            ++bin;
            if (r > below + c1) {
                below += c1;
                ++bin;
                if (r > below + c2) {
                    below += c2;
                    ++bin;
                }
            }
        }
        *prefix |= bin << shift;
        *rem = r - below;
    }
}

// xs (d, points · N): draw j of point i at xs + d·(i·N + j); w (points · N); scale: {e, T} per
// point; out[(i·d + k)·Q + q].
template <int MAP>
__global__ void __launch_bounds__(kWqThreads) wquant_select_kernel(const float* __restrict__ xs,
                                                                   const float* __restrict__ w, int d, int N,
                                                                   int64_t points, const int64_t* __restrict__ scale,
                                                                   WqNums nums, int Q, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wq_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int T = MAP == kWqBlock ? kWqThreads : 64;  // threads of a team
    const int t = MAP == kWqBlock ? tid : lane;           // this thread in its team
    const int64_t i = MAP == kWqBlock ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kWqWaves + wave;
    if (MAP == kWqWave && i >= points) return;  // the whole wave; this mapping has no workgroup barrier
    const int e = (int)scale[2 * i];
    const uint64_t total = (uint64_t)scale[2 * i + 1];
    if (total == 0) {  // the whole team: an empty point
        for (int p = t; p < d * Q; p += T) out[i * d * Q + p] = __uint_as_float(0x7fc00000u);
        return;
    }
    const int G = wq_group_dims(d, Q, MAP);
    unsigned char* mine = wq_lds + (MAP == kWqBlock ? 0 : wave * wq_team_bytes(d, Q, MAP));
    uint64_t* hist = reinterpret_cast<uint64_t*>(mine);
    uint64_t* rem = hist + G * Q * kWqBins;
    uint32_t* prefix = reinterpret_cast<uint32_t*>(rem + G * Q);
    const float4* src = reinterpret_cast<const float4*>(xs + i * N * d);
    const float* wp = w + i * N;
    const int nv = N / 4 * d;  // N·d <= 2^30: element indices stay inside int32

    for (int k0 = 0; k0 < d; k0 += G) {
        const int g = d - k0 < G ? d - k0 : G;  // dimensions of this group
        const int P = g * Q;                    // its pairs
        for (int p = t; p < P; p += T) {
            // τ = max(1, ceil(num·T / 2^32)): num <= 2^32 and T < 2^56, the product below 2^88
            const uint64_t num = nums.num[p % Q];
            const uint64_t hi = __umul64hi(num, total), lo = num * total;
            const uint64_t tau = (hi << 32) + (lo >> 32) + ((lo & 0xffffffffull) ? 1u : 0u);
            prefix[p] = 0u;
            rem[p] = tau ? tau : 1;
        }
        for (int pass = 0; pass < kWqPasses; ++pass) {
            const int shift = 24 - 8 * pass;
            const int H = pass == 0 ? g : P;  // histograms of this pass
            wq_team_sync<MAP>();              // the scans (and the setup) before the zeroing
            for (int v = t; v < H * kWqBins / 2; v += T) reinterpret_cast<uint4*>(hist)[v] = make_uint4(0u, 0u, 0u, 0u);
            wq_team_sync<MAP>();
            for (int v = t; v < nv; v += T) {
                const float4 f = src[v];
                int row = 4 * v / d, col = 4 * v - row * d;  // row and dimension of element 4v
                unsigned long long q = rs_quant(rs_key(wp[row]), e);
                const float vals[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int el = 0; el < 4; ++el) {
                    const int kk = col - k0;
                    if (q != 0 && kk >= 0 && kk < g) {
                        const uint32_t key = wq_key(vals[el]);
                        if (pass == 0) {
                            atomicAdd(reinterpret_cast<unsigned long long*>(&hist[kk * kWqBins + (key >> 24)]), q);
                        } else {
                            const uint32_t digit = (key >> shift) & 255u;
                            for (int qq = 0; qq < Q; ++qq) {
                                const int p = kk * Q + qq;
                                if (((key ^ prefix[p]) >> (shift + 8)) == 0u)
                                    atomicAdd(reinterpret_cast<unsigned long long*>(&hist[p * kWqBins + digit]), q);
                            }
                        }
                    }
                    if (++col == d) {
                        col = 0;
                        ++row;  // element 4v + el + 1 <= 4v + 3 < N·d: a row of the point
                        if (el < 3) q = rs_quant(rs_key(wp[row]), e);
                    }
                }
            }
            wq_team_sync<MAP>();
            // a wave per pair; the waves of a workgroup-team take pairs w, w + 4, ...
            for (int p = MAP == kWqBlock ? wave : 0; p < P; p += MAP == kWqBlock ? kWqWaves : 1)
                wq_scan(hist + (pass == 0 ? p / Q : p) * kWqBins, lane, &prefix[p], &rem[p], shift);
        }
        wq_team_sync<MAP>();
        for (int p = t; p < P; p += T) out[(i * d + k0) * Q + p] = wq_value(prefix[p]);
    }
}

// MaxDynamicSharedMemorySize of an instance = the largest request any launch of it has made in
// this process (the attribute belongs to the function, not to a call)
hipError_t raise_lds_limit(const void* k, int map, size_t lds) {
    static std::mutex mu;
    static size_t limit[2] = {};
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[map];
    if (lds <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

template <int MAP>
hipError_t launch_select(const float* xs, const float* w, int d, int N, int64_t points, const int64_t* scale,
                         const WqNums& nums, int Q, float* out, hipStream_t st) {
    const int64_t per_wg = MAP == kWqBlock ? 1 : kWqWaves;
    const size_t lds = (size_t)per_wg * wq_team_bytes(d, Q, MAP);
    if (lds > kWqLdsMax) return hipErrorInvalidValue;  // the static_asserts above: not reached
    const void* k = reinterpret_cast<const void*>(&wquant_select_kernel<MAP>);
    const hipError_t e = raise_lds_limit(k, MAP, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((wquant_select_kernel<MAP>), dim3((unsigned)((points + per_wg - 1) / per_wg)), dim3(kWqThreads),
                       lds, st, xs, w, d, N, points, scale, nums, Q, out);
    return hipGetLastError();
}

// the rules of n_points and n_draws every per-point call shares
int check_points_draws(int64_t n_points, int64_t n_draws) {
    if (n_points < 0) return api::set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0) return api::set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kWqDrawsMax) return api::set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    return DF_OK;
}

}  // namespace

namespace api {

int launch_weight_scale(const float* w, int64_t points, int N, int64_t* scale, hipStream_t st) {
    const bool wave = N <= kWqWaveMax;
    const int64_t blocks = wave ? (points + kWqWaves - 1) / kWqWaves : points;
    if (blocks > 0x7fffffff) return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    if (wave)
        hipLaunchKernelGGL((weight_scale_kernel<kWqWave>), dim3((unsigned)blocks), dim3(kWqThreads), 0, st, w, N, points, scale);
    else
        hipLaunchKernelGGL((weight_scale_kernel<kWqBlock>), dim3((unsigned)blocks), dim3(kWqThreads), 0, st, w, N, points, scale);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DF_OK : hip_err(e, "weight scale kernel launch");
}

}  // namespace api
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_draw_weight_scale(const float* w, int64_t n_points, int64_t n_draws, int64_t* scale_out, void* stream) {
    const int rc = check_points_draws(n_points, n_draws);
    if (rc != DF_OK) return rc;
    if (!w || !scale_out) return set_err(DF_ERR_INVALID, "null w or scale_out array");
    if (reinterpret_cast<uintptr_t>(w) % 16 != 0) return set_err(DF_ERR_INVALID, "w must be 16-byte aligned");
    if (n_points > (INT64_MAX / 16) / n_draws) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    if (n_points == 0) return DF_OK;
    return launch_weight_scale(w, n_points, (int)n_draws, scale_out, static_cast<hipStream_t>(stream));
}

int df_draw_weighted_quantiles(const float* xs, const float* w, int d, int64_t n_points, int64_t n_draws,
                               const uint64_t* nums, int n_probs, float* quant_out, int64_t* scale_out, void* stream) {
    if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
    int rc = check_points_draws(n_points, n_draws);
    if (rc != DF_OK) return rc;
    if (!xs || !w) return set_err(DF_ERR_INVALID, "null xs or w array");
    if (!quant_out || !scale_out) return set_err(DF_ERR_INVALID, "null quant_out or scale_out array");
    if (!nums) return set_err(DF_ERR_INVALID, "null nums array");
    if (reinterpret_cast<uintptr_t>(xs) % 16 != 0) return set_err(DF_ERR_INVALID, "xs must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(w) % 16 != 0) return set_err(DF_ERR_INVALID, "w must be 16-byte aligned");
    if (n_probs < 1 || n_probs > DF_WQUANT_MAX_PROBS)
        return set_err(DF_ERR_UNSUPPORTED, "n_probs must be in 1 .. DF_WQUANT_MAX_PROBS (32)");
    WqNums nm = {};
    for (int q = 0; q < n_probs; ++q) {
        if (nums[q] > kWqOne)
            return set_err(DF_ERR_INVALID, "nums[" + std::to_string(q) + "] = " + std::to_string(nums[q]) + " is above 2^32");
        nm.num[q] = nums[q];
    }
    if (n_points > (INT64_MAX / 8) / n_draws / d) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    if (n_points == 0) return DF_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_draws;
    const bool wave = N <= kWqWaveMax && n_probs <= kWqWaveMaxProbs;
    if ((wave ? (n_points + kWqWaves - 1) / kWqWaves : n_points) > 0x7fffffff)
        return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    if ((rc = launch_weight_scale(w, n_points, N, scale_out, st)) != DF_OK) return rc;
    const hipError_t e = wave ? launch_select<kWqWave>(xs, w, d, N, n_points, scale_out, nm, n_probs, quant_out, st)
                              : launch_select<kWqBlock>(xs, w, d, N, n_points, scale_out, nm, n_probs, quant_out, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "weighted quantile kernel launch");
}

}  // extern "C"
