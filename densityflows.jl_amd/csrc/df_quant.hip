// df_quant.hip — order statistics of per-point draws, per dimension, on the device:
//   df_order_statistics       the requested order statistics of every dimension of every point
//                             of a caller-owned (d, n_points · n_draws) array of draws
//   df_flow_point_quantiles   df_flow_point_stats' chunk loop (df_pstats.hip: point_draw_chunks)
//                             with the selection at its end: quantiles, and on request the SBC
//                             ranks, the sums and the draws, of one sampling pass
//
// The order is IEEE totalOrder on Float32: key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000),
// compared as uint32 (−NaN < −inf < ... < −0 < +0 < ... < +inf < +NaN).  The order statistic r
// of a point's dimension is the draw whose key is the r-th smallest; it is returned with its own
// bits (the key map is a bijection), and ties hold equal bits.
//
// order_select_kernel: one form for every N = n_draws, radix select, most significant digit
// first, 8-bit digits, 4 passes over the point's d · N contiguous floats (16-byte loads, read
// from global memory / L2 each pass: nothing of the draws is kept in LDS).  A pair is a
// (dimension, order).  Pass 0 counts the top digit once per dimension (no prefix yet: the
// orders of a dimension share the histogram); passes 1-3 count, per pair, the next digit of the
// draws whose higher digits equal the pair's prefix.  Counting is ds_add_u32 on a 256-bin
// histogram in LDS (integer sums: any order gives the same counts).  After each pass a wave
// scans a pair's histogram — lane l holds bins 4l .. 4l + 3, an inclusive scan over the lanes —
// finds the one bin b with below(b) <= rem < below(b) + count(b), appends b to the prefix and
// subtracts below(b) from the residual rank rem.  rem < (draws under the prefix) holds
// throughout, so exactly one bin answers.  After pass 3 the prefix is the key.
// The rows are N·d/4 whole float4 (N % 4 == 0): no lane reads past the point's last draw, and a
// lane past the last vector counts nothing.
//
// With N = n_draws the mapping of points follows from N alone, as in point_stats_kernel:
//   N <= 256   a wave per point, 4 points per workgroup, no workgroup barrier
//   above      a workgroup (4 waves) per point; the waves share the histograms, wave w scans
//              pairs w, w + 4, ...; workgroup barriers between counting and scanning
// The unit that owns a point (wave or workgroup) is a team.
//
// LDS of one team, G dimensions and Q orders at a time (a group: G·Q pairs):
//   [histograms: G·Q · 256 uint32 | prefix: G·Q uint32 | rem: G·Q int32 | 8·G·Q bytes unused]
// (pass 0 uses the first G histograms).  G follows from Q on the host: a workgroup-team takes
// G = min(d, 64 / Q) (at most 64 KiB of histograms, so that two workgroups fit a CU), a
// wave-team G = min(d, max(1, 16 / Q)) (at most 32 KiB per wave, 130 KiB per workgroup at
// Q = 32).  d dimensions are walked in ceil(d / G) groups; every group reads the point's draws
// again (4 passes each).  One store per (point, dimension, order); nothing is zeroed in global
// memory, no global atomics: two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kQsThreads = 256;  // 4 waves
constexpr int kQsWaves = kQsThreads / 64;
constexpr int kQsWaveMax = 256;  // N up to which a point is one wave's
constexpr int kQsBins = 256;     // 8-bit digits
constexpr int kQsPasses = 4;
constexpr int kQsBlockPairs = 64;  // pairs of a group, workgroup-team: 64 KiB of histograms
constexpr int kQsWavePairs = 16;   // pairs of a group, wave-team, while Q <= 16 (else one dimension: Q pairs)
constexpr int kQsPairBytes = 4 * kQsBins + 16;  // histogram, prefix, rem, and 8 bytes that keep a team 16-byte aligned
constexpr size_t kQsLdsMax = 160 * 1024;
constexpr int64_t kQsDrawsMax = (int64_t)1 << 24;

enum QsMap { kQsWave = 0, kQsBlock = 1 };

struct QsOrders {
    int32_t r[DF_QUANT_MAX_ORDERS];
};

__host__ __device__ constexpr int qs_group_dims(int d, int Q, int map) {
    const int cap = map == kQsBlock ? kQsBlockPairs : kQsWavePairs;
    const int g = cap / Q < 1 ? 1 : cap / Q;
    return g < d ? g : d;
}
__host__ __device__ constexpr int qs_team_bytes(int d, int Q, int map) { return qs_group_dims(d, Q, map) * Q * kQsPairBytes; }

// the cutoffs: the largest group of either mapping fits the 160 KiB of a CU
static_assert(DF_QUANT_MAX_ORDERS <= kQsBlockPairs, "one dimension's orders are one group of a workgroup-team");
static_assert((size_t)kQsBlockPairs * kQsPairBytes <= kQsLdsMax, "workgroup-team group past 160 KiB");
static_assert((size_t)kQsWaves * (kQsWavePairs > DF_QUANT_MAX_ORDERS ? kQsWavePairs : DF_QUANT_MAX_ORDERS) * kQsPairBytes <=
                  kQsLdsMax,
              "four wave-team groups past 160 KiB");
static_assert(kQsPairBytes % 16 == 0, "a wave-team's histograms are read and zeroed 16 bytes at a time");
static_assert(kQsDrawsMax * 64 < ((int64_t)1 << 31), "element indices of a point (N·d), counts and residual ranks are int32");

__device__ __forceinline__ uint32_t qs_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float qs_value(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

template <int MAP>
__device__ __forceinline__ void qs_team_sync() {
    if (MAP == kQsBlock) {
        __syncthreads();
    } else {
        // a wave's own LDS instructions are served in order: this keeps the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// One wave: the bin of h[0 .. 256) that holds rank rem (0 <= rem < Σ h), and rem inside it.
// The one lane that holds the bin appends it to *prefix at `shift` and writes the rank inside it to *rem.
__device__ __forceinline__ void qs_scan(const uint32_t* h, int lane, uint32_t* prefix, int32_t* rem, int shift) {
    const uint4 c = *reinterpret_cast<const uint4*>(h + 4 * lane);
    const uint32_t own = c.x + c.y + c.z + c.w;
    uint32_t incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s, 64);
        if (lane >= s) incl += up;
    }
    const uint32_t r = (uint32_t)*rem;  // every lane reads the same word before any lane writes it
    uint32_t below = incl - own;
    qs_team_sync<kQsWave>();
    if (below <= r && r < incl) {  // one lane
        uint32_t bin = 4 * lane;
        if (r >= below + c.x) {
            below += c.x;
            ++bin;
            if (r >= below + c.y) {
                below += c.y;
                ++bin;
                if (r >= below + c.z) {
                    below += c.z;
                    ++bin;
                }
            }
        }
        *prefix |= bin << shift;
        *rem = (int32_t)(r - below);
    }
}

// xs (d, points · N): draw j of point i at xs + d·(i·N + j); out[(i·d + k)·Q + q].
template <int MAP>
__global__ void __launch_bounds__(kQsThreads) order_select_kernel(const float* __restrict__ xs, int d, int N,
                                                                  int64_t points, QsOrders ord, int Q,
                                                                  float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int T = MAP == kQsBlock ? kQsThreads : 64;  // threads of a team
    const int t = MAP == kQsBlock ? tid : lane;           // this thread in its team
    const int64_t i = MAP == kQsBlock ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kQsWaves + wave;
    if (MAP == kQsWave && i >= points) return;  // the whole wave; this mapping has no workgroup barrier
    const int G = qs_group_dims(d, Q, MAP);
    unsigned char* mine = qs_lds + (MAP == kQsBlock ? 0 : wave * qs_team_bytes(d, Q, MAP));
    uint32_t* hist = reinterpret_cast<uint32_t*>(mine);
    uint32_t* prefix = hist + G * Q * kQsBins;
    int32_t* rem = reinterpret_cast<int32_t*>(prefix + G * Q);
    const float4* src = reinterpret_cast<const float4*>(xs + i * N * d);
    const int nv = N / 4 * d;  // N·d <= 2^30: element indices stay inside int32

    for (int k0 = 0; k0 < d; k0 += G) {
        const int g = d - k0 < G ? d - k0 : G;  // dimensions of this group
        const int P = g * Q;                    // its pairs
        for (int p = t; p < P; p += T) {
            prefix[p] = 0u;
            rem[p] = ord.r[p % Q];
        }
        for (int pass = 0; pass < kQsPasses; ++pass) {
            const int shift = 24 - 8 * pass;
            const int H = pass == 0 ? g : P;  // histograms of this pass
            qs_team_sync<MAP>();              // the scans (and the setup) before the zeroing
            for (int w = t; w < H * kQsBins / 4; w += T) reinterpret_cast<uint4*>(hist)[w] = make_uint4(0u, 0u, 0u, 0u);
            qs_team_sync<MAP>();
            for (int v = t; v < nv; v += T) {
                const float4 f = src[v];
                int col = 4 * v % d;  // dimension of element 4v
                const float vals[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kk = col - k0;
                    if (kk >= 0 && kk < g) {
                        const uint32_t key = qs_key(vals[e]);
                        if (pass == 0) {
                            atomicAdd(&hist[kk * kQsBins + (key >> 24)], 1u);
                        } else {
                            const uint32_t digit = (key >> shift) & 255u;
                            for (int q = 0; q < Q; ++q) {
                                const int p = kk * Q + q;
                                if (((key ^ prefix[p]) >> (shift + 8)) == 0u) atomicAdd(&hist[p * kQsBins + digit], 1u);
                            }
                        }
                    }
                    if (++col == d) col = 0;
                }
            }
            qs_team_sync<MAP>();
            // a wave per pair; the waves of a workgroup-team take pairs w, w + 4, ...
            for (int p = MAP == kQsBlock ? wave : 0; p < P; p += MAP == kQsBlock ? kQsWaves : 1)
                qs_scan(hist + (pass == 0 ? p / Q : p) * kQsBins, lane, &prefix[p], &rem[p], shift);
        }
        qs_team_sync<MAP>();
        for (int p = t; p < P; p += T) out[(i * d + k0) * Q + p] = qs_value(prefix[p]);
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
hipError_t launch_map(const float* xs, int d, int N, int64_t points, const QsOrders& ord, int Q, float* out,
                      hipStream_t st) {
    const int64_t per_wg = MAP == kQsBlock ? 1 : kQsWaves;
    const size_t lds = (size_t)(MAP == kQsBlock ? 1 : kQsWaves) * qs_team_bytes(d, Q, MAP);
    if (lds > kQsLdsMax) return hipErrorInvalidValue;  // the static_asserts above: not reached for Q <= 32
    const void* k = reinterpret_cast<const void*>(&order_select_kernel<MAP>);
    const hipError_t e = raise_lds_limit(k, MAP, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((order_select_kernel<MAP>), dim3((unsigned)((points + per_wg - 1) / per_wg)), dim3(kQsThreads), lds,
                       st, xs, d, N, points, ord, Q, out);
    return hipGetLastError();
}

}  // namespace

namespace api {

int check_orders(const int32_t* orders, int n_orders, int64_t n_draws) {
    if (!orders) return set_err(DF_ERR_INVALID, "null orders array");
    if (n_orders < 1 || n_orders > DF_QUANT_MAX_ORDERS)
        return set_err(DF_ERR_UNSUPPORTED, "n_orders must be in 1 .. DF_QUANT_MAX_ORDERS (32)");
    for (int q = 0; q < n_orders; ++q)
        if (orders[q] < 0 || orders[q] >= n_draws)
            return set_err(DF_ERR_INVALID, "orders[" + std::to_string(q) + "] = " + std::to_string(orders[q]) +
                                               " is outside [0, n_draws)");
    return DF_OK;
}

int launch_order_statistics(const float* xs, int d, int N, int64_t points, const int32_t* orders, int n_orders,
                            float* out, hipStream_t st) {
    QsOrders ord = {};
    for (int q = 0; q < n_orders; ++q) ord.r[q] = orders[q];
    if ((N <= kQsWaveMax ? (points + kQsWaves - 1) / kQsWaves : points) > 0x7fffffff)
        return set_err(DF_ERR_UNSUPPORTED, "too many points for one launch");
    const hipError_t e = N <= kQsWaveMax ? launch_map<kQsWave>(xs, d, N, points, ord, n_orders, out, st)
                                         : launch_map<kQsBlock>(xs, d, N, points, ord, n_orders, out, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "order statistics kernel launch");
}

}  // namespace api
}  // namespace df

using namespace df;
using namespace df::api;

extern "C" {

int df_order_statistics(const float* xs, int d, int64_t n_points, int64_t n_draws, const int32_t* orders,
                        int n_orders, float* out, void* stream) {
    if (d < 1 || d > 64) return set_err(DF_ERR_INVALID, "d must be in 1 .. 64");
    if (n_points < 0) return set_err(DF_ERR_SHAPE, "negative point count");
    if (n_draws <= 0 || n_draws % 4 != 0) return set_err(DF_ERR_INVALID, "n_draws must be a positive multiple of 4");
    if (n_draws > kQsDrawsMax) return set_err(DF_ERR_UNSUPPORTED, "a point has at most 2^24 draws (n_draws)");
    if (!xs || !out) return set_err(DF_ERR_INVALID, "null xs or out array");
    if (reinterpret_cast<uintptr_t>(xs) % 16 != 0) return set_err(DF_ERR_INVALID, "xs must be 16-byte aligned");
    const int rc = check_orders(orders, n_orders, n_draws);
    if (rc != DF_OK) return rc;
    if (n_points == 0) return DF_OK;
    if (n_points > (INT64_MAX / 8) / n_draws / d) return set_err(DF_ERR_SHAPE, "n_points · n_draws past int64");
    return launch_order_statistics(xs, d, (int)n_draws, n_points, orders, n_orders, out,
                                   static_cast<hipStream_t>(stream));
}

int df_flow_point_quantiles(df_chain* c, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                            int64_t chunk, uint64_t seed, uint64_t offset, const int32_t* orders, int n_orders,
                            float* quant_out, int32_t* rank_out, double* sums_out, float* draws_out, void* stream) {
    int rc = point_check_sizes(c, n_points, n_draws, chunk);
    if (rc != DF_OK) return rc;
    if (!quant_out && !rank_out && !sums_out && !draws_out)
        return set_err(DF_ERR_INVALID, "no output: quant_out, rank_out, sums_out and draws_out are all null");
    if (rank_out && !x) return set_err(DF_ERR_INVALID, "rank_out needs the points x (null input array)");
    if (quant_out && (rc = check_orders(orders, n_orders, n_draws)) != DF_OK) return rc;
    if (n_points == 0) return DF_OK;
    PointOutputs out;
    out.rank = rank_out;
    out.sums = sums_out;
    out.draws = draws_out;
    if (quant_out) {
        out.orders = orders;
        out.n_orders = n_orders;
        out.quant = quant_out;
    }
    return point_draw_chunks(c, x, theta_raw, n_points, n_draws, chunk, seed, offset, out, stream);
}

}  // extern "C"
