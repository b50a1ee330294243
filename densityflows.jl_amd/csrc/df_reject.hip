// df_reject.hip — sample_with_rejection(condition, flow, dims, θ, m) on the device
// (src/Flows.jl:196-229) for a described region: a box lo ≤ x ≤ hi and up to 8 half-spaces
// a·x ≤ b.  The reference draws one sample per loop iteration; here a round of candidates
// is drawn (Philox, df_random_normal's stream), sent through the fused forward!, tested,
// and the accepted ones are compacted IN ORDER behind those of the rounds before, until
// n_want slots are filled or max_tries candidates were examined.
//
// Per round, on the caller's stream: draw → θ broadcast → forward! → predicate_kernel
// (one ballot per wave) → scan_kernel (ONE workgroup: exclusive scan of the ballots'
// popcounts, the round's base and the new totals into the counters) → scatter_kernel →
// a 16-byte read-back of the counters and a stream synchronisation, which decides whether
// another round is needed.  No atomics, no scratch, no workgroup waits on another one.
//
// Candidate k is forward! of elements [d·k, d·k + d) of the (seed, offset) stream, whatever
// the rounds: a round starts at a multiple of 4 candidates, so at Philox counter
// offset + d·k0/4.  The result is the first n_want accepted candidates in increasing k.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kRejThreads = 256;               // 4 waves: thread index / 64 is the ballot's index
constexpr int kRejScanPer = 4;                 // ballots per thread and trip of the scan
constexpr int kRejMaxDim = 64;                 // df_limits.max_state
constexpr int64_t kRejMinRound = 1024;         // adaptive rounds: [2¹⁰, 2²²] candidates
constexpr int64_t kRejMaxRound = 1 << 22;
constexpr int64_t kRejMaxFixedRound = 1 << 24; // a caller's round: 64 floats · 2²⁴ < 2³¹ elements
constexpr int kRejRegionFloats = 2 * kRejMaxDim + DF_REGION_MAX_HALFSPACES * (kRejMaxDim + 1);

// One thread per candidate of the round: the region's predicate, one ballot per wave.
// reg = [lo (d) | hi (d) | a (n_half, d) row by row | b (n_half)].  count: the candidates
// of this round that are examined (the clip at max_tries is already in it); lanes past it
// read nothing and vote 0.  Every lane of a launched wave reaches the ballot.
__global__ void __launch_bounds__(kRejThreads) reject_predicate_kernel(const float* __restrict__ cand,
                                                                       const float* __restrict__ reg,
                                                                       uint64_t* __restrict__ mask, int d, int n_half,
                                                                       int32_t count, int32_t n_masks) {
#pragma clang fp contract(off)
    const int32_t i = (int32_t)(blockIdx.x * kRejThreads + threadIdx.x);
    bool pass = false;
    if (i < count) {
        const float* x = cand + (int64_t)d * i;
        const float* lo = reg;
        const float* hi = reg + d;
        const float* a = reg + 2 * d;
        const float* b = a + n_half * d;
        pass = true;
        float acc[DF_REGION_MAX_HALFSPACES];
        for (int k = 0; k < d; ++k) {
            const float xk = x[k];
            pass = pass && lo[k] <= xk && xk <= hi[k];  // a NaN coordinate rejects
#pragma unroll
            for (int h = 0; h < DF_REGION_MAX_HALFSPACES; ++h) {
                if (h < n_half) {
                    const float p = a[h * d + k] * xk;
                    acc[h] = k == 0 ? p : acc[h] + p;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < DF_REGION_MAX_HALFSPACES; ++h)
            if (h < n_half) pass = pass && acc[h] <= b[h];
    }
    const uint64_t m = __ballot(pass);
    const int32_t wave = i >> 6;
    if ((threadIdx.x & 63) == 0 && wave < n_masks) mask[wave] = m;
}

// Four consecutive ballots of the round, zero past its end (mask is 32-byte aligned at i).
__device__ __forceinline__ void load_ballots(const uint64_t* __restrict__ mask, int32_t i, int32_t n_masks,
                                             uint64_t (&m)[kRejScanPer]) {
    if (i + kRejScanPer <= n_masks) {
        const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(mask + i);
        const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(mask + i + 2);
        m[0] = lo.x, m[1] = lo.y, m[2] = hi.x, m[3] = hi.y;
    } else {
#pragma unroll
        for (int q = 0; q < kRejScanPer; ++q) m[q] = i + q < n_masks ? mask[i + q] : 0ull;
    }
}

// ONE workgroup: wave_base[w] = Σ_{v<w} popcount(mask[v]) over the round's n_masks ballots,
// 1024 at a time (four consecutive ones per thread) with a running carry, the next trip's
// ballots loaded before this trip's scan; then cnt[2] = the accepted count before the round
// (the round's base), cnt[0] += the round's accepted.
__global__ void __launch_bounds__(kRejThreads) reject_scan_kernel(const uint64_t* __restrict__ mask,
                                                                  uint32_t* __restrict__ wave_base, int32_t n_masks,
                                                                  int64_t* cnt) {
    // the four waves' totals, double-buffered: a trip's writes cannot overtake the reads
    // of the trip before, which all end before that trip's barrier
    __shared__ uint32_t wtot[2][kRejThreads / 64];
    constexpr int32_t kTrip = kRejThreads * kRejScanPer;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t carry = 0;
    int buf = 0;
    uint64_t m[kRejScanPer], nxt[kRejScanPer];
    load_ballots(mask, kRejScanPer * t, n_masks, m);
    for (int32_t first = 0; first < n_masks; first += kTrip, buf ^= 1) {
        const int32_t idx = first + kRejScanPer * t;
        load_ballots(mask, idx + kTrip, n_masks, nxt);
        uint32_t v[kRejScanPer], mine = 0;
#pragma unroll
        for (int q = 0; q < kRejScanPer; ++q) {
            v[q] = (uint32_t)__popcll(m[q]);
            mine += v[q];
        }
        uint32_t s = mine;  // inclusive scan of the threads' sums inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(s, off, 64);
            if (lane >= off) s += u;
        }
        if (lane == 63) wtot[buf][w] = s;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kRejThreads / 64; ++j) {
            const uint32_t x = wtot[buf][j];
            if (j < w) before += x;
            total += x;
        }
        uint32_t base = carry + before + (s - mine);
        if (idx + kRejScanPer <= n_masks) {
            *reinterpret_cast<uint4*>(wave_base + idx) = uint4{base, base + v[0], base + v[0] + v[1],
                                                               base + v[0] + v[1] + v[2]};
        } else {
#pragma unroll
            for (int q = 0; q < kRejScanPer; ++q) {
                if (idx + q < n_masks) wave_base[idx + q] = base;
                base += v[q];
            }
        }
        carry += total;
#pragma unroll
        for (int q = 0; q < kRejScanPer; ++q) m[q] = nxt[q];
    }
    if (t == 0) {
        const int64_t base = cnt[0];
        cnt[2] = base;
        cnt[0] = base + (int64_t)carry;
    }
}

// One thread per examined candidate: slot = round base + wave base + rank in the wave.  An
// accepted candidate with slot < n_want copies its d floats; the one that fills the last
// slot stores tried = its index + 1.  No other lane stores anything.
__global__ void __launch_bounds__(kRejThreads) reject_scatter_kernel(const float* __restrict__ cand,
                                                                     const uint64_t* __restrict__ mask,
                                                                     const uint32_t* __restrict__ wave_base,
                                                                     int64_t* cnt, float* __restrict__ x_out, int d,
                                                                     int32_t count, int64_t k0, int64_t n_want) {
    const int32_t i = (int32_t)(blockIdx.x * kRejThreads + threadIdx.x);
    if (i >= count) return;
    const int32_t wave = i >> 6;
    const int lane = i & 63;
    const uint64_t m = mask[wave];
    if (!((m >> lane) & 1ull)) return;
    const int64_t slot = cnt[2] + (int64_t)wave_base[wave] + __popcll(m & ((1ull << lane) - 1ull));
    if (slot >= n_want) return;
    const float* src = cand + (int64_t)d * i;
    float* dst = x_out + (int64_t)d * slot;
    for (int k = 0; k < d; ++k) dst[k] = src[k];
    if (slot == n_want - 1) cnt[1] = k0 + i + 1;
}

inline int64_t round_up4(int64_t v) { return (v + 3) / 4 * 4; }

// The adaptive schedule (round = 0).  Integer arithmetic only: flows.py restates it for the
// closure path, so both cut the candidate stream at the same places.
inline int64_t first_round(int64_t n_want) {
    const int64_t want = 2 * std::min(n_want, kRejMaxRound);
    return round_up4(std::min(std::max(want, kRejMinRound), kRejMaxRound));
}
// remaining / (accepted / examined), a quarter of head-room and 64 more
inline int64_t next_round(int64_t remaining, int64_t examined, int64_t accepted, int64_t prev) {
    int64_t want;
    if (accepted == 0) {
        want = 2 * prev;
    } else {
        const unsigned __int128 num = (unsigned __int128)remaining * (uint64_t)examined * 5u;
        const unsigned __int128 den = (unsigned __int128)accepted * 4u;
        const unsigned __int128 q = (num + den - 1) / den + 64;
        want = q > (unsigned __int128)kRejMaxRound ? kRejMaxRound : (int64_t)q;
    }
    return round_up4(std::min(std::max(want, kRejMinRound), kRejMaxRound));
}

bool has_nan(const float* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (std::isnan(v[i])) return true;
    return false;
}

}  // namespace
}  // namespace df

using namespace df::api;

extern "C" {

int df_flow_sample_region(df_chain* c, float* x_out, const float* theta_raw, int64_t n_want,
                          const df_region* region, int64_t max_tries, int64_t round, uint64_t seed, uint64_t offset,
                          int64_t* tried_out, int64_t* accepted_out, void* stream) {
    // ---- validation, before any device work ----
    // (the region's own checks first: they need no chain, so no device either)
    if (!region) return set_err(DF_ERR_INVALID, c ? "null region" : "null chain");
    const int d = region->d, n_half = region->n_half;
    if (d < 1 || d > df::kRejMaxDim) return set_err(DF_ERR_SHAPE, "the region's dimension must be the flow's d");
    if (n_half < 0 || n_half > DF_REGION_MAX_HALFSPACES)
        return set_err(DF_ERR_UNSUPPORTED, "a region holds 0 to 8 half-spaces");
    if (n_half > 0 && (!region->a || !region->b)) return set_err(DF_ERR_INVALID, "null half-space arrays");
    if ((region->lo && df::has_nan(region->lo, d)) || (region->hi && df::has_nan(region->hi, d)) ||
        (n_half > 0 && (df::has_nan(region->a, (int64_t)n_half * d) || df::has_nan(region->b, n_half))))
        return set_err(DF_ERR_INVALID, "NaN in the region (lo, hi, a or b)");
    if (n_want < 0 || max_tries < 0) return set_err(DF_ERR_SHAPE, "negative n_want or max_tries");
    if (round < 0) return set_err(DF_ERR_SHAPE, "negative round size");
    if (round > df::kRejMaxFixedRound) return set_err(DF_ERR_UNSUPPORTED, "a round holds at most 2^24 candidates");
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    const int n = c->plan.n;
    if (d != c->plan.d) return set_err(DF_ERR_SHAPE, "the region's dimension must be the flow's d");
    if (tried_out) *tried_out = 0;
    if (accepted_out) *accepted_out = 0;
    if (n_want == 0) return DF_OK;
    if (!x_out) return set_err(DF_ERR_INVALID, "null output array");
    if (n > 0 && !theta_raw)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    if (n > 0 && !c->has_bounds) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds)");

    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
        if (cap != hipStreamCaptureStatusNone)
            return set_err(DF_ERR_INVALID, "df_flow_sample_region synchronises every round: not inside a stream capture");
    }
    hipError_t e;
    if (!c->d_rej_region.get()) {
        if (c->d_rej_region.alloc(sizeof(float) * df::kRejRegionFloats) != hipSuccess ||
            c->d_rej_cnt.alloc(sizeof(int64_t) * 4) != hipSuccess) {
            c->d_rej_region.reset();
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (region block)");
        }
    }
    // the region block, uploaded once per call; the host copy belongs to the chain, so it
    // outlives the copy whatever this call returns
    {
        std::vector<float>& r = c->h_rej_region;
        r.assign((size_t)(2 * d + n_half * (d + 1)), 0.f);
        for (int k = 0; k < d; ++k) {
            r[k] = region->lo ? region->lo[k] : -INFINITY;
            r[d + k] = region->hi ? region->hi[k] : INFINITY;
        }
        for (int i = 0; i < n_half * d; ++i) r[2 * d + i] = region->a[i];
        for (int h = 0; h < n_half; ++h) r[2 * d + n_half * d + h] = region->b[h];
        e = hipMemcpyAsync(c->d_rej_region.get(), r.data(), sizeof(float) * r.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_err(e, "hipMemcpyAsync(region)");
    }
    int64_t* cnt = c->d_rej_cnt.as<int64_t>();
    if ((e = hipMemsetAsync(cnt, 0, sizeof(int64_t) * 4, st)) != hipSuccess) return hip_err(e, "hipMemsetAsync(counters)");

    int64_t R = round > 0 ? df::round_up4(round) : df::first_round(n_want);
    int64_t k0 = 0, accepted = 0, tried = 0;
    while (k0 < max_tries) {
        if (R > c->rej_cap) {
            if (c->d_rej_cand.get()) {
                // the workspaces belong to the chain, not to a stream: an earlier call on
                // any stream may still read them
                if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_err(e, "hipDeviceSynchronize");
            }
            c->rej_cap = 0;
            const size_t waves = (size_t)((R + 63) / 64);
            if (c->d_rej_cand.alloc(sizeof(float) * (size_t)d * R) != hipSuccess ||
                (n > 0 && c->d_rej_theta.alloc(sizeof(float) * (size_t)n * R) != hipSuccess) ||
                c->d_rej_mask.alloc(sizeof(uint64_t) * waves) != hipSuccess ||
                c->d_rej_base.alloc(sizeof(uint32_t) * waves) != hipSuccess) {
                c->d_rej_cand.reset();
                return set_err(DF_ERR_NOMEM, "hipMalloc failed (rejection workspaces)");
            }
            c->rej_cap = R;
        }
        float* cand = c->d_rej_cand.as<float>();
        int rc = df_random_normal(cand, (int64_t)d * R, seed, offset + (uint64_t)((int64_t)d * (k0 / 4)), stream);
        if (rc != DF_OK) return rc;
        const float* th = nullptr;
        if (n > 0) {
            rc = df_theta_broadcast(c->d_rej_theta.as<float>(), theta_raw, n, R, stream);
            if (rc != DF_OK) return rc;
            th = c->d_rej_theta.as<float>();
        }
        rc = df_flow_forward_inplace(c, cand, th, R, stream);
        if (rc != DF_OK) return rc;

        const int32_t count = (int32_t)std::min(R, max_tries - k0);  // examined this round
        const int32_t n_masks = (count + 63) / 64;
        const unsigned blocks = (unsigned)((count + df::kRejThreads - 1) / df::kRejThreads);
        hipLaunchKernelGGL(df::reject_predicate_kernel, dim3(blocks), dim3(df::kRejThreads), 0, st, cand,
                           c->d_rej_region.as<float>(), c->d_rej_mask.as<uint64_t>(), d, n_half, count, n_masks);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "reject_predicate_kernel launch");
        hipLaunchKernelGGL(df::reject_scan_kernel, dim3(1), dim3(df::kRejThreads), 0, st,
                           c->d_rej_mask.as<uint64_t>(), c->d_rej_base.as<uint32_t>(), n_masks, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "reject_scan_kernel launch");
        hipLaunchKernelGGL(df::reject_scatter_kernel, dim3(blocks), dim3(df::kRejThreads), 0, st, cand,
                           c->d_rej_mask.as<uint64_t>(), c->d_rej_base.as<uint32_t>(), cnt, x_out, d, count, k0,
                           n_want);
        if ((e = hipGetLastError()) != hipSuccess) return hip_err(e, "reject_scatter_kernel launch");

        // the one synchronisation of a round: is another one needed?
        int64_t host_cnt[2] = {0, 0};
        if ((e = hipMemcpyAsync(host_cnt, cnt, sizeof(host_cnt), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_err(e, "hipMemcpyAsync(counters)");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_err(e, "hipStreamSynchronize");
        k0 += count;
        accepted = std::min(host_cnt[0], n_want);
        tried = host_cnt[0] >= n_want ? host_cnt[1] : k0;
        if (host_cnt[0] >= n_want) break;
        if (round == 0) R = df::next_round(n_want - host_cnt[0], k0, host_cnt[0], R);
    }
    if (tried_out) *tried_out = tried;
    if (accepted_out) *accepted_out = accepted;
    if (accepted < n_want)
        return set_err(DF_ERR_INVALID, "Impossible to reach convergence of rejection sampling: " +
                                           std::to_string(accepted) + " of " + std::to_string(n_want) +
                                           " accepted after " + std::to_string(tried) + " candidates");
    return DF_OK;
}

}  // extern "C"
