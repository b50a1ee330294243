// df_grid.hip — logpdf(flow, (x₁, …, x_d), (θ₁, …, θ_n)) on the outer product of axis
// vectors (src/Flows.jl:287-331): a generator kernel writes the points of one chunk of the
// grid into a per-chain staging buffer, in the (d, m) / (n, m) layout df_flow_logpdf reads,
// and the fused logpdf pass runs on it — chunk after chunk on the caller's stream, so one
// staging buffer serves every chunk.  The analogue of df_sample.hip (Philox draw, then the
// fused forward!): nothing of size P = ∏ lengths is built on the host or copied over.
//
// Point order: p = i₁ + L₁·(i₂ + L₂·(…)), the first axis fastest (Iterators.product, and
// Julia's column-major reshape(…, lens...)).  The kernel copies axis values and does no
// arithmetic on them.  A chain-pass kernel's output for a sample does not depend on where
// the sample sits in the batch, so a chunked grid is bitwise df_flow_logpdf of the
// materialised points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "densityflows_hip.h"
#include "df_handle.h"

namespace df {
namespace {

constexpr int kGridMaxAxes = 64;                   // d + n ≤ df_limits.max_state
constexpr int64_t kGridDefaultChunk = 1 << 20;     // the headline batch
constexpr int64_t kGridMaxChunk = 1 << 24;         // 64 axes · 2²⁴ points: element index < 2³¹

// Axis k of the grid for the chunk that starts at point p0, with s_k = ∏_{a<k} L_a:
// p0 = Q·s_k + rem and base = Q mod L_k, so point p0 + j has
// i_k = (base + ⌊(rem + j) / s_k⌋) mod L_k: the device divides j-sized numbers by the
// stride, never the point number.  A wave64 VALU instruction takes four cycles and a 32-bit
// division expands to some thirty instructions, two per staged float; the host therefore gives each
// divisor v in [2, 2³¹) its multiplier M = ⌊2⁶⁴/v⌋ + 1 (2⁶⁴/v for a power of two):
// ⌊a/v⌋ = ⌊a·M / 2⁶⁴⌋ for every a < 2³², since a·v < 2⁶⁴.
struct GridAxis {
    uint64_t stride, len;    // s_k, L_k
    uint64_t mstride, mlen;  // their multipliers; 0 for a divisor of 1 or ≥ 2³¹
    uint64_t base, rem;
    int64_t off;             // first value of the axis in `axes`
};
struct GridDesc {
    GridAxis ax[kGridMaxAxes];
};

inline uint64_t grid_multiplier(uint64_t v) { return v >= 2 && v < (1ull << 31) ? ~0ull / v + 1 : 0; }

// ⌊a·M / 2⁶⁴⌋
__device__ __forceinline__ uint32_t mul_hi64(uint32_t a, uint64_t M) {
    return (uint32_t)(((uint64_t)a * (uint32_t)(M >> 32) + __umulhi(a, (uint32_t)M)) >> 32);
}

// i_k of point p0 + j, j ≤ 2²⁴ + 3
__device__ __forceinline__ uint64_t grid_index(const GridAxis& a, uint32_t j) {
    const uint64_t t = a.rem + j;  // < s_k + 2²⁵
    uint64_t q;                    // ⌊t / s_k⌋
    if (a.mstride)
        q = mul_hi64((uint32_t)t, a.mstride);  // s_k < 2³¹: t < 2³²
    else
        q = a.stride == 1 ? t : (uint64_t)(t >= a.stride);  // s_k ≥ 2³¹ > j: 0 or 1
    const uint64_t u = a.base + q;
    if (a.mlen && (u >> 32) == 0) return (uint32_t)u - mul_hi64((uint32_t)u, a.mlen) * (uint32_t)a.len;
    return a.len == 1 ? 0 : u % a.len;  // an axis of 2³¹ values or more
}

// threads of one launch: four staged floats each, the x array then the θ array
__host__ __device__ inline uint32_t grid_threads(uint32_t floats) { return (floats + 3) / 4; }

// One thread per four consecutive staged floats of the (d, m) x array, then of the (n, m) θ
// array (sample j's values contiguous): consecutive lanes store consecutive 16 bytes, and a
// thread's four descriptor → axis-value chains of dependent loads are in flight together.
// Both arrays start 256-byte aligned.  The elements a segment's last thread computes past
// its end have a valid axis index too; they are not stored.
__global__ void __launch_bounds__(256) grid_fill_kernel(uint32_t* __restrict__ xs, uint32_t* __restrict__ ths,
                                                        const uint32_t* __restrict__ axes, GridDesc g,
                                                        uint32_t d, uint32_t n, uint32_t m) {
    // The descriptors go through LDS: a lane reads the one of its axis, and read in place
    // that is a vector load from the kernel-argument segment for every staged float
    // (24.7 µs against 15.3 µs for the 21 MB of a 2²⁰-point chunk at d = 5).
    __shared__ GridAxis s_ax[kGridMaxAxes];
    {
        constexpr uint32_t kWords = sizeof(GridAxis) / sizeof(uint64_t);
        const uint64_t* from = reinterpret_cast<const uint64_t*>(g.ax);
        uint64_t* to = reinterpret_cast<uint64_t*>(s_ax);
        for (uint32_t w = threadIdx.x; w < (d + n) * kWords; w += 256u) to[w] = from[w];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t tx = grid_threads(d * m);
    if (i >= tx + grid_threads(n * m)) return;
    const bool th = i >= tx;
    const uint32_t e0 = 4u * (th ? i - tx : i);
    const uint32_t rows = th ? n : d, first_axis = th ? d : 0u, total = rows * m;
    uint32_t j = e0 / rows, k = e0 - j * rows;
    // three passes, so that the four descriptor loads, then the four value loads, are issued
    // back to back (the index arithmetic between them branches)
    GridAxis a[4];
    uint32_t jq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = s_ax[first_axis + k];
        jq[q] = j;
        if (++k == rows) {
            k = 0;
            ++j;
        }
    }
    const uint32_t* src[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        src[q] = axes + a[q].off + (int64_t)grid_index(a[q], jq[q]);
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *src[q];
    uint32_t* dst = (th ? ths : xs) + e0;
    if (e0 + 4 <= total) {
        *reinterpret_cast<uint4*>(dst) = uint4{v[0], v[1], v[2], v[3]};
    } else {
        for (uint32_t q = 0; q < 4 && e0 + q < total; ++q) dst[q] = v[q];
    }
}

}  // namespace
}  // namespace df

using namespace df::api;

extern "C" {

int df_flow_logpdf_grid(df_chain* c, const float* axes, const int64_t* lens, int64_t first, int64_t count,
                        float* logpdf_out, int64_t chunk, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (!lens) return set_err(DF_ERR_INVALID, "null axis lengths");
    const int d = c->plan.d, n = c->plan.n, na = d + n;
    if (na > df::kGridMaxAxes) return set_err(DF_ERR_UNSUPPORTED, "more than 64 grid axes");
    bool empty = false;
    for (int k = 0; k < na; ++k) {
        if (lens[k] < 0) return set_err(DF_ERR_SHAPE, "negative axis length");
        empty = empty || lens[k] == 0;
    }
    int64_t P = empty ? 0 : 1;
    for (int k = 0; k < na && !empty; ++k)
        if (__builtin_mul_overflow(P, lens[k], &P)) return set_err(DF_ERR_SHAPE, "grid size overflows int64");
    if (first < 0 || count < 0 || first > P || count > P - first)
        return set_err(DF_ERR_SHAPE, "window [first, first + count) outside the grid");
    if (count == 0) return DF_OK;
    if (!axes) return set_err(DF_ERR_INVALID, "null axis values");
    if (!logpdf_out) return set_err(DF_ERR_INVALID, "null logpdf output");
    if (n > 0 && !c->has_bounds) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds)");
    if (chunk < 0) return set_err(DF_ERR_SHAPE, "negative chunk size");

    // a multiple of 64 points: every chunk's output keeps logpdf_out's alignment to 256 bytes
    if (chunk == 0) chunk = df::kGridDefaultChunk;
    chunk = std::min((chunk + 63) / 64 * 64, df::kGridMaxChunk);
    chunk = std::min(chunk, (count + 63) / 64 * 64);

    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int64_t need = (int64_t)na * chunk;
    if (need > c->grid_ws_cap) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
        if (cap != hipStreamCaptureStatusNone)
            return set_err(DF_ERR_INVALID, "the grid staging workspace cannot grow during a stream capture");
        if (c->d_grid_ws.get()) {
            // the workspace belongs to the chain, not to a stream: an earlier grid call on
            // any stream may still read it
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_err(e, "hipDeviceSynchronize");
        }
        c->grid_ws_cap = 0;
        if (c->d_grid_ws.alloc(sizeof(float) * need) != hipSuccess)
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (grid staging)");
        c->grid_ws_cap = need;
    }
    float* xs = c->d_grid_ws.as<float>();
    float* ths = n > 0 ? xs + (int64_t)d * chunk : nullptr;  // 256-byte aligned: chunk is a multiple of 64

    df::GridDesc g{};
    {
        uint64_t stride = 1;
        int64_t off = 0;
        for (int k = 0; k < na; ++k) {
            g.ax[k].stride = stride;
            g.ax[k].len = (uint64_t)lens[k];
            g.ax[k].mstride = df::grid_multiplier(stride);
            g.ax[k].mlen = df::grid_multiplier((uint64_t)lens[k]);
            g.ax[k].off = off;
            stride *= (uint64_t)lens[k];  // ≤ P
            off += lens[k];
        }
    }
    for (int64_t p0 = first; p0 < first + count; p0 += chunk) {
        const int64_t m = std::min(chunk, first + count - p0);
        for (int k = 0; k < na; ++k) {
            df::GridAxis& a = g.ax[k];
            a.base = ((uint64_t)p0 / a.stride) % a.len;
            a.rem = (uint64_t)p0 % a.stride;
        }
        // (d + n) · m ≤ 64 · 2²⁴ floats
        const uint32_t threads = df::grid_threads((uint32_t)(d * m)) + df::grid_threads((uint32_t)(n * m));
        hipLaunchKernelGGL(df::grid_fill_kernel, dim3((threads + 255) / 256), dim3(256), 0, st,
                           reinterpret_cast<uint32_t*>(xs), reinterpret_cast<uint32_t*>(ths),
                           reinterpret_cast<const uint32_t*>(axes), g, (uint32_t)d, (uint32_t)n, (uint32_t)m);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_err(e, "grid_fill_kernel launch");
        const int rc = run(c, df::MODE_LOGPDF, true, xs, ths, nullptr, nullptr, logpdf_out + (p0 - first), nullptr, m,
                           stream);
        if (rc != DF_OK) return rc;
    }
    return DF_OK;
}

}  // extern "C"
