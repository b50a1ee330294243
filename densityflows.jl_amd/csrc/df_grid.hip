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
//
// df_flow_pdf_marginals runs the same two launches per chunk with the logpdf values kept in
// the staging buffer, and a third, grid_marginal_kernel, that reduces exp(logpdf) · (the
// quadrature weights of the integrated axes) into the requested 0-, 1- and 2-D tables: the
// grid-sized array never leaves the chunk.
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

// ---- marginal tables (df_flow_pdf_marginals) -------------------------------------------------
constexpr int kMargMaxReq = 128;         // a d = 11 corner is 1 + 11 + 55 = 67 requests
constexpr uint32_t kMargLdsBins = 6144;  // 48 KiB of fp64 bins per workgroup: three workgroups fit a CU's 160 KiB
constexpr uint8_t kMargNone = 0xFF;      // no kept axis in this slot
constexpr int kMargSmallAxes = 8;        // grids of up to 8 axes: the instance with 8 slots per point

// Request r keeps the axes a[r] < b[r] (kMargNone: unused; a one-axis request uses a).
// pass[r]: the pass its table is accumulated in.  Passes [0, n_lds_pass) each hold tables of
// at most kMargLdsBins bins in all, in LDS; requests with a larger table share one more pass,
// which adds to `out` directly.  Table offsets follow from the lengths: the kernel sums them.
struct alignas(4) MargDesc {
    uint8_t a[kMargMaxReq], b[kMargMaxReq], pass[kMargMaxReq];
};
static_assert(sizeof(GridDesc) + sizeof(MargDesc) + 64 <= 4096, "grid_marginal_kernel's arguments");

// Entry r of one of MargDesc's arrays, read in the kernel-argument segment as an aligned
// word: with r the same in every lane it is a scalar load, and what is selected or indexed
// with it (a pass, an axis slot) stays in scalar registers.
__device__ __forceinline__ uint32_t marg_byte(const uint8_t* v, uint32_t r) {
    return (reinterpret_cast<const uint32_t*>(v)[r >> 2] >> ((r & 3u) * 8u)) & 0xFFu;
}

// v of the lane the DPP control names, 0.0 where it names none (or the row is masked out)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ double dpp_or_zero(double v) {
    const uint64_t u = __double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_update_dpp(0u, (uint32_t)u, kCtrl, kRowMask, 0xF, false);
    const uint32_t hi = __builtin_amdgcn_update_dpp(0u, (uint32_t)(u >> 32), kCtrl, kRowMask, 0xF, false);
    return __longlong_as_double(((uint64_t)hi << 32) | lo);
}

// Lane 63 ends with the sum of the 64 lanes, added in an order that does not depend on the
// data: a scan along each row of 16 lanes (row_shr 1, 2, 4, 8), then lane 15 of a row into
// the row above (row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3).  Data-
// parallel moves in the VALU, no LDS round trip per step.
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_or_zero<0x111, 0xF>(v);
    v += dpp_or_zero<0x112, 0xF>(v);
    v += dpp_or_zero<0x114, 0xF>(v);
    v += dpp_or_zero<0x118, 0xF>(v);
    v += dpp_or_zero<0x142, 0xA>(v);
    v += dpp_or_zero<0x143, 0xC>(v);
    return v;
}

// After a chunk's logpdf pass: out[table r][i_K] += Σ exp(lp[j]) · ∏_{k ∉ K_r} w_k[i_k(j)] over
// the chunk's m points, in fp64.  Workgroup g takes the `span` consecutive points from
// g · span (span a multiple of 256), a wave 64 consecutive ones at a time, so a kept axis
// with a stride of 64 or more is constant across a wave but for the waves in which it steps.
// Per request, a wave whose 64 points share one bin adds them up across its lanes (wave_sum)
// and issues one add; any other wave adds lane by lane.  In an LDS pass those adds go to the
// workgroup's table (ds_add_f64), which is flushed when the workgroup has seen all its
// points: one global_atomic_add_f64 per workgroup and bin that is not zero.  NA: slots per
// point (index, weight, prefix and suffix product of every axis); the loops that fill them
// are unrolled, and a request reads the slots of its kept axes with a wave-uniform index
// held in a scalar register (no scratch for NA = 8; the 64-slot instance of grids of more
// than 8 axes keeps the slots in scratch).  The loop over the requests is a chain of
// dependent steps at two waves per SIMD: its descriptors are scalar loads and the wave sum
// stays in the VALU, so that no step of it waits for an LDS round trip.
template <int NA>
__global__ void __launch_bounds__(256)
grid_marginal_kernel(const float* __restrict__ lp, const double* __restrict__ weights, double* __restrict__ out,
                     GridDesc g, MargDesc q, uint32_t na, uint32_t n_req, uint32_t n_lds_pass, uint32_t n_pass,
                     uint32_t tab_bins, uint32_t m, uint32_t span) {
    __shared__ GridAxis s_ax[kGridMaxAxes];
    __shared__ uint64_t s_off[kMargMaxReq], s_size[kMargMaxReq];  // table r in `out`: first bin, bins
    __shared__ uint32_t s_loff[kMargMaxReq];                      // ... its first bin in s_tab
    __shared__ uint8_t s_a[kMargMaxReq], s_b[kMargMaxReq], s_pass[kMargMaxReq];
    extern __shared__ double s_tab[];  // tab_bins
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    {
        constexpr uint32_t kWords = sizeof(GridAxis) / sizeof(uint64_t);
        const uint64_t* from = reinterpret_cast<const uint64_t*>(g.ax);
        uint64_t* to = reinterpret_cast<uint64_t*>(s_ax);
        for (uint32_t w = tid; w < na * kWords; w += 256u) to[w] = from[w];
        if (tid < n_req) {
            s_a[tid] = q.a[tid];
            s_b[tid] = q.b[tid];
            s_pass[tid] = q.pass[tid];
        }
    }
    __syncthreads();
    if (tid < n_req) {
        const uint64_t la = s_a[tid] == kMargNone ? 1 : s_ax[s_a[tid]].len;
        s_size[tid] = la * (s_b[tid] == kMargNone ? 1 : s_ax[s_b[tid]].len);
    }
    __syncthreads();
    if (tid < n_req) {
        uint64_t off = 0;
        uint32_t loff = 0;
        for (uint32_t r = 0; r < tid; ++r) {
            off += s_size[r];
            if (s_pass[r] == s_pass[tid]) loff += (uint32_t)s_size[r];  // an LDS pass: ≤ kMargLdsBins in all
        }
        s_off[tid] = off;
        s_loff[tid] = loff;
    }
    const uint32_t j0 = blockIdx.x * span, j1 = min(m, j0 + span);  // j0 < m ≤ 2²⁴

    for (uint32_t pass = 0; pass < n_pass; ++pass) {
        const bool lds = pass < n_lds_pass;
        __syncthreads();  // the offsets; the flush of the pass before
        if (lds) {
            for (uint32_t i = tid; i < tab_bins; i += 256u) s_tab[i] = 0.0;
            __syncthreads();
        }
        for (uint32_t jb = j0 + (tid - lane); jb < j1; jb += 256u) {  // uniform across a wave
            const bool live = jb + lane < j1;
            const uint32_t j = live ? jb + lane : j1 - 1;  // a lane past the end: the last point, weight 0
            // pre[k] = e · ∏_{i<k} w_i and suf[k] = ∏_{i≥k} w_i: a request's excluded product
            // is pre[a] · (the weights between a and b) · suf[b + 1], never a quotient
            uint64_t idx[NA];
            double w[NA], pre[NA + 1], suf[NA + 1];
            pre[0] = exp((double)lp[j]);
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                idx[k] = 0;
                w[k] = 1.0;
                if (k < (int)na) {
                    idx[k] = grid_index(s_ax[k], j);
                    w[k] = weights[s_ax[k].off + (int64_t)idx[k]];
                }
                pre[k + 1] = pre[k] * w[k];
            }
            suf[NA] = 1.0;
#pragma unroll
            for (int k = NA - 1; k >= 0; --k) suf[k] = suf[k + 1] * w[k];
            for (uint32_t r = 0; r < n_req; ++r) {
                if (marg_byte(q.pass, r) != pass) continue;
                const uint32_t a = marg_byte(q.a, r), b = marg_byte(q.b, r);
                double v;
                uint64_t bin = 0;
                if (a == kMargNone) {
                    v = pre[NA];
                } else {
                    uint32_t hi = a;  // the highest kept axis
                    bin = idx[a];
                    v = pre[a];
                    if (b != kMargNone) {
                        hi = b;
                        bin += g.ax[a].len * idx[hi];
                        for (uint32_t k = a + 1; k < hi; ++k) v *= w[k];
                    }
                    v *= suf[hi + 1];
                }
                if (!live) v = 0.0;
                const uint64_t bin0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(bin >> 32)) << 32) |
                                      __builtin_amdgcn_readfirstlane((uint32_t)bin);
                const bool one_bin = __ballot(bin != bin0) == 0;  // a lane past the end has the last point's bin
                if (one_bin) v = wave_sum(v);
                // a zero changes no sum (and stays out of the bins the window does not reach)
                if ((one_bin ? lane == 63 : live) && v != 0.0) {
                    if (lds)
                        unsafeAtomicAdd(&s_tab[s_loff[r] + (uint32_t)bin], v);
                    else
                        unsafeAtomicAdd(out + s_off[r] + bin, v);
                }
            }
        }
        if (lds) {
            __syncthreads();
            for (uint32_t r = 0; r < n_req; ++r) {
                if (s_pass[r] != pass) continue;
                for (uint32_t i = tid; i < (uint32_t)s_size[r]; i += 256u) {
                    const double v = s_tab[s_loff[r] + i];
                    if (v != 0.0) unsafeAtomicAdd(out + s_off[r] + i, v);
                }
            }
        }
    }
}

}  // namespace
}  // namespace df

using namespace df::api;

namespace {

// The checks the grid entry points share: lengths, the grid's size P and the window.
int grid_check_window(const df_chain* c, const int64_t* lens, int64_t first, int64_t count) {
    const int na = c->plan.d + c->plan.n;
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
    return DF_OK;
}

// a multiple of 64 points: every chunk's output keeps its buffer's alignment to 256 bytes
int64_t grid_chunk(int64_t chunk, int64_t count) {
    if (chunk == 0) chunk = df::kGridDefaultChunk;
    chunk = std::min((chunk + 63) / 64 * 64, df::kGridMaxChunk);
    return std::min(chunk, (count + 63) / 64 * 64);
}

// The chain's staging buffer holds `need` floats after this; it only grows.
int grid_reserve(df_chain* c, int64_t need, hipStream_t st) {
    if (need <= c->grid_ws_cap) return DF_OK;
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
    return DF_OK;
}

void grid_describe(df::GridDesc& g, const int64_t* lens, int na) {
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

// Stage the m points from point p0 on: [x (d, m) | θ (n, m)] at xs / ths.
int grid_stage(df::GridDesc& g, int d, int n, int64_t p0, int64_t m, float* xs, float* ths, const float* axes,
               hipStream_t st) {
    for (int k = 0; k < d + n; ++k) {
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
    return DF_OK;
}

}  // namespace

extern "C" {

int df_flow_logpdf_grid(df_chain* c, const float* axes, const int64_t* lens, int64_t first, int64_t count,
                        float* logpdf_out, int64_t chunk, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (!lens) return set_err(DF_ERR_INVALID, "null axis lengths");
    const int d = c->plan.d, n = c->plan.n, na = d + n;
    if (const int rc = grid_check_window(c, lens, first, count)) return rc;
    if (count == 0) return DF_OK;
    if (!axes) return set_err(DF_ERR_INVALID, "null axis values");
    if (!logpdf_out) return set_err(DF_ERR_INVALID, "null logpdf output");
    if (n > 0 && !c->has_bounds) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds)");
    if (chunk < 0) return set_err(DF_ERR_SHAPE, "negative chunk size");
    chunk = grid_chunk(chunk, count);

    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = grid_reserve(c, (int64_t)na * chunk, st)) return rc;
    float* xs = c->d_grid_ws.as<float>();
    float* ths = n > 0 ? xs + (int64_t)d * chunk : nullptr;  // 256-byte aligned: chunk is a multiple of 64

    df::GridDesc g{};
    grid_describe(g, lens, na);
    for (int64_t p0 = first; p0 < first + count; p0 += chunk) {
        const int64_t m = std::min(chunk, first + count - p0);
        if (const int rc = grid_stage(g, d, n, p0, m, xs, ths, axes, st)) return rc;
        const int rc = run(c, df::MODE_LOGPDF, true, xs, ths, nullptr, nullptr, logpdf_out + (p0 - first), nullptr, m,
                           stream);
        if (rc != DF_OK) return rc;
    }
    return DF_OK;
}

int df_flow_pdf_marginals(df_chain* c, const float* axes, const double* weights, const int64_t* lens, int64_t first,
                          int64_t count, const int32_t* keep, int32_t n_marg, double* out, int64_t chunk,
                          void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (!lens) return set_err(DF_ERR_INVALID, "null axis lengths");
    if (n_marg < 0) return set_err(DF_ERR_INVALID, "negative number of marginal requests");
    if (n_marg > 0 && !keep) return set_err(DF_ERR_INVALID, "null marginal requests");
    if (n_marg > 0 && !out) return set_err(DF_ERR_INVALID, "null marginal output");
    const int d = c->plan.d, n = c->plan.n, na = d + n;
    if (const int rc = grid_check_window(c, lens, first, count)) return rc;
    if (n_marg > df::kMargMaxReq) return set_err(DF_ERR_UNSUPPORTED, "more than 128 marginal requests");

    // the requests, their tables' sizes, and the pass each table is accumulated in: an LDS
    // pass takes tables first-fit up to kMargLdsBins bins, larger tables share the last pass
    df::MargDesc q{};
    int64_t total = 0;
    uint32_t fill[df::kMargMaxReq] = {};
    int n_lds = 0;
    bool direct = false;
    for (int r = 0; r < n_marg; ++r) {
        const int32_t a = keep[2 * r], b = keep[2 * r + 1];
        if (a < -1 || a >= na || b < -1 || b >= na || (a < 0 && b >= 0) || (b >= 0 && b <= a))
            return set_err(DF_ERR_INVALID, "kept axes must be in [0, d + n), ascending and distinct (-1: unused)");
        int64_t size = a < 0 ? 1 : lens[a];
        if (b >= 0 && __builtin_mul_overflow(size, lens[b], &size))
            return set_err(DF_ERR_SHAPE, "marginal table size overflows int64");
        if (__builtin_add_overflow(total, size, &total) || total > INT64_MAX / (int64_t)sizeof(double))
            return set_err(DF_ERR_SHAPE, "total marginal table size overflows int64");
        q.a[r] = a < 0 ? df::kMargNone : (uint8_t)a;
        q.b[r] = b < 0 ? df::kMargNone : (uint8_t)b;
        if (size > (int64_t)df::kMargLdsBins) {
            q.pass[r] = df::kMargNone;  // numbered below
            direct = true;
            continue;
        }
        int p = 0;
        while (p < n_lds && fill[p] + size > df::kMargLdsBins) ++p;
        if (p == n_lds) ++n_lds;
        fill[p] += (uint32_t)size;
        q.pass[r] = (uint8_t)p;
    }
    for (int r = 0; r < n_marg; ++r)
        if (q.pass[r] == df::kMargNone) q.pass[r] = (uint8_t)n_lds;
    if (n_marg == 0) return DF_OK;
    if (count > 0) {
        if (!axes) return set_err(DF_ERR_INVALID, "null axis values");
        if (!weights) return set_err(DF_ERR_INVALID, "null axis weights");
        if (n > 0 && !c->has_bounds)
            return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds)");
        if (chunk < 0) return set_err(DF_ERR_SHAPE, "negative chunk size");
    }

    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (total > 0) {
        const hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * (size_t)total, st);
        if (e != hipSuccess) return hip_err(e, "hipMemsetAsync(marginal tables)");
    }
    if (count == 0) return DF_OK;
    chunk = grid_chunk(chunk, count);
    // the staging of df_flow_logpdf_grid and one chunk of logpdf values behind it
    if (const int rc = grid_reserve(c, (int64_t)(na + 1) * chunk, st)) return rc;
    float* xs = c->d_grid_ws.as<float>();
    float* ths = n > 0 ? xs + (int64_t)d * chunk : nullptr;
    float* lp = xs + (int64_t)na * chunk;

    const uint32_t tab_bins = *std::max_element(fill, fill + df::kMargMaxReq);
    const int wgs = 2 * std::max(c->n_cu, 1);  // two resident workgroups per CU
    auto kernel = na <= df::kMargSmallAxes ? df::grid_marginal_kernel<df::kMargSmallAxes>
                                           : df::grid_marginal_kernel<df::kGridMaxAxes>;
    df::GridDesc g{};
    grid_describe(g, lens, na);
    for (int64_t p0 = first; p0 < first + count; p0 += chunk) {
        const int64_t m = std::min(chunk, first + count - p0);
        if (const int rc = grid_stage(g, d, n, p0, m, xs, ths, axes, st)) return rc;
        const int rc = run(c, df::MODE_LOGPDF, true, xs, ths, nullptr, nullptr, lp, nullptr, m, stream);
        if (rc != DF_OK) return rc;
        // consecutive points per workgroup: a multiple of 256, at most 2²⁴
        const int64_t span = std::max<int64_t>(256, ((m + wgs - 1) / wgs + 255) / 256 * 256);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)((m + span - 1) / span)), dim3(256), sizeof(double) * tab_bins, st,
                           lp, weights, out, g, q, (uint32_t)na, (uint32_t)n_marg, (uint32_t)n_lds,
                           (uint32_t)(n_lds + (direct ? 1 : 0)), tab_bins, (uint32_t)m, (uint32_t)span);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_err(e, "grid_marginal_kernel launch");
    }
    return DF_OK;
}

}  // extern "C"
