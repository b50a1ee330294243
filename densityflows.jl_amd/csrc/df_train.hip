// df_train.hip — training kernels: the per-net reverse sweep (df_train_impl.h,
// instantiated for hidden widths 16/32/64 and 0 or 1 hidden Dense), and the
// element-wise steps around it (z̄ seed, NormalizationLayer adjoint, the
// fixed-order gradient reduction, Adam, weight regathering).
#include "df_train_impl.h"

namespace df {

namespace {

#ifndef DF_TRAIN_NAF
#define DF_TRAIN_NAF 1
#endif
// naf: the transformed-dim count; the SPLIT instances for 2 and 3 (d = 5 chains) have it
// at compile time (DF_TRAIN_NAF)
template <bool WT>
void* train_ptr_w(int ht, int nh, int am, bool split, int naf) {
    if (split) {
        if (nh != 1 || am != trn::AM_RELU) return nullptr;
        const int nf = DF_TRAIN_NAF ? naf : 0;
        if (ht == 2) return nf == 2 ? train_kernel_ptr<2, 1, trn::AM_RELU, true, 2, WT>()
                            : nf == 3 ? train_kernel_ptr<2, 1, trn::AM_RELU, true, 3, WT>()
                                      : train_kernel_ptr<2, 1, trn::AM_RELU, true, 0, WT>();
        if (ht == 4) return nf == 2 ? train_kernel_ptr<4, 1, trn::AM_RELU, true, 2, WT>()
                            : nf == 3 ? train_kernel_ptr<4, 1, trn::AM_RELU, true, 3, WT>()
                                      : train_kernel_ptr<4, 1, trn::AM_RELU, true, 0, WT>();
        return nullptr;
    }
#define DF_T(H)                                                                                           \
    (nh ? (am == trn::AM_RELU ? train_kernel_ptr<H, 1, trn::AM_RELU, false, 0, WT>()                     \
                              : (am == trn::AM_PRE ? train_kernel_ptr<H, 1, trn::AM_PRE, false, 0, WT>()  \
                                                   : train_kernel_ptr<H, 1, trn::AM_Y, false, 0, WT>()))  \
        : (am == trn::AM_RELU ? train_kernel_ptr<H, 0, trn::AM_RELU, false, 0, WT>()                     \
                              : (am == trn::AM_PRE ? train_kernel_ptr<H, 0, trn::AM_PRE, false, 0, WT>()  \
                                                   : train_kernel_ptr<H, 0, trn::AM_Y, false, 0, WT>())))
    switch (ht) {
        case 1: return DF_T(1);
        case 2: return DF_T(2);
        case 4: return DF_T(4);
        default: return nullptr;
    }
#undef DF_T
}

// wt: the weighted instance (j̄ per sample from TrainArgs::wj)
void* train_ptr(int ht, int nh, int am, bool split = false, int naf = 0, bool wt = false) {
    return wt ? train_ptr_w<true>(ht, nh, am, split, naf) : train_ptr_w<false>(ht, nh, am, split, naf);
}

// z̄ = z / N
__global__ void scale_kernel(float* dst, const float* src, float s, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[i] * s;
}

// The weighted seed: z̄[i][:] = z[i][:] · wj[i]
__global__ void scale_rows_kernel(float* dst, const float* src, const float* wj, int d, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[i] * wj[i / d];
}

// ---- sample weights (df_train_gradient_w) ----
// Fixed-order fp64 sums.  A batch is cut into spans of kWsumSpan elements, one workgroup
// each: thread t adds its span's elements t, t + 256, ... in increasing order, then the
// workgroup's tree over LDS; the span sums are added the same way by one workgroup.  The
// order depends on the element count alone.  v(i) is the i-th term.
template <typename Term>
__device__ inline double wsum_block(int64_t count, double* red, Term&& v) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kWsumThreads) s += v(i);
    __syncthreads();  // (red may still be read from the previous sum)
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = kWsumThreads / 2; k >= 1; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + k];
        __syncthreads();
    }
    return red[0];
}

// part[b] = Σ over span b of w_i · lp_i (fp64 product of the two floats), or of w_i (lp == nullptr)
__global__ __launch_bounds__(kWsumThreads) void wsum_partial_kernel(const float* w, const float* lp, int64_t count,
                                                                    double* part) {
    __shared__ double red[kWsumThreads];
    const int64_t b0 = (int64_t)blockIdx.x * kWsumSpan;
    const int64_t n = count - b0 < kWsumSpan ? count - b0 : kWsumSpan;
    const double s = lp ? wsum_block(n, red, [&](int64_t i) { return (double)w[b0 + i] * (double)lp[b0 + i]; })
                        : wsum_block(n, red, [&](int64_t i) { return (double)w[b0 + i]; });
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kWsumThreads) void wsum_final_kernel(const double* part, int64_t n_parts, double* out) {
    __shared__ double red[kWsumThreads];
    const double s = wsum_block(n_parts, red, [&](int64_t i) { return part[i]; });
    if (threadIdx.x == 0) *out = s;
}

// wj = w · inv_W over span blockIdx.x, inv_W = 1.f / (float)W.  W is w_total when that is > 0,
// else Σ w: the sum of the n_parts span sums in part (every workgroup adds them in the same
// order), or with one span the sum of w itself.  wsums[1] = W (wsums may be nullptr).  Only
// w_total comes from the host: a replayed graph sums the weights it finds.
__global__ __launch_bounds__(kWsumThreads) void weight_norm_kernel(const float* w, int64_t count, double w_total,
                                                                   const double* part, int64_t n_parts, float* wj,
                                                                   double* wsums) {
    __shared__ double red[kWsumThreads];
    double W = w_total;
    if (!(w_total > 0.0))
        W = n_parts > 1 ? wsum_block(n_parts, red, [&](int64_t i) { return part[i]; })
                        : wsum_block(count, red, [&](int64_t i) { return (double)w[i]; });
    const float inv_w = 1.f / (float)W;
    const int64_t b0 = (int64_t)blockIdx.x * kWsumSpan;
    const int64_t n = count - b0 < kWsumSpan ? count - b0 : kWsumSpan;
    for (int64_t i = threadIdx.x; i < n; i += kWsumThreads) wj[b0 + i] = w[b0 + i] * inv_w;
    if (blockIdx.x == 0 && threadIdx.x == 0 && wsums) wsums[1] = W;
}

// NormalizationLayer inverse z = (β(x - x_min) + α(x_max - x)) / x_diff
// (src/norm/Normalization.jl:66-76):  x̄ = z̄ · (β - α) / x_diff
__global__ void norm_adjoint_kernel(float* zbar, const float* xmin, const float* xmax, float alpha, float beta,
                                    int d, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const int c = (int)(i % d);
        zbar[i] = zbar[i] * ((beta - alpha) / (xmax[c] - xmin[c]));
    }
}

// ∇[p] = Σ_w partial[w][p], w in increasing order (bitwise reproducible)
__global__ void reduce_grads_kernel(const float* partial, int n_parts, int64_t p_total, float* grad) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= p_total) return;
    float s = 0.f;
    for (int w = 0; w < n_parts; ++w) s += partial[(int64_t)w * p_total + p];
    grad[p] = s;
}

// The same sums, four parameters per thread (p_total % 4 == 0): 16-byte loads, eight
// partial rows in flight per thread; each sum still runs over w in increasing order.
__global__ void reduce_grads4_kernel(const float* partial, int n_parts, int64_t p_total, float* grad) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p >= p_total) return;
    v4 s = v4{0.f, 0.f, 0.f, 0.f};
    int w = 0;
    for (; w + 8 <= n_parts; w += 8) {
        v4 r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = *reinterpret_cast<const v4*>(partial + (int64_t)(w + k) * p_total + p);
#pragma unroll
        for (int k = 0; k < 8; ++k) s = s + r[k];
    }
    for (; w < n_parts; ++w) s = s + *reinterpret_cast<const v4*>(partial + (int64_t)w * p_total + p);
    *reinterpret_cast<v4*>(grad + p) = s;
}

// Optimisers.Adam (apply!, Optimisers.jl v0.4):
//   m = β1 m + (1-β1) g;  v = β2 v + (1-β2) g²
//   x -= m / (1-β1ᵗ) / (sqrt(v / (1-β2ᵗ)) + ϵ) · η          (all Float32)
// βᵗ lives on the device (bt[0], bt[1]) so that a captured train step (hipGraph)
// replays with the current power; adam_advance_kernel moves it on after the update.
__global__ void adam_kernel(float* x, const float* g, float* m, float* v, int64_t count, float eta, float b1,
                            float b2, float eps, const float* bt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float bt1 = bt[0], bt2 = bt[1];
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float upd = mi / (1.f - bt1) / (sqrtf(vi / (1.f - bt2)) + eps) * eta;
    x[i] = x[i] - upd;
}

__global__ void adam_advance_kernel(float* bt, float b1, float b2) {
    if (threadIdx.x == 0) {
        bt[0] = bt[0] * b1;  // βᵗ .* β in Float32 (Optimisers.Adam)
        bt[1] = bt[1] * b2;
    }
}

// ---- optimiser chains (Optimisers.OptimiserChain): dx = g through the rules in order ----
// Every rule is one fixed sequence of correctly rounded Float32 operations, so a Float32
// restatement matches it: contraction is off in each function below (as the Makefile's
// -ffp-contract=off has it for the whole unit), and / and sqrtf round correctly.

// clamp(dx, -δ, δ) as Base.clamp: a NaN passes through
__device__ inline float opt_clip_grad(float dx, float delta) {
    return dx > delta ? delta : (dx < -delta ? -delta : dx);
}

__device__ inline float opt_weight_decay(float dx, float x, float lambda) {
#pragma clang fp contract(off)
    const float lx = lambda * x;
    return dx + lx;
}

// The stateless rules [0, n_pre) that stand before the chain's ClipNorm.
__device__ inline float opt_pre_rules(const OptChain& ch, int n_pre, float dx, float x) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < kOptMaxRules; ++r) {
        if (r >= n_pre) break;
        const float p0 = ch.p[r][0];
        switch (ch.kind[r]) {
            case DF_OPT_CLIP_GRAD: dx = opt_clip_grad(dx, p0); break;
            case DF_OPT_WEIGHT_DECAY: dx = opt_weight_decay(dx, x, p0); break;
            case DF_OPT_DESCENT: dx = p0 * dx; break;
            default: break;
        }
    }
    return dx;
}

// out[t] = Σ dx² over tensor t (or its square root), one workgroup per tensor.  Element j of
// the tensor belongs to quad q = j / 4, thread q % 256, accumulator j % 4; each accumulator
// adds its quads in increasing order, then (a0 + a1) + (a2 + a3), then the workgroup's tree
// over LDS: the same order on every run and for both load widths (16-byte loads when the
// tensor starts on a 16-byte boundary, scalar loads otherwise).  The longest chain of
// additions is kSumsqK (df_train.h).
__global__ __launch_bounds__(kOptThreads) void tensor_sumsq_kernel(const float* g, const float* x,
                                                                   const int32_t* toff, OptChain ch, int n_pre,
                                                                   int need_x, int take_sqrt, float* out) {
#pragma clang fp contract(off)
    typedef float v4 __attribute__((ext_vector_type(4)));
    __shared__ float red[kOptThreads];
    const int t = blockIdx.x;
    const int64_t base = toff[t];
    const int n = toff[t + 1] - toff[t];
    const float* gt = g + base;
    const float* xt = x + base;
    const bool vec = (base & 3) == 0;  // (g and x are hipMalloc allocations)
    const int nq = (n + 3) / 4;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = threadIdx.x; q < nq; q += kOptThreads) {
        const int j = 4 * q;
        float d[4], xv[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && j + 4 <= n) {
            const v4 gq = *reinterpret_cast<const v4*>(gt + j);
            d[0] = gq.x, d[1] = gq.y, d[2] = gq.z, d[3] = gq.w;
            if (need_x) {
                const v4 xq = *reinterpret_cast<const v4*>(xt + j);
                xv[0] = xq.x, xv[1] = xq.y, xv[2] = xq.z, xv[3] = xq.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = j + c < n;
                d[c] = in ? gt[j + c] : 0.f;
                if (need_x) xv[c] = in ? xt[j + c] : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // (past the tensor's end: dx = 0, which adds +0 and leaves the sum as it is)
            const float dx = j + c < n ? opt_pre_rules(ch, n_pre, d[c], xv[c]) : 0.f;
            const float sq = dx * dx;
            a[c] = a[c] + sq;
        }
    }
    red[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    for (int s = kOptThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[t] = take_sqrt ? sqrtf(red[0]) : red[0];
}

// The whole chain on one element, then x -= dx.  Adam is adam_kernel's arithmetic on the
// incoming dx; ClipNorm's scale comes from sumsq[tensor] (tensor_sumsq_kernel).
__global__ __launch_bounds__(kOptThreads) void opt_chain_kernel(float* x, const float* g, float* m, float* v,
                                                                const float* bt, const float* sumsq,
                                                                const OptBlock* blocks, OptChain ch) {
#pragma clang fp contract(off)
    const OptBlock b = blocks[blockIdx.x];
    if ((int)threadIdx.x >= b.count) return;
    const int64_t i = (int64_t)b.begin + threadIdx.x;
    const float xi = x[i];
    float dx = g[i];
#pragma unroll
    for (int r = 0; r < kOptMaxRules; ++r) {
        if (r >= ch.n) break;
        const float p0 = ch.p[r][0];
        switch (ch.kind[r]) {
            case DF_OPT_CLIP_GRAD: dx = opt_clip_grad(dx, p0); break;
            case DF_OPT_WEIGHT_DECAY: dx = opt_weight_decay(dx, xi, p0); break;
            case DF_OPT_DESCENT: dx = p0 * dx; break;
            case DF_OPT_CLIP_NORM: {
                const float nrm = sqrtf(sumsq[b.tensor]);
                if (nrm > p0) {
                    const float scale = p0 / nrm;
                    dx = dx * scale;
                }
                break;
            }
            case DF_OPT_ADAM: {
                const float b1 = ch.p[r][1], b2 = ch.p[r][2], eps = ch.p[r][3];
                const float bt1 = bt[0], bt2 = bt[1];
                const float mi = b1 * m[i] + (1.f - b1) * dx;
                const float vi = b2 * v[i] + (1.f - b2) * (dx * dx);
                m[i] = mi;
                v[i] = vi;
                dx = mi / (1.f - bt1) / (sqrtf(vi / (1.f - bt2)) + eps) * p0;
                break;
            }
            default: break;
        }
    }
    x[i] = xi - dx;
}

__global__ void repack_kernel(float* blob, const int32_t* dst, const int32_t* src, int64_t count,
                              const float* params) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) blob[dst[i]] = params[src[i]];
}

__global__ void repack_split_kernel(uint8_t* blob, const int32_t* dst, const int32_t* src, int64_t count,
                                    const float* params) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t code = src[i];
    const float v = params[code >> 2];
    const int plane = code & 3;
    if (plane == 3) *reinterpret_cast<float*>(blob + dst[i]) = v;
    else *reinterpret_cast<uint16_t*>(blob + dst[i]) = bf16_split_plane(v, plane);
}

unsigned blocks_for(int64_t count, int threads) { return (unsigned)((count + threads - 1) / threads); }

}  // namespace

size_t train_net_lds(int ht, const GNet& g) {
    const size_t tarea = (size_t)kTrainWaves * 2 * 16 * ht * kTS * 4;
    // the reduction: the net's trainables + dW0 / dW1 / dW_out in padded regions
    // (train_net_kernel; generous bounds: n_in, n_out <= 16, dW1 rows <= h + 8 apart)
    const size_t h = (size_t)g.h_true;
    const size_t red = (((size_t)g.p_count + 3) + (h + 1) * 16 + 3 + h * (h + 8) + 3 + 17 * h) * 4;
    if (g.split) return (size_t)g.sfwd_bytes + ht * 1024 + g.st_bytes + (tarea > red ? tarea : red);
    return (size_t)g.fwd_bytes + g.t_bytes + (tarea > red ? tarea : red);
}

hipError_t set_train_lds_limit(size_t lds) {
    for (bool wt : {false, true}) {
        for (int ht : {1, 2, 4})
            for (int nh = 0; nh < 2; ++nh)
                for (int am = 0; am < 3; ++am) {
                    hipError_t e = hipFuncSetAttribute(train_ptr(ht, nh, am, false, 0, wt),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                    if (e != hipSuccess) return e;
                }
        for (int ht : {2, 4}) {
            for (int naf : {0, 2, 3}) {
                hipError_t e = hipFuncSetAttribute(train_ptr(ht, 1, trn::AM_RELU, true, naf, wt),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return e;
            }
        }
    }
    return hipSuccess;
}

hipError_t launch_train_net(int ht, int nh, int am, const TrainArgs& a, unsigned grid, size_t lds,
                            hipStream_t st) {
    // out_valu<NO = NAF> needs n_out = n_af, the 4x4x1 x̄ at most 4 conditioner inputs
    const int naf = (a.net.split && a.net.su.n_out == a.n_af && a.net.n_in <= 4) ? a.n_af : 0;
    void* k = train_ptr(ht, nh, am, a.net.split != 0, naf, a.wj != nullptr);
    if (!k) return hipErrorInvalidValue;
    void* args[] = {const_cast<TrainArgs*>(&a)};
    return hipLaunchKernel(k, dim3(grid), dim3(train_threads(a.net.split != 0)), args, lds, st);
}

hipError_t train_net_occupancy(int ht, int nh, int am, size_t lds, int* blocks, bool split) {
    void* k = train_ptr(ht, nh, am, split);
    if (!k) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k, train_threads(split), lds);
}

hipError_t launch_scale(float* dst, const float* src, float s, int64_t count, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, dst, src, s, count);
    return hipGetLastError();
}

hipError_t launch_scale_rows(float* dst, const float* src, const float* wj, int d, int64_t batch, hipStream_t st) {
    const int64_t count = batch * d;
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, dst, src, wj, d, count);
    return hipGetLastError();
}

hipError_t launch_weight_norm(const float* w, int64_t batch, double w_total, double* part, float* wj, double* wsums,
                              hipStream_t st) {
    const int64_t nb = wsum_parts(batch);
    if (nb <= 0) return hipSuccess;
    const bool own = !(w_total > 0.0);
    if (own && nb > 1)
        hipLaunchKernelGGL(wsum_partial_kernel, dim3((unsigned)nb), dim3(kWsumThreads), 0, st, w,
                           static_cast<const float*>(nullptr), batch, part);
    hipLaunchKernelGGL(weight_norm_kernel, dim3((unsigned)nb), dim3(kWsumThreads), 0, st, w, batch, w_total,
                       static_cast<const double*>(part), nb, wj, wsums);
    return hipGetLastError();
}

hipError_t launch_weighted_lp_sum(const float* w, const float* lp, int64_t batch, double* part, double* out,
                                  hipStream_t st) {
    const int64_t nb = wsum_parts(batch);
    if (nb <= 0) return hipMemsetAsync(out, 0, sizeof(double), st);
    hipLaunchKernelGGL(wsum_partial_kernel, dim3((unsigned)nb), dim3(kWsumThreads), 0, st, w, lp, batch,
                       nb == 1 ? out : part);
    if (nb > 1)
        hipLaunchKernelGGL(wsum_final_kernel, dim3(1), dim3(kWsumThreads), 0, st, static_cast<const double*>(part), nb,
                           out);
    return hipGetLastError();
}

hipError_t launch_norm_adjoint(float* zbar, const float* xmin, const float* xmax, float alpha, float beta, int d,
                               int64_t batch, hipStream_t st) {
    const int64_t count = batch * d;
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(norm_adjoint_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, zbar, xmin, xmax,
                       alpha, beta, d, count);
    return hipGetLastError();
}

hipError_t launch_reduce_grads(const float* partial, int n_parts, int64_t p_total, float* grad, hipStream_t st) {
    if (p_total <= 0) return hipSuccess;
    if (p_total % 4 == 0 && (reinterpret_cast<uintptr_t>(partial) % 16) == 0 && (reinterpret_cast<uintptr_t>(grad) % 16) == 0)
        hipLaunchKernelGGL(reduce_grads4_kernel, dim3(blocks_for(p_total / 4, 256)), dim3(256), 0, st, partial,
                           n_parts, p_total, grad);
    else
        hipLaunchKernelGGL(reduce_grads_kernel, dim3(blocks_for(p_total, 256)), dim3(256), 0, st, partial, n_parts,
                           p_total, grad);
    return hipGetLastError();
}

hipError_t launch_adam(float* x, const float* g, float* m, float* v, int64_t count, float eta, float b1, float b2,
                       float eps, float* bt, hipStream_t st) {
    if (count > 0)
        hipLaunchKernelGGL(adam_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, x, g, m, v, count, eta, b1, b2,
                           eps, static_cast<const float*>(bt));
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, st, bt, b1, b2);
    return hipGetLastError();
}

hipError_t launch_tensor_sumsq(const float* g, const float* x, const int32_t* toff, int n_tensors, const OptChain& ch,
                               int n_pre, bool take_sqrt, float* out, hipStream_t st) {
    if (n_tensors <= 0) return hipSuccess;
    int need_x = 0;
    for (int r = 0; r < n_pre; ++r) need_x |= ch.kind[r] == DF_OPT_WEIGHT_DECAY;
    hipLaunchKernelGGL(tensor_sumsq_kernel, dim3((unsigned)n_tensors), dim3(kOptThreads), 0, st, g, x, toff, ch, n_pre,
                       need_x, take_sqrt ? 1 : 0, out);
    return hipGetLastError();
}

hipError_t launch_opt_chain(float* x, const float* g, float* m, float* v, float* bt, const float* sumsq,
                            const OptBlock* blocks, int64_t n_blocks, const OptChain& ch, hipStream_t st) {
    if (n_blocks > 0)
        hipLaunchKernelGGL(opt_chain_kernel, dim3((unsigned)n_blocks), dim3(kOptThreads), 0, st, x, g, m, v,
                           static_cast<const float*>(bt), sumsq, blocks, ch);
    for (int r = 0; r < ch.n; ++r)
        if (ch.kind[r] == DF_OPT_ADAM)
            hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, st, bt, ch.p[r][1], ch.p[r][2]);
    return hipGetLastError();
}

hipError_t launch_repack(float* blob, const int32_t* dst, const int32_t* src, int64_t count, const float* params,
                         hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(repack_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, blob, dst, src, count, params);
    return hipGetLastError();
}

hipError_t launch_repack_split(uint8_t* blob, const int32_t* dst, const int32_t* src, int64_t count,
                               const float* params, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(repack_split_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, blob, dst, src, count,
                       params);
    return hipGetLastError();
}

}  // namespace df
