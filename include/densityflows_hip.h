/*
 * densityflows_hip.h — C ABI of the MI355X-native DensityFlows.jl hot path.
 *
 * The library (libdensityflows_hip.so, built for gfx950) evaluates a
 * DensityFlows.jl `FlowChain` of RealNVP / NICE coupling layers, coupling
 * blocks and NormalizationLayers over a batch of samples with fused HIP
 * kernels: the s/t conditioner MLPs run on f32 MFMA, the coupling transform,
 * the per-layer log-det-Jacobian (ldj) accumulation and the base-density
 * logpdf are fused behind them.
 *
 * Every entry point below replaces one Julia method of the reference
 * (DensityFlows.jl v1.0.0).  A Julia front-end binds them with `ccall`
 * (see INTEGRATION.md and densityflows.jl_amd/julia/DensityFlowsHIP.jl);
 * the Python host mirror binds them with ctypes.
 *
 * Conventions
 * -----------
 *  - Memory layout is exactly Julia's: a (d, B) Float32 matrix is
 *    column-major, so sample j occupies x[d*j .. d*j+d-1].  θ is (n, B), may
 *    be n = 0 (pointer may then be NULL).  ldj / logpdf are (B,).
 *  - Dense weights are Flux's `Dense.weight`: an (out, in) column-major
 *    Float32 matrix (W[i + out*k] = W_ik); `bias` has `out` entries or is
 *    NULL (`bias=false`).  Axes are Julia's 1-based index vectors.
 *  - Batch-compute calls take DEVICE pointers and a HIP stream (NULL = the
 *    default stream) and are stream-ordered (asynchronous w.r.t. the host).
 *  - All functions return DF_OK (0) or a negative df_status; the message of
 *    the last error on the calling thread is returned by df_last_error().
 *  - A df_chain handle is bound to one device and is not thread-safe;
 *    different handles may be used concurrently.
 */
#ifndef DENSITYFLOWS_HIP_H
#define DENSITYFLOWS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DF_ABI_VERSION 5

typedef enum df_status {
    DF_OK = 0,
    DF_ERR_INVALID = -1,     /* malformed descriptor / argument (Julia: ArgumentError) */
    DF_ERR_SHAPE = -2,       /* shape or rank mismatch (Julia: AssertionError / DimensionMismatch) */
    DF_ERR_HIP = -3,         /* HIP runtime error */
    DF_ERR_UNSUPPORTED = -4, /* structure outside the kernel's limits (see df_limits) */
    DF_ERR_NOMEM = -5,       /* device allocation failed */
    DF_ERR_NONFINITE = -6    /* a NaN/Inf was found where the caller asked for a check */
} df_status;

/* Activation functions σ of Flux.Dense (NNlib definitions). */
typedef enum df_act {
    DF_ACT_IDENTITY = 0,
    DF_ACT_RELU = 1,
    DF_ACT_TANH = 2,
    DF_ACT_SIGMOID = 3,
    DF_ACT_SOFTPLUS = 4,
    DF_ACT_LOGCOSH = 5,
    DF_ACT_LEAKYRELU = 6,  /* slope 0.01 */
    DF_ACT_ELU = 7,        /* α = 1 */
    DF_ACT_SWISH = 8
} df_act;

/* FlowElement kinds that the kernels evaluate. */
typedef enum df_layer_kind {
    DF_LAYER_RNVP = 0, /* RNVPCouplingLayer  (src/affine/RNVP.jl:41-48)          */
    DF_LAYER_NICE = 1, /* NICECouplingLayer  (src/affine/NICE.jl:31-36)          */
    DF_LAYER_NORM = 2  /* NormalizationLayer (src/norm/Normalization.jl:30-35)   */
} df_layer_kind;

/* One Flux.Dense(in, out, σ; bias).  src/Layers.jl:33-50. */
typedef struct df_dense_desc {
    int32_t in_dim;
    int32_t out_dim;
    int32_t act;        /* df_act */
    const float* W;     /* (out, in) column-major, host memory */
    const float* b;     /* out entries, or NULL for bias=false */
} df_dense_desc;

/* One flat layer of the chain.  CouplingBlocks (src/Blocks.jl:64-75) are
 * given as two consecutive layers with the same `element` index; the chain's
 * ldj is then accumulated exactly as the reference groups it:
 *   element ldj = ldj_1 .+ ldj_2            (src/Blocks.jl:136,149)
 *   chain ldj   = ldj_e1 .+ ldj_e2 .+ ...   (src/Chains.jl:160,179)          */
typedef struct df_layer_desc {
    int32_t kind;       /* df_layer_kind */
    int32_t element;    /* index of the FlowElement this layer belongs to */
    /* coupling layers: CouplingAxes (src/Axes.jl:28-35), 1-based */
    int32_t n_af;
    const int32_t* axis_af;  /* transformed dims, user (mask) order      */
    int32_t n_nn;
    const int32_t* axis_nn;  /* conditioner input rows of vcat(θ, z)     */
    int32_t n_dense_s;       /* 0 for NICE */
    const df_dense_desc* s_net;
    int32_t n_dense_t;
    const df_dense_desc* t_net;
    /* NormalizationLayer fields */
    const float* x_min;      /* d entries */
    const float* x_max;      /* d entries */
    float alpha;
    float beta;
} df_layer_desc;

typedef struct df_chain_desc {
    int32_t abi_version;     /* DF_ABI_VERSION */
    int32_t d;               /* data dimensions */
    int32_t n;               /* condition dimensions (0 = unconditional) */
    int32_t n_layers;
    const df_layer_desc* layers;
} df_chain_desc;

/* Structural limits of the fused kernels. */
typedef struct df_limits {
    int32_t max_state;       /* n + d                      */
    int32_t max_hidden;      /* widest hidden Dense        */
    int32_t max_af;          /* transformed dims per layer */
    int32_t max_layers;
} df_limits;

typedef struct df_chain_info {
    int32_t d, n, n_layers;
    int32_t hidden_tiles;         /* kernel variant: padded hidden width / 16 */
    int32_t samples_per_block;    /* samples one workgroup processes          */
    int32_t n_stages;             /* LDS weight stages per chain pass         */
    int64_t n_params;             /* trainable parameters (Flux.trainables)   */
    double flops_per_sample;      /* 2 × Σ Dense MACs (algorithmic)           */
    int64_t weight_bytes;         /* packed device weight blob                */
    int32_t kernel;               /* chain-pass kernel: 0 generic, 1 specialised,
                                     2 specialised relu-only, 3 FAST, 4 FAST on
                                     bf16x3 split stages (SPLIT), 5 wide,
                                     6 wide SPLIT                              */
    int32_t reserved;
    double split_flops_per_sample; /* part of flops_per_sample that kernels 4
                                      and 6 run as six bf16 products on MFMA */
} df_chain_info;

int df_get_abi_version(void);
const char* df_last_error(void);
int df_get_limits(df_limits* out);

/* ---- chain lifetime ------------------------------------------------------ */

typedef struct df_chain df_chain;

/* Validate and plan a descriptor without touching a device (the same checks
 * df_chain_create performs); fills `info` when non-NULL. */
int df_chain_validate(const df_chain_desc* desc, df_chain_info* info);

/* Build a device-resident chain (weights are copied and re-laid-out into MFMA
 * fragment order).  Replaces the Julia-side `FlowChain` object
 * (src/Chains.jl:78-80) for evaluation.  `device` = HIP device ordinal. */
int df_chain_create(df_chain** out, const df_chain_desc* desc, int device);
int df_chain_destroy(df_chain* chain);
int df_chain_get_info(const df_chain* chain, df_chain_info* out);

/* Replace the chain's parameters (Dense weights and biases, NormalizationLayer
 * bounds) with those of `desc`, which must describe the same structure (same
 * layers, axes, widths, activations and bias flags) — e.g. the model after
 * Optimisers.update! on the host, or one read by load_flow
 * (src/Loading.jl:324-376).  Synchronous.  Not allowed while df_train handles
 * are bound to the chain (they own the parameters: df_train_set_params). */
int df_chain_set_weights(df_chain* chain, const df_chain_desc* desc);

/* θ bounds of the Flow's MetaData (src/Data.jl:75-86; n floats each, host
 * memory).  Enables the df_flow_* entry points' in-kernel θ normalisation. */
int df_chain_set_theta_bounds(df_chain* chain, const float* theta_min, const float* theta_max);

/* ---- chain level (θ used as given) ---------------------------------------
 * forward(chain, z, θ)  -> (x, ldj)      src/Chains.jl:168-184
 * backward(chain, x, θ) -> (z, ldj)      src/Chains.jl:149-165
 * forward!(chain, z, θ)                  src/Chains.jl:187-197  (in place, no ldj)
 * `ldj` may be NULL (not written).  `x_out` may alias `z` for forward. */
int df_chain_forward(df_chain* chain, const float* z, const float* theta,
                     float* x_out, float* ldj_out, int64_t batch, void* stream);
int df_chain_backward(df_chain* chain, const float* x, const float* theta,
                      float* z_out, float* ldj_out, int64_t batch, void* stream);
int df_chain_forward_inplace(df_chain* chain, float* z, const float* theta,
                             int64_t batch, void* stream);

/* df_chain_logpdf / df_chain_logpdf_sum: the same quantities as df_flow_logpdf /
 * df_flow_logpdf_sum below with θ used as given — logpdf / loss of the MODEL,
 * as train! evaluates them on normalized_training_data (src/Flows.jl:391-392,
 * 419-430): backward(flow.model, x, t) then the MvNormal(0, I) log-density.
 * Independent of the chain's θ bounds. */
int df_chain_logpdf(df_chain* chain, const float* x, const float* theta,
                    float* logpdf_out, int64_t batch, void* stream);
int df_chain_logpdf_sum(df_chain* chain, const float* x, const float* theta,
                        double* sum_out, int64_t batch, void* stream);

/* ---- flow level (θ raw, normalised in-kernel with the stored bounds) -----
 * The @flow_wrapper methods (src/Macros.jl:104-112, applied at
 * src/DensityFlows.jl:72): f(flow, y, θ) = f(flow.model, y, normalize_input(θ)).
 * df_flow_logpdf: src/Flows.jl:272-281 — backward pass + MvNormal(0, I)
 * log-density + ldj, written per sample.
 * df_flow_logpdf_sum: Σ_j logpdf_j accumulated in fp64, deterministic
 * order, written to ONE double in device memory (the NLL partial that
 * src/Flows.jl:352-359 averages; all-reduced across GPUs by the caller). */
int df_flow_forward(df_chain* chain, const float* z, const float* theta_raw,
                    float* x_out, float* ldj_out, int64_t batch, void* stream);
int df_flow_backward(df_chain* chain, const float* x, const float* theta_raw,
                     float* z_out, float* ldj_out, int64_t batch, void* stream);
int df_flow_forward_inplace(df_chain* chain, float* z, const float* theta_raw,
                            int64_t batch, void* stream);
int df_flow_logpdf(df_chain* chain, const float* x, const float* theta_raw,
                   float* logpdf_out, int64_t batch, void* stream);
int df_flow_logpdf_sum(df_chain* chain, const float* x, const float* theta_raw,
                       double* sum_out, int64_t batch, void* stream);

/* ---- sampling ---------------------------------------------------------------
 * sample(flow, dims, θ) (src/Flows.jl:157-192): r ~ MvNormal(0, I) (Flows.jl:114)
 * drawn on the device, then forward!(flow, r, θ) — df_flow_forward_inplace, θ raw and
 * normalised in the kernel with the chain's bounds.  x_out: (d, batch) device memory;
 * for dims = (d1, d2, ...) pass batch = prod(dims) (the column-major (d, dims...) array
 * is the (d, batch) one).  theta_broadcast = 0: theta_raw is (n, batch); 1: theta_raw
 * is ONE n-vector used for every sample (the NTuple θ method, Flows.jl:178-188).
 * The draw: element k of the (d, batch) array comes from Philox4x32-10 with key =
 * seed and counter (offset + k/4, 0, 0, 0), word k%4; words (0,1), (2,3) are
 * Box-Muller pairs.  Julia's Xoshiro stream is not reproduced (by design);
 * df_random_normal returns the same draw on its own, so a caller can check
 * forward!(draw) against df_flow_sample with the same (seed, offset). */
int df_flow_sample(df_chain* chain, float* x_out, const float* theta_raw, int theta_broadcast, int64_t batch,
                   uint64_t seed, uint64_t offset, void* stream);
int df_random_normal(float* out, int64_t count, uint64_t seed, uint64_t offset, void* stream);

/* ---- sampling with the density, and its moments (additive to ABI 5) -------------
 * df_flow_sample_logpdf: x ~ q(. | θ) together with log q(x | θ), for importance weights,
 * evidence estimates and entropies, at the cost of ONE forward pass per sample (sample then
 * logpdf costs a forward and a full inverse pass).  Stream, θ handling (raw θ, bounds
 * required when n > 0, theta_broadcast through the chain's θ workspace) and errors are
 * df_flow_sample's.  With z the (d, batch) draw df_random_normal(seed, offset) returns:
 *   x_out (d, batch)   bitwise what df_flow_forward(z, θ) returns.  df_flow_sample runs
 *                      forward! instead; whether the two agree bit for bit is a property of
 *                      the chain-pass kernels that nothing here promises.
 *   logpdf_out[j]      = -(d·log(2π) + Σ_k z_kj²)/2 - ldj_j  with ldj bitwise
 *                      df_flow_forward's, every operation one Float32 operation in this order:
 *                        s = z_0j·z_0j;  s = s + z_kj·z_kj  for k = 1 .. d-1;
 *                        b = -((float)d·(float)log(2π) + s) / 2;   logpdf_out[j] = b - ldj_j
 * Three launches behind the draw: b into logpdf_out, df_flow_forward in place in x_out with
 * the ldj into a workspace of max(batch, 1024) floats that belongs to the chain and only
 * grows (growing it inside a stream capture is DF_ERR_INVALID), then the subtraction.  No
 * host synchronisation; capturable once the workspaces are warm.
 * logpdf_out == NULL: the draw and df_flow_forward alone.  batch == 0: DF_OK, nothing runs. */
int df_flow_sample_logpdf(df_chain* chain, float* x_out, float* logpdf_out, const float* theta_raw,
                          int theta_broadcast, int64_t batch, uint64_t seed, uint64_t offset, void* stream);
/* The moment block of the calls below: 3 + m + m² doubles in DEVICE memory,
 *   out[0]          = the number of samples, as a double
 *   out[1], out[2]  = Σ_j lp_j,  Σ_j lp_j²
 *   out[3 .. 3+m)   = Σ_j g_aj
 *   out[3+m .. )    = Σ_j g_aj·g_bj, the full m × m matrix, column-major; both triangles
 *                     hold the same bits
 * of per-sample Float32 values lp_j and g_aj converted to double; products and sums are in
 * double.  The sums are reduced WITHOUT atomics in a fixed order (two runs give the same
 * bits): workgroup b of G sums a contiguous range of samples — thread i of 256 its samples
 * i, i + 256, ... of the range in increasing order, the threads by a fixed tree — and the G
 * partial blocks are then added in workgroup order.  G follows from the batch and the
 * device (the chain's grid), so blocks of different batch sizes or devices differ in the
 * last bits.  A non-finite value propagates into the entries it touches.  The partial
 * blocks live in a workspace of the calling handle that only grows.
 *
 * df_flow_sample_logpdf_moments: m = 0, lp_j = log q(x_j | θ) of n_samples draws at ONE raw
 * θ (a device n-vector; NULL for n = 0), every chain class: the entropy H = -out[1]/out[0]
 * and its standard error from one forward pass per sample.  Sample s is sample s of
 * df_flow_sample_logpdf(batch = n_samples, theta_broadcast = 1, seed, offset).  The call
 * proceeds `chunk` samples at a time (0: 2^20; rounded up to a multiple of 4, a Philox
 * counter boundary; at most 2^24): chunk i, starting at sample start_i, is
 * df_flow_sample_logpdf at offset + d·start_i/4 into chain-owned workspaces (x, lp; they
 * only grow, not inside a capture) and its block c_i is added to out3, which is zeroed on the
 * stream first: out3 = ((0 + c_1) + c_2) + ...  No host synchronisation.
 * n_samples == 0: DF_OK, out3 zeroed.  DF_ERR_INVALID: a null chain or out3, bounds not set
 * (n > 0); DF_ERR_SHAPE: n_samples or chunk < 0, θ missing; DF_ERR_UNSUPPORTED: chunk > 2^24. */
int df_flow_sample_logpdf_moments(df_chain* chain, const float* theta_raw, int64_t n_samples, int64_t chunk,
                                  uint64_t seed, uint64_t offset, double* out3, void* stream);

/* ---- calibration: HPD ranks of points under the flow (additive to ABI 5) ---------
 * df_flow_hpd_ranks: the expected-coverage test of a conditional density, every chain class.
 * For each of n_points held-out pairs (x_i, θ_i) the call draws n_draws samples of q(. | θ_i)
 * and counts those with a higher density than x_i; rank_i / n_draws is the point's credibility
 * level, uniform on [0, 1] for a calibrated flow.  All pointers are DEVICE memory.
 *   x (d, n_points), theta_raw (n, n_points) raw θ (NULL for n = 0; bounds required as for
 *   df_flow_sample).
 *   rank_out[i]  (int32) = #{k < n_draws : lp_ik > lp_i}, a Float32 IEEE comparison: a NaN on
 *                either side counts nothing; lp_i = -inf is below every finite draw.
 *   lp_i         what df_flow_logpdf(x, theta_raw, batch = n_points) returns for point i (one
 *                inverse pass over all points, before the first chunk); written to logpdf_out
 *                when that is not NULL, otherwise to a workspace of the chain.
 *   lp_ik        log q of draw k of point i; written to draws_logpdf_out[i·n_draws + k] when
 *                that is not NULL (n_points · n_draws floats).
 * Which draw is which: draw k of point i is sample j = i·n_draws + k of
 * df_flow_sample_logpdf(batch = n_points·n_draws, theta_broadcast = 0, θ_j = θ_i, seed,
 * offset), and lp_ik is bitwise that call's logpdf_out[j] wherever both run the same chain-pass
 * kernel family: the same base term, the same df_flow_forward ldj and the same single Float32
 * subtraction.  n_draws must be a positive multiple of 4 (a Philox counter boundary), so point
 * i's draws start at counter offset + d·i·n_draws/4 and depend neither on the other points nor
 * on the chunking.
 * The call proceeds by whole points, G = max(1, chunk / n_draws) points at a time (chunk in
 * samples; 0: 2^20; at most 2^24).  Per chunk: the draw, θ row i repeated over its draws, the
 * base term, df_flow_forward in place with the ldj into a workspace, and one count kernel
 * (wave64 ballots and population counts, the waves of a workgroup added through LDS in wave
 * order, one store per point, no atomics).  The workspaces (x draws, repeated θ, base term,
 * ldj, the points' lp) belong to the chain and only grow; growing one inside a stream capture
 * is DF_ERR_INVALID.  No host synchronisation; capturable once the workspaces are warm.
 * n_points == 0: DF_OK, nothing runs, nothing is written.
 * DF_ERR_INVALID: a null chain, x or rank_out; n_draws not a positive multiple of 4; bounds
 * not set (n > 0).  DF_ERR_SHAPE: n_points or chunk < 0, θ missing, n_points·n_draws past
 * int64.  DF_ERR_UNSUPPORTED: chunk > 2^24, n_draws > 2^24. */
int df_flow_hpd_ranks(df_chain* chain, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                      int64_t chunk, uint64_t seed, uint64_t offset, int32_t* rank_out, float* logpdf_out,
                      float* draws_logpdf_out, void* stream);

/* ---- posterior summaries: SBC ranks, shifted sums per point (additive to ABI 5) ----
 * df_flow_point_stats: the samples of q(. | θ_i) reduced per point, every chain class.  For each
 * of n_points pairs (x_i, θ_i) the call draws n_draws samples and returns, per dimension k < d,
 * the simulation-based-calibration rank of x_i[k] among them, and the sums behind the posterior
 * mean and covariance.  All pointers are DEVICE memory, sample j at ptr + d·j.
 *   x (d, n_points) the points, needed with rank_out only (NULL otherwise); theta_raw
 *   (n, n_points) raw θ (NULL for n = 0; bounds required as for df_flow_sample).
 *   rank_out[i·d + k] (int32) = #{j < n_draws : draw_ij[k] < x_i[k]}, a Float32 IEEE
 *                comparison: a tie counts nothing, a NaN on either side counts nothing.
 *                Uniform on {0 .. n_draws} for a calibrated flow.
 *   sums_out     n_points blocks of S = 2d + d(d+1)/2 doubles.  Block i:
 *                  c[k], k < d                 the shift: draw 0 of point i, as a double
 *                  S1[k] at d + k              Σ_j (draw_ij[k] − c[k])
 *                  S2[a, b] at 2d + a(a+1)/2 + b, a >= b
 *                                              Σ_j (draw_ij[a] − c[a])·(draw_ij[b] − c[b])
 *                every value converted to double before the subtraction; the products are
 *                fused into the running sum (one rounding per term).  mean = c + S1/N,
 *                cov = (S2 − S1 S1ᵀ/N)/(N − 1).  A NaN draw makes the sums it touches NaN, a
 *                NaN in draw 0 every entry of its dimension; nothing is checked.
 *   draws_out    (d, n_points·n_draws), when not NULL: the samples themselves, copied
 *                device-to-device chunk by chunk; any 4-byte aligned pointer.
 * At least one of the three outputs is given; the others may be NULL, and what is not asked for
 * is not computed (ranks alone read no pair, sums alone read no point).
 * Which draw is which: draw k of point i is sample j = i·n_draws + k of df_flow_sample(batch =
 * n_points·n_draws, theta_broadcast = 0, θ_j = θ_i, seed, offset), bitwise wherever both run the
 * same chain-pass kernel family, and its base normal is the one df_flow_hpd_ranks uses at the
 * same (seed, offset).  n_draws must be a positive multiple of 4 (a Philox counter boundary):
 * point i's draws start at counter offset + d·i·n_draws/4.
 * The call proceeds by whole points, G = max(1, chunk / n_draws) points at a time (chunk in
 * samples; 0: 2^20; at most 2^24).  Per chunk: the draw, θ row i repeated over its draws,
 * df_flow_forward_inplace, and one reduction kernel.  The counts are exact.  Every fp64 sum is
 * added in an order fixed by (d, n_draws) alone (tiles of 64 draws; df_pstats.hip states it),
 * without atomics: two calls give the same bytes, whatever the chunk, the other points or the
 * device's size, and so does point i computed alone at offset + d·i·n_draws/4 (within one
 * chain-pass kernel family).
 * The workspaces (x draws, repeated θ) are df_flow_hpd_ranks' own: they belong to the chain and
 * only grow; growing one inside a stream capture is DF_ERR_INVALID.  No host synchronisation;
 * capturable once the workspaces are warm.
 * n_points == 0: DF_OK, nothing runs, nothing is written.
 * DF_ERR_INVALID: a null chain; n_draws not a positive multiple of 4 (it is not rounded); all
 * three outputs NULL; rank_out without x; bounds not set (n > 0).  DF_ERR_SHAPE: n_points or
 * chunk < 0, θ missing, n_points·n_draws past int64.  DF_ERR_UNSUPPORTED: chunk > 2^24,
 * n_draws > 2^24. */
int df_flow_point_stats(df_chain* chain, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                        int64_t chunk, uint64_t seed, uint64_t offset, int32_t* rank_out, double* sums_out,
                        float* draws_out, void* stream);

/* ---- posterior quantiles: order statistics per point and dimension (additive to ABI 5) ----
 * The order on Float32 is IEEE totalOrder: key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000),
 * compared as uint32: −NaN < −inf < ... < −0 < +0 < ... < +inf < +NaN.  The order statistic r
 * (0-based, 0 <= r < n_draws) of dimension k of a point is the draw whose key is the r-th
 * smallest among the point's n_draws draws of that dimension, returned with its own bits; ties
 * hold equal keys and hence equal bits.  Nothing is interpolated on the device: a quantile
 * between two draws is the caller's lo + (hi − lo)·g from two order statistics.
 *
 * df_order_statistics: the selection alone, on the current device (as df_random_normal).
 *   xs (d, n_points·n_draws) DEVICE, 16-byte aligned, draw j of point i at xs + d·(i·n_draws + j);
 *   orders: HOST array of n_orders int32, each in [0, n_draws), in any order, repeats allowed;
 *           read at call time and passed to the kernel by value: no copy, no synchronisation,
 *           capturable;
 *   out[(i·d + k)·n_orders + q] (DEVICE) = order statistic orders[q] of dimension k of point i.
 * One radix-select kernel (df_quant.hip: 8-bit digits, 4 passes over a point's draws, integer
 * counts in LDS, a wave per point up to n_draws = 256 and a workgroup per point above; what does
 * not fit the LDS at once is walked in groups of dimensions).  One store per (point, dimension,
 * order); nothing is zeroed, no global atomics: two calls give the same bytes.
 * Checked in this order before any device work: 1 <= d <= 64 (DF_ERR_INVALID); n_points < 0
 * (DF_ERR_SHAPE); n_draws a positive multiple of 4 (DF_ERR_INVALID) and at most 2^24
 * (DF_ERR_UNSUPPORTED); xs and out non-null, xs 16-byte aligned (DF_ERR_INVALID); orders
 * non-null (DF_ERR_INVALID), 1 <= n_orders <= DF_QUANT_MAX_ORDERS (DF_ERR_UNSUPPORTED), every
 * order in [0, n_draws) (DF_ERR_INVALID, the message names the index).  Then n_points == 0:
 * DF_OK, nothing launched, nothing written.
 *
 * df_flow_point_quantiles: df_flow_point_stats with the selection at the end of every chunk.
 * The draws, the θ repeat, the chunking by whole points, the workspaces, the counters
 * (offset + d·i·n_draws/4) and the rules and messages for the chain, n_points, n_draws, chunk,
 * θ and the bounds are df_flow_point_stats': draw j of point i is bitwise the draw that call
 * makes at the same (seed, offset).  quant_out is as `out` above.  rank_out (needs x), sums_out
 * and draws_out are optional and bitwise what df_flow_point_stats writes (the same kernel and
 * the same copy, on the chunk the selection reads).  At least one of the four outputs is given;
 * quant_out needs orders and 1 <= n_orders <= DF_QUANT_MAX_ORDERS, checked as above after the
 * outputs; with quant_out NULL, orders and n_orders are ignored.  The workspaces are
 * df_flow_hpd_ranks' and df_flow_point_stats': calls on different streams must not overlap.
 * No host synchronisation; capturable once the workspaces are warm.  n_points == 0: DF_OK,
 * nothing runs, nothing is written (the argument rules still hold). */
#define DF_QUANT_MAX_ORDERS 32

int df_order_statistics(const float* xs, int d, int64_t n_points, int64_t n_draws, const int32_t* orders,
                        int n_orders, float* out, void* stream);

int df_flow_point_quantiles(df_chain* chain, const float* x, const float* theta_raw, int64_t n_points,
                            int64_t n_draws, int64_t chunk, uint64_t seed, uint64_t offset, const int32_t* orders,
                            int n_orders, float* quant_out, int32_t* rank_out, double* sums_out, float* draws_out,
                            void* stream);

/* ---- posterior histograms: 1-D and 2-D marginal counts per point (additive to ABI 5) ----
 * The corner plot of q(. | θ_i) from its draws: integer counts, exact and bitwise reproducible
 * however the work is split (no floating-point atomic anywhere).
 *
 * df_draw_histograms: the counting alone, on the current device (as df_order_statistics).
 *   xs (d, n_points·n_draws) DEVICE, 16-byte aligned, draw j of point i at xs + d·(i·n_draws + j);
 *   bins: HOST, d int32; bins[k] = L_k bins of dimension k, 0: no edges, no table may keep it;
 *   edges: DEVICE Float32, the L_k + 1 edges of every dimension with L_k > 0, one after the
 *          other in dimension order.  The call does not read them (that would synchronise):
 *          they are expected strictly increasing without NaN.  For any content (unsorted, equal,
 *          NaN) every add lands inside the point's own block or is dropped;
 *   keep: HOST, n_tables requests of two int32 as df_flow_pdf_marginals takes them: {a, -1} the
 *         1-D table of dimension a, {a, b} with a < b the 2-D table; requests are distinct.
 *         bins and keep are read at call time and reach the kernel by value: no copy, no
 *         synchronisation, capturable;
 *   counts_out: DEVICE int32, point i owns a block of T = Σ_j size_j words, size_j = L_a or
 *         L_a·L_b; table j sits behind the tables before it (request order), the lower-numbered
 *         kept dimension runs fastest: index i_a + L_a·i_b.
 * Bin rule (numpy's for explicit edges): bin j, 0 <= j < L, holds e_j <= v < e_{j+1}, the last
 * bin also v == e_L; Float32 comparisons, −0 equals +0, ±inf are ordinary values and an
 * infinite edge is allowed.  A draw below e_0, above e_L or NaN is counted nowhere in the
 * tables that keep that dimension (a table's sum is its inside count); a 2-D table counts a
 * draw when both coordinates are inside.  The counts equal np.histogram / np.histogram2d of the
 * same Float32 draws bit for bit.
 * One kernel (df_hist.hip): tables and edges in LDS, a branch-free binary search of 8 steps per
 * kept dimension, integer LDS adds, one flush per (point, group of tables); a wave per point up
 * to n_draws = 256 and a workgroup per point above, plain stores of every word (zero bins
 * included), nothing zeroed, no global atomics.  Above n_draws = DF_HIST_SPLIT_DRAWS a point's
 * draws are divided among ceil(n_draws / DF_HIST_SPLIT_DRAWS) workgroups: the blocks are zeroed
 * on the stream and the partial tables merge with integer global atomic adds — the same bytes.
 * (The environment variable DF_HIST_SPLIT_DRAWS, a multiple of 256 above 256, overrides the
 * threshold at call time: a tuning aid, the counts do not depend on it.)
 * What does not fit the LDS at once (at most 64 KiB of tables: one 128 x 128 table) is walked
 * in groups of tables planned on the host (df_hist_plan.cpp); every group reads the draws again.
 * Checked in this order before any device work, also for an empty call: 1 <= d <= 64
 * (DF_ERR_INVALID); n_points >= 0 (DF_ERR_SHAPE); n_draws a positive multiple of 4
 * (DF_ERR_INVALID) and at most 2^24 (DF_ERR_UNSUPPORTED); xs, counts_out, edges, bins, keep
 * non-null and xs 16-byte aligned (DF_ERR_INVALID); 1 <= n_tables <= DF_HIST_MAX_TABLES
 * (DF_ERR_UNSUPPORTED); every bins[k] in [0, DF_HIST_MAX_BINS] (negative: DF_ERR_INVALID, above:
 * DF_ERR_UNSUPPORTED; the message names k); every request well formed — first index in [0, d),
 * second −1 or in (first, d), both of dimensions with bins > 0, no request repeated
 * (DF_ERR_INVALID, the message names the request); T within int32 and T·n_points within int64
 * (DF_ERR_SHAPE).  Then n_points == 0: DF_OK, nothing launched, nothing written.
 *
 * df_flow_point_histograms: df_flow_point_stats' chunk loop with the counting at the end of
 * every chunk.  The draws, the θ repeat, the chunking by whole points, the workspaces, the
 * counters (offset + d·i·n_draws/4) and the rules and messages for the chain, n_points, n_draws,
 * chunk, θ and the bounds are df_flow_point_stats': draw j of point i is bitwise the draw that
 * call makes at the same (seed, offset), and draws_out (optional) is bitwise its copy.
 * counts_out may be NULL when draws_out is given; edges, bins, keep and n_tables are then
 * ignored.  Both NULL is DF_ERR_INVALID.  The table rules above are checked after the outputs.
 * Calls on one chain must not overlap on different streams (the workspaces are the chain's).
 * No host synchronisation; capturable once the workspaces are warm. */
#define DF_HIST_MAX_BINS 128    /* bins per dimension: one 128 x 128 table is 64 KiB of LDS */
#define DF_HIST_MAX_TABLES 2080 /* 64 + 64·63/2: the full corner at d = 64 */
#define DF_HIST_SPLIT_DRAWS 2048 /* draws of a point per workgroup above this n_draws */

int df_draw_histograms(const float* xs, int d, int64_t n_points, int64_t n_draws, const float* edges,
                       const int32_t* bins, const int32_t* keep, int32_t n_tables, int32_t* counts_out,
                       void* stream);

int df_flow_point_histograms(df_chain* chain, const float* theta_raw, int64_t n_points, int64_t n_draws,
                             int64_t chunk, uint64_t seed, uint64_t offset, const float* edges,
                             const int32_t* bins, const int32_t* keep, int32_t n_tables, int32_t* counts_out,
                             float* draws_out, void* stream);

/* ---- importance weights: evidence, ESS, weighted moments per point (additive to ABI 5) ----
 * What follows df_flow_sample_logpdf: the draws of q(. | θ_i) are weighted with
 * w = p̃(x) / q(x | θ_i), p̃ the caller's unnormalised target.  Both calls run on the current
 * device (as df_order_statistics) on the caller's arrays, per point, in fp64, in a fixed order
 * without atomics: two calls give the same bytes, and so does point i computed alone with the
 * pointers advanced.  All pointers are DEVICE memory.  Neither call synchronises, zeroes
 * anything or owns a workspace: both are capturable.  The point mapping follows from n_draws as
 * in df_flow_point_stats (df_iw.hip states the order of every sum).
 *
 * df_importance_weights: per-draw log-weights into stabilised weights and their sums.
 *   logw (n_points · n_draws) Float32, 16-byte aligned, draw j of point i at i·n_draws + j:
 *        log p̃ − log q, formed by the caller.
 *   m_i  the largest non-NaN logw of point i (fmaxf; exact).
 *   w_out[i·n_draws + j] = expf(logw_ij − m_i): one Float32 subtraction, then the library's
 *        expf; the largest weight of a point is 1.  Any 4-byte aligned pointer; it must not
 *        overlap logw (not checked).
 *   stats_out: 4 doubles per point, { (double)m_i, W1 = Σ_j (double)w_ij, W2 = Σ_j (double)w_ij²,
 *        n_pos = #{j : w_ij > 0} as a double }.  The squares are exact in fp64: only the
 *        additions round.
 * Either output may be NULL, not both.  From the block the host forms
 *   log Ẑ_i = m_i + log(W1/N),  ESS_i = W1²/W2,  stderr(log Ẑ_i) = sqrt((N·W2/W1² − 1)/(N − 1)).
 * Nothing is checked on the device (a check would synchronise): logw = −inf gives weight 0; a NaN
 * logw gives a NaN weight for that draw and NaN W1, W2 for its point only (m_i and n_pos, which
 * does not count it, stay numbers); a +inf logw makes m_i = +inf, the weight of that draw NaN,
 * every other weight of the point 0 and W1, W2 NaN; a point whose logw are all −inf has
 * m_i = −inf, every weight and W1, W2 NaN and n_pos 0.  Other points are not touched.
 * Checked in this order before any device work, also for an empty call: n_points >= 0
 * (DF_ERR_SHAPE); n_draws a positive multiple of 4 (DF_ERR_INVALID: the draws come from calls
 * with that rule, and a point's row stays 16-byte aligned) and at most 2^24
 * (DF_ERR_UNSUPPORTED); logw non-null and 16-byte aligned (DF_ERR_INVALID); w_out and stats_out
 * both NULL (DF_ERR_INVALID); n_points · n_draws within int64 (DF_ERR_SHAPE).  Then
 * n_points == 0: DF_OK, nothing launched, nothing written.
 *
 * df_draw_weighted_stats: the weighted sibling of df_flow_point_stats' reduction.
 *   xs (d, n_points·n_draws) 16-byte aligned, draw j of point i at xs + d·(i·n_draws + j): the
 *        layout of draws_out.  w (n_points · n_draws) Float32, 16-byte aligned, as w_out above:
 *        any weights, expected finite and >= 0 (not checked).  x (d, n_points): the points,
 *        needed with wrank_out only.
 *   wrank_out[i·d + k] = Σ_j (double)w_ij · [draw_ij[k] < x_i[k]], the Float32 comparison of
 *        df_flow_point_stats: a tie counts nothing, a NaN on either side counts nothing.
 *        Divided by W1 it is the weighted posterior CDF at the point: the weighted SBC statistic.
 *   sums_out: n_points blocks of 2 + 2d + d(d+1)/2 doubles.  Block i:
 *          W1, W2                              Σ_j w_ij, Σ_j w_ij², in double
 *          c[k] at 2 + k                       the shift: draw 0 of point i, as a double
 *          S1w[k] at 2 + d + k                 Σ_j w_ij·(draw_ij[k] − c[k])
 *          S2w[a, b] at 2 + 2d + a(a+1)/2 + b, a >= b
 *                                              Σ_j w_ij·(draw_ij[a] − c[a])·(draw_ij[b] − c[b])
 *        every value converted to double first; w·(v_a − c_a) is one fp64 multiply, and its
 *        product with (v_b − c_b) (with 1.0 for S1w) is fused into the running sum.  The order
 *        of these sums is df_flow_point_stats': with every weight 1.0f, entries [2, ..) are that
 *        call's block of the same draws bit for bit, wrank_out its rank_out and W1 = W2 = n_draws.
 *        mean = c + S1w/W1, cov = S2w/W1 − δδᵀ with δ = S1w/W1, times 1/(1 − W2/W1²) for the
 *        reliability-weights correction.  A NaN draw makes the sums it touches NaN (a NaN in
 *        draw 0 every entry of its dimension), a NaN weight every sum of its point that its row
 *        enters; nothing is checked.
 * Either output may be NULL, not both; what is not asked for is not computed.
 * Checked in this order before any device work, also for an empty call: 1 <= d <= 64
 * (DF_ERR_INVALID); n_points, then n_draws, as above; xs and w non-null and 16-byte aligned
 * (DF_ERR_INVALID); both outputs NULL, or wrank_out without x (DF_ERR_INVALID); the sizes within
 * int64 (DF_ERR_SHAPE).  Then n_points == 0: DF_OK, nothing launched, nothing written. */
int df_importance_weights(const float* logw, int64_t n_points, int64_t n_draws, float* w_out, double* stats_out,
                          void* stream);

int df_draw_weighted_stats(const float* xs, const float* w, const float* x, int d, int64_t n_points, int64_t n_draws,
                           double* wrank_out, double* sums_out, void* stream);

/* ---- importance resampling -----------------------------------------------------
 * df_draw_resample: per point, n_out picks among its n_draws weighted draws and, gathered, the
 * picked rows — the weighted draws of q(. | θ_i) resampled to equally weighted draws of the
 * corrected posterior, which df_order_statistics, df_draw_histograms and df_draw_weighted_stats
 * (at unit weights) take unchanged.  No handle: the call runs on the current device on the
 * caller's arrays.  All pointers are DEVICE memory.  Nothing is zeroed, nothing synchronises,
 * there are no atomics: the call is capturable.
 *   xs (d, n_points·n_draws), draw j of point i at xs + d·(i·n_draws + j), and w (n_points ·
 *        n_draws) Float32: the layouts of df_draw_weighted_stats; both 16-byte aligned.
 *   idx_out (n_points · n_out) int32: pick k of point i at i·n_out + k, an index within the
 *        point, in [0, n_draws), or −1.
 *   xs_out (d, n_points·n_out): the picked rows, row k of point i at xs_out + d·(i·n_out + k),
 *        copied bit for bit.  It must not overlap xs (not checked).
 *   Either output may be NULL, not both.  With xs_out NULL, xs and d are not looked at.
 *   cdf_ws: a caller-owned workspace of n_points · n_draws uint64 words, 8-byte aligned, needed
 *        when n_draws > DF_RESAMPLE_LDS_DRAWS and ignored otherwise.  Its content after the
 *        call is unspecified.
 * The contract is integer arithmetic throughout: the picks are bitwise reproducible and do not
 * depend on the kernel mapping, the grid, the other points or the chunking of a call.  For one
 * point with weights w_0 .. w_{N−1}:
 *   Quantisation.  A weight takes part when it is finite and > 0.  NaN, ±inf, negative values
 *        and ±0 get q_j = 0 and are never picked.  With wmax the largest weight that takes part
 *        and wmax = f·2^e, f in [0.5, 1) (frexp),
 *          q_j = rint(ldexp((double)w_j, 32 − e)), half to even, as uint64:
 *        the largest q lies in [2^31, 2^32].  Conversion, a power-of-two scale and rint are
 *        exact or correctly rounded: no division, no exp.  A weight below 2^−33 of the point's
 *        scale 2^e becomes 0: at most N·2^−33 of the largest weight's mass is lost.
 *   Scan.  C_0 = 0, C_{j+1} = C_j + q_j, T = C_N < 2^56.
 *   Pick k of K = n_out: with a numerator num_k and a denominator D, the one j with
 *          C_j·D <= num_k·T < C_{j+1}·D        (so q_j > 0),
 *        the products, below 2^112, compared as 128-bit integers; no division.
 *          DF_RESAMPLE_SYSTEMATIC   one 32-bit word r_i per point,  num_k = k·2^32 + r_i,  D = K·2^32
 *          DF_RESAMPLE_STRATIFIED   one 32-bit word r_ik per pick,  num_k = k·2^32 + r_ik, D = K·2^32
 *          DF_RESAMPLE_MULTINOMIAL  one 64-bit word r_ik per pick,  num_k = r_ik,          D = 2^64
 *        (multinomial: C_j <= umulhi64(r_ik, T) < C_{j+1}).
 *   Random words: Philox4x32-10 with key = (seed low, seed high) and counter (c low, c high, 1,
 *        0); the third counter word 1 keeps the stream disjoint from df_random_normal's
 *        (ctr, 0, 0, 0) at the same (seed, offset).
 *          systematic    c = offset + i,                    output word 0
 *          stratified    c = offset + i·(K/4) + k/4,        output word k % 4
 *          multinomial   c = offset + i·(K/2) + k/2,        output words 2(k%2) (low), 2(k%2)+1 (high)
 *        A call consumes n_points, n_points·K/4 and n_points·K/2 counters; a call on the points
 *        [a, b) — pointers advanced — with offset advanced by a, a·K/4 or a·K/2 reproduces the
 *        whole call's picks for those points.
 *   Degenerate point (T = 0: no weight takes part): every pick is −1 and every gathered row is
 *        all-NaN (0x7fc00000).  Other points keep their bits; an index of −1 is never dereferenced.
 *   Output order: systematic and stratified picks are non-decreasing in k; multinomial picks come
 *        in stream order, an exchangeable sample.
 * For any content of w the search stays inside [0, n_draws) and the stores inside the point's own
 * output block.  The scan lives in LDS up to n_draws = DF_RESAMPLE_LDS_DRAWS (a wave per point up
 * to 256 draws, a workgroup per point above) and in cdf_ws past it, where the picks of one point
 * spread over the device; the picks do not depend on the path.
 * Checked in this order before any device work, also for an empty call: method in 0 .. 2
 * (DF_ERR_INVALID); n_points, then n_draws, as in df_importance_weights; n_out a positive multiple
 * of 4 (DF_ERR_INVALID: the result goes straight into the per-point calls, and the Philox counter
 * boundaries fall between points) and at most 2^24 (DF_ERR_UNSUPPORTED); w non-null and 16-byte
 * aligned (DF_ERR_INVALID); both outputs NULL (DF_ERR_INVALID); with xs_out: 1 <= d <= 64, xs
 * non-null and 16-byte aligned (DF_ERR_INVALID); n_draws > DF_RESAMPLE_LDS_DRAWS with cdf_ws NULL
 * or not 8-byte aligned (DF_ERR_INVALID); the sizes within int64 (DF_ERR_SHAPE).  Then
 * n_points == 0: DF_OK, nothing launched, nothing written. */
#define DF_RESAMPLE_SYSTEMATIC 0
#define DF_RESAMPLE_STRATIFIED 1
#define DF_RESAMPLE_MULTINOMIAL 2
#define DF_RESAMPLE_LDS_DRAWS 4096 /* n_draws up to which a point's scan lives in LDS */

int df_draw_resample(const float* xs, const float* w, void* cdf_ws, int d, int64_t n_points, int64_t n_draws,
                     int64_t n_out, int method, uint64_t seed, uint64_t offset, float* xs_out, int32_t* idx_out,
                     void* stream);

/* ---- weighted quantiles and histograms -----------------------------------------
 * df_draw_weight_scale, df_draw_weighted_quantiles, df_draw_weighted_histograms: the median
 * with its interval and the corner plot of per-point draws under importance weights, without
 * resampling.  No handle: the calls run on the current device on the caller's arrays.  All
 * pointers are DEVICE memory except nums, bins and keep (HOST arrays read at call time).
 *   xs (d, n_points·n_draws) and w (n_points · n_draws) Float32: the layouts of
 *        df_draw_weighted_stats and df_draw_resample; both 16-byte aligned.
 *   scale_out (2 int64 per point): {e, T} of point i at 2i, an empty point gives {0, 0}.  It is
 *        required in all three calls: it gives the sums their unit, and it is the hand-off
 *        between the scale kernel and the main kernel of the two larger calls (no hidden
 *        workspace, nothing grows).
 * Everything below is integer arithmetic after the quantisation, so the results are bitwise
 * reproducible and depend neither on the kernel mapping nor on the grid, the other points or the
 * split of a point among workgroups.
 *   Scale of a point (df_draw_resample's, unchanged).  A weight takes part when its bits lie in
 *        [1, 0x7f7fffff]: finite and > 0.  With wmax = f·2^e, f in [0.5, 1), the largest such
 *        weight of the point, q_j = rint(w_j·2^(32 − e)), half to even, formed from the bits.
 *        NaN, ±inf, negative and ±0 weights give q_j = 0.  q_j < 2^32 and T = Σ q_j < 2^56.  A
 *        point with T = 0 is empty.  A weight below 2^−33 of the scale 2^e becomes 0: at most
 *        N·2^−33 of the largest weight's mass is dropped; the rounding is at most half a unit of
 *        2^−32 of the scale per weight; everything past that is exact.
 *   Weighted quantile.  The target is a numerator nums[q] in [0, 2^32] over the denominator
 *        2^32 (a probability p maps to rint((double)p·2^32)).  τ = max(1, ceil(num·T / 2^32)),
 *        the product, below 2^88, as a 128-bit integer.  Per dimension, with key the IEEE
 *        totalOrder key of df_order_statistics and C(k) = Σ {q_j : key_j <= k}, the result is
 *        the draw with the smallest key k such that C(k) >= τ, returned with its own bits: the
 *        inverted-CDF rule on the quantised weights, no interpolation.  num = 0 gives the
 *        smallest draw with a weight that takes part, num = 2^32 the largest such draw; the
 *        result is always a draw with q_j > 0 or one that shares its bits.  NaN draws are not
 *        skipped: they sort to the ends, as in df_order_statistics.  An empty point gives
 *        0x7fc00000 in every slot.
 *        quant_out: element (i·d + k)·n_probs + q, the layout of df_order_statistics' out.
 *   Weighted histogram.  The bin rule, the edge search and the table requests (edges, bins,
 *        keep, n_tables) are df_draw_histograms'.  A bin holds Σ q_j over the draws
 *        df_draw_histograms would have counted there, as uint64: at most T, it cannot overflow.
 *        The mass in the caller's units is bin·2^(e − 32), the normalised mass bin / T.
 *        sums_out: per point a block of the tables in request order, the layout of counts_out
 *        with 8-byte words.  A table holds at most DF_WHIST_MAX_TABLE_BINS bins.  Above
 *        n_draws = DF_HIST_SPLIT_DRAWS a point's draws are divided among workgroups as in
 *        df_draw_histograms: the blocks are zeroed on the stream and take 64-bit integer atomic
 *        adds; below, every bin is written with a plain store.
 *   Unit weights: q_j = 2^31, e = 1; every weighted table is df_draw_histograms' table shifted
 *        left by 31, and for n_draws a power of two the quantile at num = (r + 1)·2^32/n_draws
 *        is order statistic r of df_order_statistics, bit for bit.
 * Checked in this order before any device work, also for an empty call (df_draw_weight_scale:
 * the rules that name its arguments): 1 <= d <= 64 (DF_ERR_INVALID); n_points >= 0
 * (DF_ERR_SHAPE); n_draws a positive multiple of 4 (DF_ERR_INVALID) and at most 2^24
 * (DF_ERR_UNSUPPORTED); every pointer non-null, then xs and w 16-byte aligned (DF_ERR_INVALID);
 * 1 <= n_probs <= DF_WQUANT_MAX_PROBS (DF_ERR_UNSUPPORTED) and every nums[q] <= 2^32
 * (DF_ERR_INVALID, the message names the index); the table rules of df_draw_histograms with
 * their statuses, then a table above DF_WHIST_MAX_TABLE_BINS (DF_ERR_UNSUPPORTED, the message
 * names the request); the sizes within int64 (DF_ERR_SHAPE).  Then n_points == 0: DF_OK, nothing
 * launched, nothing written.  Nothing is checked on the device: for any content of xs, w and
 * edges the reads stay inside the caller's arrays and the stores inside the point's own blocks. */
#define DF_WQUANT_MAX_PROBS 32
#define DF_WHIST_MAX_TABLE_BINS 8192 /* one table: 64 KiB of uint64 in LDS */

int df_draw_weight_scale(const float* w, int64_t n_points, int64_t n_draws, int64_t* scale_out, void* stream);

int df_draw_weighted_quantiles(const float* xs, const float* w, int d, int64_t n_points, int64_t n_draws,
                               const uint64_t* nums, int n_probs, float* quant_out, int64_t* scale_out, void* stream);

int df_draw_weighted_histograms(const float* xs, const float* w, int d, int64_t n_points, int64_t n_draws,
                                const float* edges, const int32_t* bins, const int32_t* keep, int32_t n_tables,
                                uint64_t* sums_out, int64_t* scale_out, void* stream);

/* ---- grid logpdf------------------------------------------------------------
 * logpdf(flow, (x_1, ..., x_d), (θ_1, ..., θ_n)) (src/Flows.jl:287-331; pdf, :348-349, is
 * its exp): the log-density on the outer product of one vector per dimension, generated on
 * the device — nothing of the grid's size is built on the host.
 * axes: DEVICE memory, the d + n axis vectors one after the other (x axes, then raw θ
 * axes; θ is normalised in the kernel with the chain's bounds).  lens: HOST memory, their
 * d + n lengths; a θ given as one value is an axis of length 1.
 * Point p of the P = prod(lens) points has the multi-index (i_1, ..., i_{d+n}) with
 * p = i_1 + L_1 (i_2 + L_2 (...)): the first axis runs fastest, which is
 * Iterators.product order and the column-major reshape(..., lens...).  P may exceed
 * 2^32; the call evaluates the window [first, first + count) and writes `count` values
 * to logpdf_out (DEVICE), bitwise what df_flow_logpdf gives on the same points.
 * The window is evaluated `chunk` points at a time (0: 2^20; rounded up to a multiple of
 * 64, at most 2^24) through a staging buffer of (d + n) * chunk floats that belongs to
 * the chain and only grows; growing it inside a stream capture is DF_ERR_INVALID.
 * count == 0 or an empty axis: DF_OK, nothing launched, logpdf_out untouched.
 * DF_ERR_SHAPE: a negative length, P past int64, a window outside [0, P]. */
int df_flow_logpdf_grid(df_chain* chain, const float* axes, const int64_t* lens, int64_t first, int64_t count,
                        float* logpdf_out, int64_t chunk, void* stream);

/* ---- marginal densities over grid axes (additive to ABI 5) --------------------
 * The 0-, 1- and 2-D marginal tables of pdf on the grid of df_flow_logpdf_grid, reduced on
 * the device chunk by chunk: nothing of the grid's size is written anywhere.
 * axes, lens, first, count, chunk, stream: as for df_flow_logpdf_grid.  weights: DEVICE,
 * one double per axis value, laid out like `axes` (quadrature weights, the caller's rule).
 * keep: HOST, n_marg requests of two int32 each, the kept axes in ascending order, -1 for
 * an unused slot: {-1,-1} the total mass, {a,-1} a 1-D table, {a,b} with a < b a 2-D one.
 * For request K
 *   m_K[i_K] = sum over the window's points p with kept indices i_K of
 *              exp(logpdf(p)) * prod over k not in K of w_k[i_k(p)]
 * with logpdf(p) bitwise df_flow_logpdf_grid's value, exp taken in double of that float,
 * products and sums in double.  Kept axes may be θ axes.
 * out: DEVICE doubles, table j behind the tables before it: 1, L_a or L_a * L_b values,
 * the lower-numbered kept axis fastest.  The call zeroes the tables on the stream and
 * then adds the window's sums: results of several windows (calls, devices) add up.
 * Sums are accumulated with floating-point atomic adds: two runs may differ in the last
 * bits.  No host synchronisation; the staging buffer of df_flow_logpdf_grid is used,
 * one chunk of floats larger, under the same growth rules.
 * count == 0: DF_OK, tables zeroed, nothing launched.  n_marg == 0: DF_OK, nothing runs.
 * DF_ERR_INVALID: a null chain, lens, keep or out (n_marg > 0), null axes or weights
 * (count > 0), a kept index outside [0, d + n), not ascending or repeated.
 * DF_ERR_SHAPE: as df_flow_logpdf_grid, or a total table size past int64.
 * DF_ERR_UNSUPPORTED: more than 128 requests. */
int df_flow_pdf_marginals(df_chain* chain, const float* axes, const double* weights, const int64_t* lens,
                          int64_t first, int64_t count, const int32_t* keep, int32_t n_marg, double* out,
                          int64_t chunk, void* stream);

/* out (n, batch) = the n-vector theta in every column, on the device: the NTuple θ of
 * logpdf(flow, x, θ::Tuple) (src/Flows.jl:284, collect(θ) broadcast over the points). */
int df_theta_broadcast(float* out, const float* theta, int n, int64_t batch, void* stream);

/* ---- truncated sampling (additive to ABI 5) -----------------------------------
 * sample_with_rejection(condition, flow, dims, θ, m) (src/Flows.jl:196-229) for a
 * condition given as a region: the first n_want samples of the flow that lie inside it.
 * The region (all HOST memory, Float32; NaN anywhere is DF_ERR_INVALID):
 *   box          lo[k] <= x[k] <= hi[k] for each of the d dimensions; ±inf allowed; a NULL
 *                lo / hi is -inf / +inf everywhere; lo > hi is legal and rejects everything
 *   half-spaces  n_half in 0..DF_REGION_MAX_HALFSPACES rows of a (n_half, d), row by row:
 *                acc = a[h][0]*x[0]; acc = acc + a[h][k]*x[k] for k = 1 .. d-1; acc <= b[h]
 * Every operation is one Float32 operation, never contracted; comparisons are as written,
 * so a NaN coordinate or a NaN sum rejects.  x is the flow's output (df_flow_sample's).
 * theta_raw: DEVICE, ONE n-vector used for every candidate (the NTuple θ of the
 * reference's signature); NULL for n = 0.
 * Candidates: candidate k = 0, 1, ... is forward! of elements [d*k, d*k + d) of the
 * df_random_normal(seed, offset) stream, so candidates 0..N-1 are what df_flow_sample
 * (batch = N, seed, offset) returns — as far as df_flow_forward_inplace itself gives a
 * sample the same bits at every batch size.  x_out (DEVICE, d * n_want floats) receives
 * the first n_want accepted candidates in increasing k; that does not depend on the rounds.
 *   accepted = min(n_want, accepted among the candidates examined)
 *   tried    = 1 + the index of the candidate that filled the last slot; when the slots
 *              were not filled, the number of candidates examined
 * Candidates with index >= max_tries are never examined (the reference: max_tries = m *
 * n_want, m = 100).  Slots not filled within max_tries: DF_ERR_INVALID, "Impossible to
 * reach convergence of rejection sampling" and the counts; tried_out / accepted_out (HOST,
 * either may be NULL) are still written, the first `accepted` rows of x_out are valid and
 * the rest of x_out is untouched.
 * Rounds: candidates are drawn, sent through forward! and examined a round at a time;
 * a round is a multiple of 4 candidates (a Philox counter boundary; a requested size is
 * rounded up) and is always drawn and forwarded whole, also past max_tries.  round > 0:
 * that size for every round (at most 2^24, else DF_ERR_UNSUPPORTED).  round = 0: the first
 * round holds 2 * n_want candidates, a later one remaining * examined / accepted with a
 * quarter of head-room, each within [2^10, 2^22].
 * SYNCHRONISATION: each round ends with a 16-byte device-to-host copy of the counters
 * and a hipStreamSynchronize of `stream`; there is no other.  The call therefore returns
 * with its work done, and is DF_ERR_INVALID inside a stream capture.  Its workspaces (one
 * round's candidates, θ broadcast, ballots and bases; the region block; the counters)
 * belong to the chain and only grow.
 * Checked before any device work: NULL region, NULL chain -> DF_ERR_INVALID; region->d
 * not the chain's d -> DF_ERR_SHAPE; n_half outside 0..8 -> DF_ERR_UNSUPPORTED; n_want,
 * max_tries or round < 0 -> DF_ERR_SHAPE; n_want == 0 -> DF_OK, nothing runs; θ missing or
 * bounds not set: df_flow_sample's errors. */
#define DF_REGION_MAX_HALFSPACES 8
typedef struct df_region {
    int32_t d, n_half;
    const float* lo;  /* d, or NULL */
    const float* hi;  /* d, or NULL */
    const float* a;   /* n_half * d */
    const float* b;   /* n_half */
} df_region;
int df_flow_sample_region(df_chain* chain, float* x_out, const float* theta_raw, int64_t n_want,
                          const df_region* region, int64_t max_tries, int64_t round, uint64_t seed, uint64_t offset,
                          int64_t* tried_out, int64_t* accepted_out, void* stream);

/* ---- training ---------------------------------------------------------------
 * train!(flow, data, opt_state; ...) src/Flows.jl:380-445: per batch
 *   grads = Flux.gradient(m -> loss(backward(m, x, θ)...), flow.model)   (:398-411)
 *   Optimisers.update!(opt_state, flow.model, grads[1])                  (:413)
 * with loss = -mean(logpdf(MvNormal(0, I), z) .+ ldj)  (src/Flows.jl:352-359)
 * and the custom pullbacks rrule(RNVP_backward) (src/affine/RNVP.jl:99-147),
 * rrule(NICE_backward) (src/affine/NICE.jl:84-113).
 *
 * A df_train handle owns the flat trainable parameters of its chain in
 * Flux.trainables order (per coupling layer: s_net then t_net; per Dense:
 * weight (out×in column-major) then bias; NormalizationLayer: none), the
 * Adam state and the gradient buffer, and rewrites the chain's packed
 * weights after every update, so df_chain_* / df_flow_* calls on the chain
 * see the trained parameters.  Supported: every chain df_chain_create accepts
 * (conditioner width <= 256, any depth — a single Dense included — e.g. the
 * hidden-256 config-5 model), with any of the nine DF_ACT_* activations; σ'
 * follows NNlib's derivative rules (from the output for relu / tanh_fast /
 * sigmoid_fast / leakyrelu / elu, from the pre-activation for softplus /
 * logcosh / swish).  Conditioners of the hidden <= 64, <= 4-output default
 * shape (_dflt_net, src/Layers.jl:33-50, n_sublayers <= 2) run one fused kernel
 * per net; the rest run the layer-wise MFMA path. */

typedef struct df_train df_train;

/* Optimisers.Adam(η, β, ϵ) (Optimisers.jl v0.4; defaults 1e-3, (0.9, 0.999), 1e-8) */
typedef struct df_adam {
    float eta;
    float beta1, beta2;
    float epsilon;
} df_adam;

/* Optimisers.setup(Adam(...), flow.model): state m = v = 0, βᵗ = β.
 *
 * A trainer starts from the parameters its chain evaluates at the moment of creation: those
 * of df_chain_create / the last df_chain_set_weights, or, once a trainer has updated the
 * chain (a step, df_train_set_params), that trainer's — whether it is still alive or was
 * destroyed.  df_train_get_params of the new trainer returns them, its first gradient is
 * taken at them, and its creation changes no bit of what the chain computes.
 *
 * df_train_destroy of the trainer that wrote the chain's weights last copies its parameters
 * into the chain's host plan (one device synchronisation), so that they outlive it; the
 * chain goes on evaluating them.  Several trainers may be alive on one chain.  Each one
 * rewrites the chain's packed weights when it updates, so after either of two trainers has
 * stepped the two have diverged: the chain evaluates the parameters of the one that updated
 * last, and the other keeps its own vector, state and private weight copies until its next
 * update puts them back.  Use one trainer at a time unless that is what you want. */
int df_train_create(df_train** out, df_chain* chain, const df_adam* opt);
int df_train_destroy(df_train* t);
/* Form of the reverse sweep behind df_train_gradient.  Every form
 * computes the same gradient (rrule(RNVP_backward), src/affine/RNVP.jl:99-147, through
 * Flux.gradient, src/Flows.jl:398-411); df_train_create picks one from the chain:
 *   DF_SWEEP_FUSED      one fused per-net kernel: every conditioner the default
 *                       _dflt_net shape at hidden <= 64, <= 4 transformed dims;
 *   DF_SWEEP_H0FREE     layer-wise; the inverse pass keeps each net's features and H1,
 *                       the split dW1 recomputes H0: wide SPLIT chains whose nets are all
 *                       Dense(<= 32, 256, relu) → Dense(256, 256, relu) → Dense(256, <= 32);
 *   DF_SWEEP_KEPT       layer-wise; the inverse pass keeps every hidden activation
 *                       (chains on the generic or wide kernels, when they fit in half the
 *                       free device memory);
 *   DF_SWEEP_RECOMPUTE  layer-wise; the sweep recomputes the hidden activations.
 * H0FREE → KEPT → RECOMPUTE is also the fallback order when device memory runs short
 * (decided at the first gradient of each batch capacity). */
typedef enum df_sweep_form {
    DF_SWEEP_AUTO = 0,
    DF_SWEEP_FUSED = 1,
    DF_SWEEP_H0FREE = 2,
    DF_SWEEP_KEPT = 3,
    DF_SWEEP_RECOMPUTE = 4,
    /* request only: any layer-wise form (the library picks among the three above) */
    DF_SWEEP_LAYERWISE = 5,
    /* flag (with a layer-wise form): each net's dW products and the next net's
     * backward front as separate launches instead of merged ones (the same sums in
     * the same order: a bitwise A/B reference for the merged launches) */
    DF_SWEEP_SEPARATE = 16
} df_sweep_form;
/* df_train_create with a requested sweep form (DF_SWEEP_AUTO: as df_train_create).
 * A form the chain cannot take returns DF_ERR_UNSUPPORTED. */
int df_train_create_ex(df_train** out, df_chain* chain, const df_adam* opt, int sweep);
/* The form the trainer runs (before its first gradient: the one it will try first). */
int df_train_sweep(const df_train* t, int* form);
/* Number of trainable parameters (length of the flat vectors below). */
int df_train_num_params(const df_train* t, int64_t* count);
/* How the trainer's entry points (df_train_gradient and every step built on
 * it) read θ.  train! feeds the model normalised θ (normalized_training_data,
 * src/Data.jl:189-193, src/Flows.jl:391-392); a host may instead hand over the
 * raw θ and let the kernels normalise it with the Flow's MetaData bounds.
 *   DF_THETA_AUTO  (the default): normalise iff the chain has θ bounds
 *                  (df_chain_set_theta_bounds) at the time of the call;
 *   DF_THETA_RAW:  θ is raw and always normalised with the chain's bounds
 *                  (n > 0 without bounds: DF_ERR_INVALID);
 *   DF_THETA_GIVEN: θ is used as given (already normalised); the chain's
 *                  bounds are never consulted, so a later
 *                  df_chain_set_theta_bounds (e.g. by sample) cannot change
 *                  what this trainer computes.
 * A captured df_train_step_graph step is re-captured when the effective
 * convention changes. */
typedef enum df_theta_input {
    DF_THETA_AUTO = 0,
    DF_THETA_RAW = 1,
    DF_THETA_GIVEN = 2
} df_theta_input;
int df_train_set_theta_input(df_train* t, int mode);
/* Gradient of loss over this batch with the mean taken over `n_total`
 * samples (n_total = batch on one GPU; the global batch under data
 * parallelism, so the per-rank gradients SUM to the global one).  θ as the
 * trainer's df_theta_input says (default: normalised with the chain's
 * bounds when set).
 * The result is left in the device buffer returned by df_train_grad_ptr.
 * `logpdf_sum` (device double, may be NULL) receives Σ logpdf of the batch
 * at the current parameters (the loss before the update is -Σ/n_total). */
int df_train_gradient(df_train* t, const float* x, const float* theta_raw, int64_t batch, int64_t n_total,
                      double* logpdf_sum, void* stream);
/* Per-sample gradients of the log-density in its inputs (ABI 5), at the trainer's
 * current parameters.  For every sample j:
 *   logpdf_out[j]      = logpdf(MvNormal(0,I), z_j) + ldj_j,  (z, ldj) = backward(chain, x, θ)
 *   grad_x[:, j]       = ∂logpdf_out[j] / ∂x[:, j]       (d, batch), column-major like x
 *   grad_theta[:, j]   = ∂logpdf_out[j] / ∂θ[:, j]       (n, batch), column-major like θ
 * which is Zygote.gradient((x, θ) -> sum(logpdf(flow, x, θ)), x, θ) through
 * rrule(RNVP_backward) / rrule(NICE_backward) (src/affine/RNVP.jl:137-141,
 * NICE.jl:102-111).  Each output may be NULL and is then not written; grad_theta is
 * ignored when n = 0.  θ is read as df_train_set_theta_input says, like
 * df_train_gradient; when it is raw (normalised in the kernels with the chain's bounds)
 * grad_theta is the gradient in the raw θ: θ̄ / (θmax - θmin), and exactly 0 in a row
 * with θmax == θmin (grad_normalisation, src/Data.jl:236-241).
 * The call changes neither the parameters, the Adam state, the gradient of
 * df_train_gradient nor its Σ logpdf: df_train_gradient → df_train_logpdf_grad →
 * df_train_apply applies the same step as without the middle call.  It is stream-ordered
 * and bitwise reproducible.  grad_x and grad_theta serve as the sweep's workspace while
 * the call runs on the stream.
 * Only trainers on the fused sweep (df_train_sweep: DF_SWEEP_FUSED) are supported.  For a
 * layer-wise trainer (a conditioner with hidden width > 64, more than one hidden Dense,
 * or more than 4 transformed dims in a layer) the call returns DF_ERR_UNSUPPORTED and the
 * trainer stays usable.  batch == 0: DF_OK, nothing written. */
int df_train_logpdf_grad(df_train* t, const float* x, const float* theta, float* logpdf_out, float* grad_x,
                         float* grad_theta, int64_t batch, void* stream);
/* Score moments (additive to ABI 5): df_train_logpdf_grad on (x, θ) reduced on the device into
 * the moment block described at df_flow_sample_logpdf_moments, with m = n, lp = logpdf_out
 * and g = grad_theta (n = 0: the three lp entries alone, the sweep is skipped).  Nothing of
 * the batch's size reaches the host; lp, grad_theta and the sweep's z̄ go to workspaces the
 * trainer owns (they only grow, not inside a stream capture).  θ is read as
 * df_train_set_theta_input says, and the guarantee about the parameters, the optimiser
 * state and the pending gradient is df_train_logpdf_grad's, as is DF_ERR_UNSUPPORTED for a
 * layer-wise trainer (which stays usable).  accumulate == 0: out is overwritten;
 * accumulate == 1: the block is added to out, one fp64 add per entry.  batch == 0: out is
 * zeroed (accumulate == 0) or left as it is (accumulate == 1).  Correct for every n the
 * chain limits allow, tuned for n <= 8 (one pass over the samples; a larger n takes one
 * pass per pair of 8-row tiles of the matrix). */
int df_train_score_moments(df_train* t, const float* x, const float* theta, int64_t batch, double* out,
                           int accumulate, void* stream);
/* The Fisher matrix F(θ) = E_{x ~ q(.|θ)}[∂θ logq ∂θ logqᵀ] = out[3+n ..] / out[0], with the
 * mean score and the entropy sums beside it: the moment block over n_samples draws at ONE
 * raw θ (a device n-vector, NULL for n = 0; bounds required as for df_flow_sample).  Sample s
 * is sample s of df_flow_sample(batch = n_samples, seed, offset).  Chunks as for
 * df_flow_sample_logpdf_moments; per chunk: df_flow_sample at offset + d·start_i/4 into a
 * workspace, the score sweep in the RAW θ whatever df_train_set_theta_input says (the
 * setting is left as it is), and the reduction added to out, which is zeroed on the stream
 * first: out = ((0 + c_1) + c_2) + ...  No host synchronisation.  The workspaces (x, the θ
 * broadcast, lp, gθ, z̄) belong to the trainer, only grow, and may not grow inside a capture.
 * n_samples == 0: DF_OK, out zeroed.  Errors as df_flow_sample_logpdf_moments and
 * df_train_score_moments. */
int df_train_fisher(df_train* t, const float* theta_raw, int64_t n_samples, int64_t chunk, uint64_t seed,
                    uint64_t offset, double* out, void* stream);
/* Device pointer of the flat gradient (count floats); all-reduce it here
 * for multi-GPU data parallelism. */
int df_train_grad_ptr(df_train* t, float** grad_dev);
/* One optimiser step (Adam, or the chain of df_train_create_opt) with the current
 * gradient; repacks the chain's weights. */
int df_train_apply(df_train* t, void* stream);
/* df_train_gradient (n_total = batch) followed by df_train_apply. */
int df_train_step(df_train* t, const float* x, const float* theta_raw, int64_t batch, double* logpdf_sum,
                  void* stream);
/* df_train_gradient (mean over n_total) + df_train_apply as ONE hipGraph
 * launch: the reverse sweep's per-net kernels, reduction, Adam and repack
 * are captured the second time the same (x, θ, batch, n_total, logpdf_sum)
 * buffers are seen and replayed from then on (the first call runs eagerly).
 * For train!'s mini-batch loop (src/Flows.jl:396-414) with reused device
 * staging buffers, where per-launch overhead dominates small batches.
 * Captures are dropped when a buffer they name is reallocated.  Not for
 * data parallelism (the gradient all-reduce sits between the two halves). */
int df_train_step_graph(df_train* t, const float* x, const float* theta_raw, int64_t batch, int64_t n_total,
                        double* logpdf_sum, void* stream);
/* ---- device-resident epochs (additive to ABI 5) -------------------------------
 * A data set that stays on the device: x_set (d, n_samples) and theta_set (n, n_samples),
 * column-major like every batch (each sample's values contiguous), and an optional order
 * of n_samples int32 sample indices (a permutation for a shuffled epoch; repeats allowed).
 *
 * df_batch_gather: one mini-batch out of the set, for hosts that keep their own loop.
 *   x_out[:, j] = x_set[:, order[first + j]],  theta_out[:, j] = theta_set[:, order[first + j]]
 * for j < count (order == NULL: sample first + j).  One launch serves both arrays;
 * n == 0: x alone, the θ pointers are ignored.  Stream-ordered, no synchronisation; nothing
 * past `count` samples of the outputs is written; count == 0 writes nothing.
 * [first, first + count) outside [0, n_samples): DF_ERR_INVALID.  The order's entries are
 * NOT checked here (that costs a synchronisation, see df_train_epoch): an entry outside
 * [0, n_samples) gathers sample 0 instead, it never becomes an address. */
int df_batch_gather(float* x_out, float* theta_out, const float* x_set, const float* theta_set, int d, int n,
                    int64_t n_samples, const int32_t* order, int64_t first, int64_t count, void* stream);
/* One epoch of train!'s mini-batch loop (src/Flows.jl:396-417) on a resident set:
 * ceil(n_samples / batchsize) steps, step i being df_train_step on the samples
 * order[i·batchsize ... min((i+1)·batchsize, n_samples)) (the partial last batch is kept,
 * as Flux.DataLoader keeps it), with the trainer's optimiser (df_train_create_opt,
 * df_train_adjust) and θ convention (df_train_set_theta_input).  Parameters and optimiser
 * state afterwards are bitwise those of that loop of df_train_step calls.
 * step_logpdf_sum (device, one double per step, may be NULL) receives every step's
 * Σ logpdf at the parameters before its update (the step's loss is -Σ/batch).
 * The mini-batches are gathered on the device into staging buffers the trainer owns
 * (sized at the first use of a batchsize); the position in the epoch is a device counter,
 * so every full-batch step is the same captured graph (a second one serves the partial
 * last batch): gather, gradient, update and counter advance replay as one launch per
 * step.  The two graphs live in slots of their own beside df_train_step_graph's, are
 * captured the second time their step is seen with the same (x_set, theta_set,
 * n_samples, order, batchsize, step_logpdf_sum), and are re-captured after
 * df_train_adjust or when a buffer they name was reallocated.
 * The call is stream-ordered and returns without waiting for the steps.  With an order it
 * synchronises the stream once, before the first step, to check the order: entries outside
 * [0, n_samples) return DF_ERR_INVALID (the message names their number) and no step is
 * enqueued.  With order == NULL it does not synchronise.  No step costs a host
 * synchronisation or a host-to-device copy.
 * Under df_train_set_debug the steps run eagerly with the per-step loss check: a
 * non-finite loss returns DF_ERR_NONFINITE, leaves the parameters at the last good step and
 * writes the refused step's index to *steps_done.  Otherwise *steps_done (host, may be
 * NULL) is the number of steps enqueued.
 * n_samples == 0: DF_OK, nothing runs.  batchsize <= 0 or x_set == NULL: DF_ERR_INVALID.
 * n_samples >= 2^31: DF_ERR_SHAPE.  Not for data parallelism (df_train_step_dist). */
int df_train_epoch(df_train* t, const float* x_set, const float* theta_set, int64_t n_samples, const int32_t* order,
                   int64_t batchsize, double* step_logpdf_sum, int64_t* steps_done, void* stream);
/* ---- sample weights (additive to ABI 5) ----------------------------------------
 * The weighted loss of one mini-batch,  loss_w = -Σ_i w_i·logpdf_i / W,  W = Σ_i w_i:
 * for nested-sampling and importance-sampling chains, reweighted simulations, event
 * weights.  w is a device float[batch]; wsums a device double[2] that receives
 * {Σ_i w_i·logpdf_i, W} (may be NULL); the loss is -wsums[0] / wsums[1].
 *   W      summed in fp64 in a fixed order on the device (w_total == 0), or w_total as
 *          given (w_total > 0: data-parallel shards pass the global sum, so the shards'
 *          gradients add up to the global batch's gradient);
 *   inv_W  = 1.f / (float)W, so that w ≡ 1 gives 1.f / (float)batch bit for bit: with unit
 *          weights the gradient is bitwise df_train_gradient's with n_total = batch;
 *   wj_i   = w_i · inv_W in Float32 is the only form of the weights the sweep sees
 *          (z̄_i = z_i·wj_i, j̄_i = wj_i): scaling every weight by a power of two changes
 *          no bit of the gradient;
 *   Σw·lp  summed in fp64 in a fixed order over the per-sample Float32 logpdf.
 * NOT checked (a check would synchronise, as for df_batch_gather's order): the weights
 * are expected finite and >= 0 with W > 0.  A zero-weight sample must still have finite
 * x and θ (0·NaN is NaN).  W <= 0 or a non-finite weight gives a non-finite loss and
 * gradient; under df_train_set_debug such a step is refused with DF_ERR_NONFINITE (the
 * read-back divides by W).  Nothing past `batch` entries of x, θ or w is read.
 * w_total negative or NaN, or w == NULL with batch > 0: DF_ERR_INVALID.
 * batch == 0: zero gradient, zero wsums.
 * df_train_step_w: gradient_w (w_total = 0) + df_train_apply.
 * df_train_step_graph_w: that step as one hipGraph, as df_train_step_graph; the capture is
 * keyed by (x, θ, w, batch, w_total, wsums).  W is recomputed inside the graph, so
 * rewriting the weight buffer between replays is honoured. */
int df_train_gradient_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                        double w_total, double* wsums, void* stream);
int df_train_step_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                    double* wsums, void* stream);
int df_train_step_graph_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                          double w_total, double* wsums, void* stream);
/* df_batch_gather with the set's weights: also w_out[j] = w_set[order[first + j]], in the
 * same launch.  Every rule of df_batch_gather holds (a bad order entry gathers sample 0 of
 * all three arrays). */
int df_batch_gather_w(float* x_out, float* theta_out, float* w_out, const float* x_set, const float* theta_set,
                      const float* w_set, int d, int n, int64_t n_samples, const int32_t* order, int64_t first,
                      int64_t count, void* stream);
/* df_train_epoch with sample weights (w_set: device float[n_samples]): step i is
 * df_train_step_w on its mini-batch with the gathered weights, W being that mini-batch's
 * own sum.  step_wsums (device, 2 doubles per step, may be NULL) receives every step's
 * {Σ w·logpdf, W}.  Every rule of df_train_epoch holds; the weighted steps are captured in
 * graph slots of their own. */
int df_train_epoch_w(df_train* t, const float* x_set, const float* theta_set, const float* w_set, int64_t n_samples,
                     const int32_t* order, int64_t batchsize, double* step_wsums, int64_t* steps_done, void* stream);
/* wsums[0..1] = {Σ_j w_j·logpdf_j, Σ_j w_j} over a batch, both in fp64 in a fixed order
 * (the epoch losses of a weighted set: -wsums[0] / wsums[1]).  df_flow_*: θ raw;
 * df_chain_*: θ as given.  batch == 0 zeroes wsums.  The per-sample logpdf goes through a
 * workspace the chain owns (it only grows). */
int df_flow_logpdf_wsum(df_chain* chain, const float* x, const float* theta_raw, const float* w, int64_t batch,
                        double* wsums, void* stream);
int df_chain_logpdf_wsum(df_chain* chain, const float* x, const float* theta, const float* w, int64_t batch,
                         double* wsums, void* stream);
/* train!(...; debug=true) (src/Flows.jl:404-409): when on, df_train_apply
 * (and the steps built on it) first reads the Σ logpdf of the last gradient
 * evaluation back to the host; if the loss is NaN or ±Inf the parameters are
 * NOT updated and DF_ERR_NONFINITE is returned (the reference throws an
 * ArgumentError before Optimisers.update!).  Costs one 8-byte device→host
 * copy and a stream synchronisation per step; df_train_step_graph runs its
 * steps eagerly while it is on. */
int df_train_set_debug(df_train* t, int on);
/* Copy the current trainables to / from host memory (count floats). */
int df_train_get_params(df_train* t, float* host_out, int64_t count);
int df_train_set_params(df_train* t, const float* host_in, int64_t count);

/* ---- optimiser chains: Optimisers.OptimiserChain on the device (additive to ABI 5) ----
 * A chain is an ordered list of 1..DF_OPT_MAX_RULES rules.  For every parameter tensor
 * (one Dense weight or one Dense bias: the leaves Optimisers.setup sees), with x the
 * parameters before the step and dx = the flat gradient (df_train_gradient, or what the
 * all-reduce left), each rule in order maps dx ← rule(x, dx), then x ← x - dx.  Float32:
 *   DF_OPT_ADAM          p = {η, β1, β2, ϵ}   Optimisers.Adam on the incoming dx: m, v updated,
 *                                             dx = m / (1-β1ᵗ) / (sqrt(v / (1-β2ᵗ)) + ϵ) · η
 *   DF_OPT_DESCENT       p = {η}              dx = η · dx
 *   DF_OPT_CLIP_GRAD     p = {δ}              dx = clamp(dx, -δ, δ)
 *   DF_OPT_CLIP_NORM     p = {ω}              nrm = sqrt(Σ dx²) over the tensor (p = 2);
 *                                             nrm > ω: dx = dx · (ω / nrm), else dx as it is
 *                                             (so also for nrm == 0 and a NaN nrm)
 *   DF_OPT_WEIGHT_DECAY  p = {λ}              dx = dx + λ · x
 * WeightDecay before Adam is L2 regularisation, after it decoupled decay (AdamW).
 * Limits: at most one Adam, at most one ClipNorm and at least one of Adam / Descent per
 * chain; a ClipNorm stands before the chain's Adam.  Outside them: DF_ERR_UNSUPPORTED.
 * Bad values (δ, ω <= 0, λ < 0, η < 0, β outside [0, 1), ϵ < 0, any NaN): DF_ERR_INVALID.
 * The message names the rule. */
#define DF_OPT_MAX_RULES 8
typedef enum df_opt_kind {
    DF_OPT_ADAM = 1,
    DF_OPT_DESCENT = 2,
    DF_OPT_CLIP_GRAD = 3,
    DF_OPT_CLIP_NORM = 4,
    DF_OPT_WEIGHT_DECAY = 5
} df_opt_kind;
typedef struct df_opt_rule {
    int32_t kind;
    float p[4];
} df_opt_rule;
/* Optimisers.setup(OptimiserChain(rules...), flow.model), with a sweep form as
 * df_train_create_ex.  df_train_create / df_train_create_ex are the one-rule chain [Adam];
 * a chain that is exactly [Adam] runs their kernels. */
int df_train_create_opt(df_train** out, df_chain* chain, const df_opt_rule* rules, int n_rules, int sweep);
/* Optimisers.adjust!(state, η): sets η of the chain's Adam, or without one of its first
 * Descent; m, v and βᵗ are kept.  Captured df_train_step_graph steps are re-captured. */
int df_train_adjust(df_train* t, float eta);
/* The parameter tensors as slices of the flat vectors: `count` tensors, and count + 1
 * offsets (host memory; tensor k is [offsets[k], offsets[k+1]), offsets[count] =
 * df_train_num_params).  ClipNorm's norms are taken over these. */
int df_train_num_tensors(const df_train* t, int64_t* count);
int df_train_tensor_offsets(const df_train* t, int64_t* offsets_out, int64_t count_plus_1);
/* Per-tensor 2-norms of the gradient buffer as it stands (df_train_num_tensors device
 * floats).  Stream-ordered, changes no state, bitwise reproducible (fixed-order sums). */
int df_train_grad_norms(df_train* t, float* out_dev, void* stream);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------
 * The batch is sharded into contiguous sample blocks (samples are independent
 * through the chain, src/Chains.jl:149-197); the only exchanges are the sums
 * the reference's reductions imply:
 *   loss = -mean(logpdf)  (src/Flows.jl:352-359) → all-reduce {Σ logpdf, count}
 *   Flux.gradient          (src/Flows.jl:398-411) → all-reduce of the flat ∇
 * RCCL is resolved at run time (an already-loaded librccl is reused, else
 * librccl.so.1); without it these calls return DF_ERR_UNSUPPORTED.
 *
 * Bootstrap: rank 0 calls df_comm_get_unique_id and ships the
 * DF_COMM_ID_BYTES bytes to every rank out of band (MPI, a file, a TCP
 * store); then every rank calls df_comm_init_rank (collective). */

typedef struct df_comm df_comm;

#define DF_COMM_ID_BYTES 128

typedef enum df_dtype { DF_DTYPE_F32 = 0, DF_DTYPE_F64 = 1 } df_dtype;

int df_comm_get_unique_id(void* id_out /* DF_COMM_ID_BYTES */);
int df_comm_init_rank(df_comm** out, int nranks, const void* id, int rank, int device);
int df_comm_destroy(df_comm* comm);
int df_comm_get_info(const df_comm* comm, int* rank, int* nranks, int* device);
/* In-place sum over all ranks of `count` elements of device memory, ordered
 * on `stream`. */
int df_comm_allreduce_sum(df_comm* comm, void* buf_dev, int64_t count, int dtype, void* stream);
/* The NLL of a sharded batch (config 3): this rank's Σ logpdf of its shard
 * (df_flow_logpdf_sum) and its sample count are written to sum_count[0..1]
 * (device doubles) and all-reduced, so on return (stream-ordered) every rank
 * holds the global {Σ, N}; loss = -Σ / N.  comm = NULL: this process only. */
int df_flow_nll(df_chain* chain, df_comm* comm, const float* x, const float* theta_raw, int64_t batch,
                double* sum_count, void* stream);
/* df_flow_nll with θ used as given (normalised): the sharded loss of the model
 * on normalized data, as train!'s epoch losses (src/Flows.jl:419-430). */
int df_chain_nll(df_chain* chain, df_comm* comm, const float* x, const float* theta, int64_t batch,
                 double* sum_count, void* stream);
/* All-reduce (sum) of the flat gradient of df_train_gradient; every rank must
 * have called df_train_gradient with n_total = the global batch. */
int df_train_allreduce_gradient(df_train* t, df_comm* comm, void* stream);
/* One data-parallel train! step on this rank's shard: df_train_gradient (mean
 * over n_total, the global batch) → all-reduce of ∇ and of Σ logpdf →
 * df_train_apply (identical Adam step on every rank).  `logpdf_sum` (device
 * double or NULL) receives the GLOBAL Σ logpdf.  comm = NULL: one process. */
int df_train_step_dist(df_train* t, df_comm* comm, const float* x, const float* theta_raw, int64_t batch,
                       int64_t n_total, double* logpdf_sum, void* stream);

/* ---- diagnostics (no reference counterpart) ---------------------------------
 * Effective shader clock of the fused chain-pass kernels, the evidence behind a
 * clock-normalised benchmark time (the chip lowers its clock under load, and
 * devices differ).  on = 1 zeroes the stamp buffer and makes every later chain
 * pass of this handle that runs the specialised (kernels 1-4) or wide (5, 6)
 * kernel accumulate, per workgroup, Δs_memtime (shader cycles) and
 * Δs_memrealtime (100 MHz ticks) over its wave 0's lifetime; on = 0 stops.
 * df_chain_clock_read synchronises the device and returns the median over
 * workgroup slots and the ratio of sums (GHz), and the number of slots
 * stamped (0: nothing stamped yet). */
int df_chain_clock_probe(df_chain* chain, int on);
int df_chain_clock_read(df_chain* chain, double* ghz_median, double* ghz_mean, int64_t* n_slots);

/* ---- device memory helpers (for hosts without a GPU array package) ------ */
int df_device_alloc(void** ptr, size_t bytes);
int df_device_free(void* ptr);
int df_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int df_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int df_stream_synchronize(void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DENSITYFLOWS_HIP_H */
