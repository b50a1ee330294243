// df_train.h — launch interface of the training path (reverse sweep of the
// NLL through the inverse pass, Adam, weight repacking).
//
// One training step (src/Flows.jl:396-414: Flux.gradient of
// loss(backward(model, x, θ)) then Optimisers.update!):
//   1. inverse pass on the specialised kernel, keeping every layer's output
//      U[li] ([layer][sample][d], U[0] = z) and the Σ logpdf partials;
//   2. z̄ = z / N (∂loss/∂z for loss = -mean(logpdf(MvNormal(0,I), z) + ldj));
//   3. layers in chain order li = 0..L-1 (reverse of the inverse pass): one
//      train_net_kernel launch per conditioner (s-net, then t-net), which
//      recomputes the net on U[li+1], applies the coupling pullback
//      (rrule(RNVP_backward) src/affine/RNVP.jl:119-143, NICE.jl:102-111),
//      back-propagates through the Dense chain on MFMA, accumulates dW / db per
//      workgroup in registers and updates z̄ in place; NormalizationLayer
//      scales z̄ element-wise;
//   4. a fixed-order reduction of the per-workgroup partials → ∇ (flat,
//      Flux.trainables order); [multi-GPU: the caller all-reduces ∇ here];
//   5. Adam (Optimisers.jl) on the flat parameters, then the packed weight
//      blobs are regathered from them on device.
#pragma once

#include <hip/hip_runtime.h>

#include "df_train_plan.h"

namespace df {

#ifndef DF_TRAIN_WAVES
#define DF_TRAIN_WAVES 8
#endif
constexpr int kTrainWaves = DF_TRAIN_WAVES;     // waves per workgroup of the fused net kernel
constexpr int kTrainThreads = 64 * kTrainWaves;
// 16-sample tiles one wave of a SPLIT instance carries through the sweep together: with
// 2, a workgroup is kTrainWaves / 2 waves (one per SIMD, VGPRs + AGPRs = 512 per lane)
// and each wave interleaves two independent tiles (df_train_impl.h).  The per-SIMD tile
// count, the LDS transpose area and the tiles per workgroup pass are unchanged.
#ifndef DF_TRAIN_TT
#define DF_TRAIN_TT 1
#endif
constexpr int kTrainSplitTT = DF_TRAIN_TT;
static_assert(kTrainWaves % kTrainSplitTT == 0, "tiles per wave must divide the workgroup's tile count");
constexpr int train_threads(bool split) { return split ? kTrainThreads / kTrainSplitTT : kTrainThreads; }
// Per-wave transpose buffers [row][16 samples] (df_train_impl.h): rows of 20 floats (row
// R and R + 4 of a ds_write_b32 half-wave hit disjoint bank halves) and, with
// DF_TRAIN_SWZ, the 4-float column quads XOR-swizzled by row (trn::rswz: Gray bit of
// (R >> 2) & 3 ^ bit 4 of R) so both b128 fragment read shapes are bank-conflict free too.
#ifndef DF_TRAIN_SWZ
#define DF_TRAIN_SWZ 1
#endif
constexpr int kTS = 20;  // row stride (floats)

namespace trn {
// σ' applied by the layer-wise δ kernels when the factor was stored at recompute
// time (nets with a pre-activation σ): hprev then holds σ'(x) itself.
constexpr int kDactStored = 64;
}  // namespace trn

struct TrainArgs {
    const float* u_in;       // U[li+1]: the layer's input in the inverse pass
    const float* u_out;      // U[li]:   its output
    const float* theta;
    const float* tmin;       // θ bounds (nullptr: θ used as given)
    const float* tmax;
    const int32_t* feat;     // [16] state slot of conditioner feature k (n + d → zero)
    const int32_t* af;       // [n_af] state slots of the transformed dims
    float* zbar;             // [sample][d] adjoint of the layer output, updated in place
    float* ebuf;             // [sample][4] exp(-s) from the s-net launch
    float* partial;          // [workgroup][p_total] gradient partials
    const uint8_t* blob;     // chain weight blob (forward fragments)
    const uint8_t* tblob;    // transposed fragments
    const uint8_t* sblob;    // SPLIT: the chain's SPLIT blob (forward region of the net)
    const uint8_t* tsblob;   // SPLIT: the trainer's W1ᵀ planes
    int64_t batch;
    int64_t p_total;
    int d, n, n_af, kind, phase;
    float inv_n;             // 1 / (global batch size)
    GNet net;
    const float* wj;         // weighted instances: [sample] w_s / W (j̄ per sample), else nullptr
};

size_t train_net_lds(int ht, const GNet& g);
hipError_t set_train_lds_limit(size_t lds);
hipError_t launch_train_net(int ht, int nh, int am, const TrainArgs& a, unsigned grid, size_t lds,
                            hipStream_t st);
hipError_t train_net_occupancy(int ht, int nh, int am, size_t lds, int* blocks, bool split = false);

hipError_t launch_scale(float* dst, const float* src, float s, int64_t count, hipStream_t st);
hipError_t launch_norm_adjoint(float* zbar, const float* xmin, const float* xmax, float alpha, float beta, int d,
                               int64_t batch, hipStream_t st);

// ---- sample weights (df_train_gradient_w, df_flow_logpdf_wsum) ----
// The fp64 sums run in a fixed order over spans of kWsumSpan elements, one workgroup each
// (df_train.hip); `part` holds one double per span (wsum_parts(batch)).
constexpr int kWsumThreads = 256;
constexpr int64_t kWsumSpan = 16 * kWsumThreads;
inline int64_t wsum_parts(int64_t batch) { return (batch + kWsumSpan - 1) / kWsumSpan; }
// wj[i] = w[i] · (1.f / (float)W), W = w_total if > 0 else Σ w; wsums[1] = W (wsums may be nullptr)
hipError_t launch_weight_norm(const float* w, int64_t batch, double w_total, double* part, float* wj, double* wsums,
                              hipStream_t st);
// *out = Σ w_i · lp_i
hipError_t launch_weighted_lp_sum(const float* w, const float* lp, int64_t batch, double* part, double* out,
                                  hipStream_t st);
// z̄[i][:] = z[i][:] · wj[i] ([sample][d])
hipError_t launch_scale_rows(float* dst, const float* src, const float* wj, int d, int64_t batch, hipStream_t st);
hipError_t launch_reduce_grads(const float* partial, int n_parts, int64_t p_total, float* grad, hipStream_t st);
// Adam update with βᵗ read from bt[0..1] on the device, then βᵗ .*= β (one more launch).
hipError_t launch_adam(float* x, const float* g, float* m, float* v, int64_t count, float eta, float b1, float b2,
                       float eps, float* bt, hipStream_t st);
hipError_t launch_repack(float* blob, const int32_t* dst, const int32_t* src, int64_t count, const float* params,
                         hipStream_t st);
// SPLIT blob: byte offset dst[i] ← bf16 plane (src[i] & 3) of params[src[i] >> 2] (plane 3: the f32 value)
hipError_t launch_repack_split(uint8_t* blob, const int32_t* dst, const int32_t* src, int64_t count,
                               const float* params, hipStream_t st);

// ---- optimiser chains (df_train_create_opt; Optimisers.OptimiserChain) ----
// tensor_sumsq_kernel: the longest chain of additions one element's square goes through.
// 4 accumulators per thread, each over every 256th quad of the tensor (a tensor has at
// most 256·256 floats = 16,384 quads: 64 additions), 2 levels to combine the four, and
// the 8 levels of the workgroup's tree.
constexpr int kSumsqK = 64 + 2 + 8;
// out[t] = Σ dx² over tensor t = [toff[t], toff[t+1]) with dx = g after rules [0, n_pre) of
// the chain (x: the parameters, read by WeightDecay), or its square root (take_sqrt).
// One workgroup per tensor, fixed summation order, no atomics.
hipError_t launch_tensor_sumsq(const float* g, const float* x, const int32_t* toff, int n_tensors, const OptChain& ch,
                               int n_pre, bool take_sqrt, float* out, hipStream_t st);
// The whole chain per element, then x -= dx; with an Adam in the chain βᵗ .*= β follows
// (adam_advance_kernel).  sumsq: launch_tensor_sumsq's output for the chain's ClipNorm.
hipError_t launch_opt_chain(float* x, const float* g, float* m, float* v, float* bt, const float* sumsq,
                            const OptBlock* blocks, int64_t n_blocks, const OptChain& ch, hipStream_t st);

// ---- device-resident epochs (df_batch_gather, df_train_epoch; df_epoch.hip) ----
// x_out[j] / th_out[j] (d / n floats per sample) = row order[pos + j] of the set (order ==
// nullptr: pos + j) for j < count, pos = first + *cursor · batchsize (cursor == nullptr:
// first).  A position or an index outside [0, n_samples) reads row 0.  th_out or th_set
// nullptr: x alone.
hipError_t launch_batch_gather(float* x_out, float* th_out, const float* x_set, const float* th_set, int d, int n,
                               int64_t n_samples, const int32_t* order, int64_t first, const int64_t* cursor,
                               int64_t batchsize, int64_t count, hipStream_t st);
// ... and w_out[j] = w_set[row j] in the same launch (the weighted instance of the kernel)
hipError_t launch_batch_gather_w(float* x_out, float* th_out, float* w_out, const float* x_set, const float* th_set,
                                 const float* w_set, int d, int n, int64_t n_samples, const int32_t* order,
                                 int64_t first, const int64_t* cursor, int64_t batchsize, int64_t count,
                                 hipStream_t st);
// step_ws[2·*cursor .. +1] = ws[0..1] (step_ws may be nullptr), then *cursor += 1: one thread
hipError_t launch_cursor_advance_w(int64_t* cursor, const double* ws, double* step_ws, hipStream_t st);
// *bad (device int) = how many of order[0, n_samples) lie outside [0, n_samples)
hipError_t launch_order_range(const int32_t* order, int64_t n_samples, int* bad, hipStream_t st);
// step_lp[*cursor] = *lp (step_lp may be nullptr), then *cursor += 1: one thread
hipError_t launch_cursor_advance(int64_t* cursor, const double* lp, double* step_lp, hipStream_t st);

// ---- per-sample input gradients of logpdf (df_train_logpdf_grad; df_score_impl.h) ----
// The same sweep as the trainer's with the seed z̄ = -z, j̄ = 1 and no reduction over the
// batch: score_net_kernel recomputes one conditioner (exact f32, GNet::u), applies the
// coupling pullback and back-propagates to the conditioner input; its rows go to z̄
// (identity dims) and, new here, to θ̄ (θ slots).  No dW / db, no LDS transposes.
// 4 waves per workgroup, one 16-sample tile each and one wave per SIMD: the hidden-64
// instances hold 157-168 VGPRs, 3 waves per SIMD, which an 8-wave workgroup (2 per SIMD)
// cannot fill
constexpr int kScoreWaves = 4;
constexpr int kScoreThreads = 64 * kScoreWaves;

struct ScoreArgs {
    const float* u_in;       // U[li+1]: the layer's input in the inverse pass
    const float* u_out;      // U[li]:   its output
    const float* theta;
    const float* tmin;       // θ bounds (nullptr: θ used as given)
    const float* tmax;
    const int32_t* feat;     // [16] state slot of conditioner feature k (n + d → zero)
    const int32_t* af;       // [n_af] state slots of the transformed dims
    float* zbar;             // [sample][d] adjoint of the layer output, updated in place
    float* thbar;            // [sample][n] adjoint of the (normalised) θ, added to in place; may be nullptr
    float* ebuf;             // [sample][4] exp(-s) from the s-net launch
    const uint8_t* blob;     // chain weight blob (forward fragments)
    const uint8_t* tblob;    // transposed fragments
    int64_t batch;
    int d, n, n_af, kind, phase;
    GNet net;                // the net of this launch; pair launches: the layer's s-net
    GNet net2;               // pair launches (one per RNVP layer): its t-net
};

inline size_t score_net_lds(const GNet& g) { return (size_t)g.fwd_bytes + (size_t)g.t_bytes; }
constexpr size_t kScoreLdsMax = 160 * 1024;    // LDS of a gfx950 workgroup
// (sets the instance's MaxDynamicSharedMemorySize to the largest lds it has been launched with)
// pair: one launch runs a.net (s) then a.net2 (t) of an RNVP layer; lds holds both
hipError_t launch_score_net(int ht, int nh, int am, bool pair, const ScoreArgs& a, unsigned grid, size_t lds,
                            hipStream_t st);
hipError_t score_net_occupancy(int ht, int nh, int am, bool pair, size_t lds, int* blocks);
// gθ[j][i] = θ̄[j][i] / (θmax[i] - θmin[i]), 0 where θmax == θmin (normalize_input's constant rows)
hipError_t launch_score_theta_raw(float* gth, const float* tmin, const float* tmax, int n, int64_t batch,
                                  hipStream_t st);

}  // namespace df
