// df_trainer.h — the df_train handle: its host plan (df_train_plan.h) and its device state.
// Private to the training units: df_train_capi.hip (the entry points) and df_lsweep.hip (the
// layer-wise reverse sweep).
#pragma once

#include "df_handle.h"
#include "df_ltrain.h"
#include "df_train.h"

// One launch of df_train_logpdf_grad's sweep.
struct ScoreOp {
    int layer;   // index in plan.layers
    int net;     // index in TrainPlan::nets (pair: the s-net), -1 for a NormalizationLayer
    int net2;    // pair: the t-net, else -1
    int phase;
    size_t lds;
};

// One captured step (run_captured, df_train_capi.hip): valid while the buffers it names are
// the ones it was captured with.
struct StepGraph {
    hipGraphExec_t exec = nullptr;
    int seen = 0;                     // eager runs of this step (captured on the second)
    int64_t cap_gen = -1, partial_gen = -1;
    int flow = -1;                    // the θ convention it was recorded with (θ normalised in-kernel or not)
};

// A captured df_train_step_graph step and the caller's buffers it names.
struct TrainGraph {
    const void *x = nullptr, *theta = nullptr, *lp = nullptr;
    int64_t batch = 0, n_total = 0;
    StepGraph g;
    uint64_t last_use = 0;
    const void* w = nullptr;  // df_train_step_graph_w: the weight buffer and w_total
    double w_total = 0.0;
};

// What a captured epoch step names besides the trainer's own buffers.
struct EpochKey {
    const float* x_set = nullptr;
    const float* theta_set = nullptr;
    const int32_t* order = nullptr;
    const double* step_lp = nullptr;
    int64_t n_samples = 0, batchsize = 0;
    const float* w_set = nullptr;  // df_train_epoch_w
    bool operator==(const EpochKey& o) const {
        return x_set == o.x_set && theta_set == o.theta_set && order == o.order && step_lp == o.step_lp &&
               n_samples == o.n_samples && batchsize == o.batchsize && w_set == o.w_set;
    }
};

// One device-side regather of a packed blob from the flat parameters (launch_repack, or
// launch_repack_split for bf16x3 plane blobs).  The blob belongs to the chain or the trainer;
// n = 0: the chain has no such blob, nothing launches.
struct RepackMap {
    void* blob = nullptr;
    DevBuf dst, src;
    int64_t n = 0;
    bool split = false;
};

// The batch-sized buffers: ensure_capacity replaces them all together.
struct BatchBufs {
    DevBuf d_snap, d_zbar, d_ebuf;
    std::vector<DevBuf> d_lh, d_ld;  // H_k and δ_k buffers [cap][lwidth]
    std::vector<DevBuf> d_lv;        // σ'(x_k) buffers [cap][lwidth] (nets with LNet::pre)
    DevBuf d_lyp[2];                 // ȳ  [cap][lwidth], by net parity
    DevBuf d_lbp[2];                 // δ of the last hidden Dense [cap][lwidth], by net parity
    DevBuf d_lx;                     // gathered conditioner input [cap][lwidth]
    // hidden activations kept by the inverse pass (generic kernel): the sweep then
    // skips the forward recompute.  [(layer·2 + net)·lmax_h + k][B][lwidth]
    DevBuf d_hsave;
    // H0-free sweep (df_train::fmode): feature rows and the relu mask of H0
    DevBuf d_fsave, d_hmask;
};

struct df_train {
    df_chain* c = nullptr;
    df::TrainPlan tp;                 // what the host decided at creation; constant from then on
    // live optimiser state, copied from the plan: df_train_adjust sets η here, and the kernels
    // take both by value at launch
    df_adam opt{};
    df::OptChain och{};
    DevBuf d_bt;                      // device βᵗ of the next update (Adam), [β1ᵗ, β2ᵗ]
    int64_t cap_gen = 0;              // bumped when the batch-sized buffers are reallocated
    hipStream_t cap_stream = nullptr; // capture stream of run_captured
    std::vector<TrainGraph> graphs;
    uint64_t use_clock = 0;
    DevBuf d_params, d_m, d_v, d_grad, d_partial, d_lpsum;  // float [P] (d_partial: [grid][P]); double Σ logpdf
    DevBuf d_tblob, d_tsblob, d_lsblob, d_lblob;            // TrainPlan's four blobs
    // every packed blob's regather from d_params, in launch order (TrainPlan::map_sources)
    std::vector<RepackMap> maps;
    BatchBufs bb;
    bool debug = false;               // df_train_set_debug: refuse updates on a non-finite loss
    int theta_input = DF_THETA_AUTO;  // df_train_set_theta_input
    const double* last_lp = nullptr;  // Σ logpdf written by the last df_train_gradient
    int64_t last_n = 0;               // ... and the n_total it was taken over
    // a weighted gradient (df_train_gradient_w) wrote {Σ w·lp, W} at last_lp: last_ws == last_lp, else nullptr
    const double* last_ws = nullptr;
    // the weighted gradient's buffers (ensure_weight_capacity, at the first weighted call):
    // wj = w / W and the per-sample logpdf, float [wcap]; the span sums of the fp64
    // reductions; the trainer's own {Σ w·lp, W}
    DevBuf d_wj, d_wlp, d_wpart, d_wsums;
    int64_t wcap = 0;
    int64_t cap = 0;       // batch capacity of bb
    int grid = 0;          // workgroups of a full net launch (resident on the device)
    size_t lds_max = 0;
    // df_train_logpdf_grad (score_net_kernel), planned on the first call: one launch per
    // RNVP layer (both nets) where that fits, else per net; resident workgroups
    std::vector<ScoreOp> score_ops;
    int score_grid = 0;
    bool score_per_net = false;       // DF_SCORE_PER_NET=1 at df_train_create: per-net launches only (A/B)
    int lgrid = 0;                   // workgroups of the dW kernels (partial rows)
    bool hsave_on = false;           // bb.d_hsave is in use
    // H0-free sweep (TrainPlan::fmode at first; ensure_capacity clears it when the buffers do
    // not fit): the inverse pass keeps each net's features vcat(θ, u)[axis_nn] ([layer·2 +
    // net][B][32]) and H1 only (d_hsave with one slot per net); the split dW1 recomputes H0 from
    // the features and writes its relu mask (d_hmask, 1 KiB per 32 samples) for the W1ᵀδ1 epilogue
    bool fmode = false;
    DevBuf d_toff;                   // TrainPlan::toff, on the device once a kernel needs it
    DevBuf d_sumsq, d_oblocks;       // float [tensors] Σ dx²; TrainPlan::oblocks
    // df_train_epoch: the mini-batch staging buffers ((d, ecap) and (n, ecap), sized at the
    // first use of a batchsize, only growing), the device cursor (int64 step index, then the
    // int count of order_range_kernel) and the two captured steps (gather, gradient, update,
    // cursor advance) with their sample counts: slot 0 the full batch, slot 1 the epoch's
    // partial last batch.  Valid while the epoch's key and the buffers it names stand
    DevBuf d_ex, d_eth, d_cursor;
    int64_t ecap = 0;
    EpochKey ekey;
    StepGraph eg[2];
    int64_t eg_count[2] = {0, 0};
    // df_train_epoch_w: the gathered weights (float [ewcap]) and the weighted steps' own key
    // and graph slots
    DevBuf d_ew;
    int64_t ewcap = 0;
    EpochKey ekeyw;
    StepGraph egw[2];
    int64_t egw_count[2] = {0, 0};
    // df_train_score_moments / df_train_fisher (df_moments.hip); capacities in bytes, they only
    // grow: the sweep's lp (float [batch]) and gθ (n, batch), the reduction's per-workgroup
    // blocks (double [workgroups][3 + n + n²]), and one chunk's draws x (d, chunk) with the θ
    // broadcast (n, chunk)
    DevBuf d_mom_lp, d_mom_g, d_mom_part, d_mom_x, d_mom_th;
    int64_t mom_lp_cap = 0, mom_g_cap = 0, mom_part_cap = 0, mom_x_cap = 0, mom_th_cap = 0;
};

// the H0-free sweep is planned and its buffers fit (ensure_capacity)
inline bool h0free(const df_train* t) { return t->fmode && t->hsave_on && t->bb.d_fsave.get(); }

// Whether the kernels normalise θ for this trainer (df_theta_input); DF_THETA_RAW
// without bounds on a conditional chain is an error (-1).
inline int theta_flow(const df_train* t) {
    const df_chain* c = t->c;
    if (c->plan.n == 0) return 0;
    switch (t->theta_input) {
    case DF_THETA_GIVEN: return 0;
    case DF_THETA_RAW: return c->has_bounds ? 1 : -1;
    default: return c->has_bounds ? 1 : 0;
    }
}

// The per-layer arguments every sweep kernel takes: LDenseArgs, TrainArgs and ScoreArgs
// name them alike.
template <typename Args>
void fill_layer_args(Args& a, const df_train* t, int layer, int phase, const float* x, const float* theta, bool flow,
                     int64_t batch) {
    const df_chain* c = t->c;
    const df::Plan& P = c->plan;
    const df::DevLayer& L = P.layers[layer];
    const float* snap = t->bb.d_snap.as<const float>();
    const float* bounds = c->d_bounds.as<const float>();
    const int32_t* tables = c->d_tables.as<const int32_t>();
    const int64_t bd = batch * P.d;
    a.u_in = (layer + 1 < P.n_layers) ? snap + (int64_t)(layer + 1) * bd : x;
    a.u_out = snap + (int64_t)layer * bd;
    a.theta = theta;
    a.tmin = flow ? bounds : nullptr;
    a.tmax = flow ? bounds + P.n : nullptr;
    a.feat = tables + L.feat_tab;
    a.af = tables + L.af_tab;
    a.d = P.d;
    a.n = P.n;
    a.n_af = L.n_af;
    a.kind = L.kind;
    a.phase = phase;
    a.batch = batch;
}

// The adjoint of a NormalizationLayer, element-wise on z̄.
inline hipError_t norm_adjoint(const df_train* t, int layer, float* zbar, int64_t batch, hipStream_t st) {
    const df::Plan& P = t->c->plan;
    const df::DevLayer& L = P.layers[layer];
    const float* xmn = t->c->d_params.as<const float>() + L.norm_off;
    return df::launch_norm_adjoint(zbar, xmn, xmn + P.d, L.alpha, L.beta, P.d, batch, st);
}

namespace df {
namespace api {
// df_train_logpdf_grad past its trainer-class and batch checks (df_train_capi.hip; batch > 0,
// fused sweep).  flow: -1 θ as df_train_set_theta_input says, 1 raw θ normalised with the
// chain's bounds, 0 θ as given.
int score_sweep(df_train* t, const float* x, const float* theta, float* logpdf_out, float* grad_x, float* grad_theta,
                int64_t batch, int flow, hipStream_t st);
}  // namespace api
}  // namespace df

// df_lsweep.hip: the dynamic LDS its kernel families declare (df_train_create_opt), and the
// reverse sweep of the layer-wise path (chain order, see df_ltrain.h).
hipError_t lsweep_set_lds_limits();
// wj: the weighted loss's j̄ per sample (nullptr: inv_n for every sample)
int lsweep(df_train* t, const float* x, const float* theta, int64_t batch, float inv_n, const float* wj, bool flow,
           hipStream_t st);
