// df_train_capi.hip — the training entry points of the C ABI (df_train_*).
//
// Host side of one train! step (src/Flows.jl:396-414); the device work is in
// df_train.hip / df_train_impl.h, the inverse pass with per-layer outputs in
// the specialised chain kernel (df_uniform_impl.h, ChainArgs::snap).  What a trainer decides
// on the host is planned in df_train_plan.cpp; the layer-wise sweep's launches are in
// df_lsweep.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <new>

#include "df_trainer.h"

using namespace df;
using namespace df::api;

namespace {

void drop(StepGraph& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    g = StepGraph{};
}

// The captured graphs and their stream (the device buffers free themselves with the handle).
void free_all(df_train* t) {
    for (TrainGraph& g : t->graphs) drop(g.g);
    t->graphs.clear();
    for (StepGraph& g : t->eg) drop(g);
    for (StepGraph& g : t->egw) drop(g);
    if (t->cap_stream) (void)hipStreamDestroy(t->cap_stream);
    t->cap_stream = nullptr;
}

int ensure_capacity(df_train* t, int64_t batch) {
    if (batch <= t->cap) return DF_OK;
    t->cap_gen++;  // captured train steps name the old buffers
    const Plan& P = t->c->plan;
    t->bb = BatchBufs{};  // every old buffer goes before the new ones are sized (hipMemGetInfo below)
    BatchBufs& bb = t->bb;
    t->cap = 0;
    const int64_t cap = std::max<int64_t>(batch, 1024);
    const int ew = t->tp.layerwise ? 32 : 4;  // exp(-s) row width
    auto nomem = [] { return set_err(DF_ERR_NOMEM, "hipMalloc failed (training activations)"); };
    if (bb.d_snap.alloc(sizeof(float) * P.n_layers * cap * P.d) != hipSuccess ||
        bb.d_zbar.alloc(sizeof(float) * cap * P.d) != hipSuccess ||
        bb.d_ebuf.alloc(sizeof(float) * cap * ew) != hipSuccess)
        return nomem();
    if (t->tp.layerwise) {
        const size_t row = sizeof(float) * (size_t)cap * t->tp.lwidth;
        for (DevBuf* b : {&bb.d_lyp[0], &bb.d_lyp[1], &bb.d_lbp[0], &bb.d_lbp[1], &bb.d_lx})
            if (b->alloc(row) != hipSuccess) return nomem();
        // keep the inverse pass's hidden activations when the chain runs on the generic
        // kernel and they fit (else the sweep recomputes them)
        t->hsave_on = false;
        if (!P.uniform && t->tp.sweep_req != DF_SWEEP_RECOMPUTE) {
            // fmode: H1 only, plus the 32-float feature rows and the relu-mask buffer; else
            // H0 and H1 of every net.  Whatever does not fit falls back: fmode → kept H0/H1
            // → recompute (the sweep's forms, struct df_train)
            size_t free_b = 0, total_b = 0;
            const bool info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
            auto try_keep = [&](bool fm) {
                const size_t hbytes = row * (size_t)P.n_layers * 2 * (fm ? 1 : t->tp.lmax_h);
                const size_t fbytes = fm ? sizeof(float) * (size_t)cap * 32 * P.n_layers * 2 : 0;
                const size_t mbytes = fm ? (size_t)(cap + 31) / 32 * 1024 : 0;
                if (!info || hbytes + fbytes + mbytes >= free_b / 2) return false;
                DevBuf h, f, m;  // (all three or none)
                if (h.alloc(hbytes) != hipSuccess ||
                    (fm && (f.alloc(fbytes) != hipSuccess || m.alloc(mbytes) != hipSuccess)))
                    return false;
                bb.d_hsave = std::move(h);
                bb.d_fsave = std::move(f);
                bb.d_hmask = std::move(m);
                return true;
            };
            if (t->fmode && !try_keep(true)) t->fmode = false;  // sized for H0 and H1 below
            if (t->fmode || try_keep(false)) t->hsave_on = true;
            (void)hipGetLastError();
        }
        for (int k = 0; k <= t->tp.lmax_h; ++k) {
            DevBuf h, dl, dv;
            const bool pre = t->tp.any_pre && k < t->tp.lmax_h;
            if (h.alloc(row) != hipSuccess || dl.alloc(row) != hipSuccess || (pre && dv.alloc(row) != hipSuccess))
                return nomem();
            bb.d_lh.push_back(std::move(h));
            bb.d_ld.push_back(std::move(dl));
            if (pre) bb.d_lv.push_back(std::move(dv));
        }
    }
    t->cap = cap;
    return DF_OK;
}

int repack(df_train* t, hipStream_t st) {
    const float* params = t->d_params.as<const float>();
    for (const RepackMap& m : t->maps) {
        const int32_t *dst = m.dst.as<const int32_t>(), *src = m.src.as<const int32_t>();
        const hipError_t e = m.split ? launch_repack_split(static_cast<uint8_t*>(m.blob), dst, src, m.n, params, st)
                                     : launch_repack(static_cast<float*>(m.blob), dst, src, m.n, params, st);
        if (e != hipSuccess) return hip_err(e, "repack kernel launch");
    }
    t->c->params_owner = t;  // the chain evaluates this trainer's parameters from here on
    return DF_OK;
}

int ensure_toff(df_train* t) { return t->d_toff.get() ? DF_OK : upload(t->tp.toff, t->d_toff); }

// Device state of an optimiser chain: the tensor offsets, Σ dx² per tensor and the update
// kernel's workgroup → tensor table (TrainPlan::oblocks).
int setup_chain(df_train* t) {
    int rc = ensure_toff(t);
    if (rc == DF_OK) rc = upload(t->tp.oblocks, t->d_oblocks);
    if (rc != DF_OK) return rc;
    const size_t sb = sizeof(float) * (size_t)std::max((int)t->tp.toff.size() - 1, 4);
    if (t->d_sumsq.alloc(sb) != hipSuccess) return set_err(DF_ERR_NOMEM, "hipMalloc failed (optimiser chain)");
    if (hipMemset(t->d_sumsq.get(), 0, sb) != hipSuccess) return set_err(DF_ERR_HIP, "hipMemset(optimiser chain)");
    return DF_OK;
}

// The weighted gradient's buffers, sized with the batch buffers (allocated at the first
// weighted call, so an unweighted trainer's allocations keep their sequence): wj and the
// per-sample logpdf (float [cap] each) and the span sums of the fp64 reductions.
int ensure_weight_capacity(df_train* t) {
    if (t->wcap >= t->cap) return DF_OK;
    t->cap_gen++;  // captured weighted steps name the old buffers
    t->wcap = 0;
    if (t->d_wj.alloc(sizeof(float) * t->cap) != hipSuccess || t->d_wlp.alloc(sizeof(float) * t->cap) != hipSuccess ||
        t->d_wpart.alloc(sizeof(double) * std::max<int64_t>(wsum_parts(t->cap), 1)) != hipSuccess)
        return set_err(DF_ERR_NOMEM, "hipMalloc failed (sample weights)");
    t->wcap = t->cap;
    return DF_OK;
}

// The gradient of one mini-batch.  w == nullptr: -mean(logpdf) over n_total, Σ logpdf to *sums
// (or the trainer's own double).  w: the weighted loss (df_train_gradient_w), {Σ w·lp, W} to
// sums[0..1]; the sweep's two seeds are then per sample (wj = w / W), from the trainer's
// weight buffers.
int gradient(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch, int64_t n_total,
             double w_total, double* sums, void* stream) {
    df_chain* c = t->c;
    const Plan& P = c->plan;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* lp = sums ? sums : t->d_lpsum.as<double>();  // where this gradient writes Σ logpdf
    t->last_lp = lp;
    t->last_n = n_total;
    t->last_ws = w ? lp : nullptr;
    if (batch == 0) {
        hipError_t e = hipMemsetAsync(t->d_grad.get(), 0, sizeof(float) * t->tp.n_params, st);
        if (e == hipSuccess) e = hipMemsetAsync(lp, 0, sizeof(double), st);
        return e == hipSuccess ? DF_OK : hip_err(e, "hipMemsetAsync");
    }
    if (!x) return set_err(DF_ERR_INVALID, "null input array");
    if (P.n > 0 && !theta_raw)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    const int tf = theta_flow(t);
    if (tf < 0) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds) for DF_THETA_RAW");
    const bool flow = tf == 1;
    int rc = ensure_capacity(t, batch);
    if (rc == DF_OK && w) rc = ensure_weight_capacity(t);
    if (rc != DF_OK) return rc;
    const BatchBufs& bb = t->bb;
    float *snap = bb.d_snap.as<float>(), *zbar = bb.d_zbar.as<float>();
    float *partial = t->d_partial.as<float>(), *grad = t->d_grad.as<float>();
    float* wj = w ? t->d_wj.as<float>() : nullptr;

    // 1. inverse pass keeping every layer's output (U[li] = snap[li], U[0] = z); weighted:
    //    logpdf per sample instead of its sum
    const bool fm = h0free(t);  // H0-free sweep (features + H1 kept)
    rc = run(c, MODE_LOGPDF, flow, x, theta_raw, nullptr, nullptr, w ? t->d_wlp.as<float>() : nullptr,
             w ? nullptr : lp, batch,
             stream, snap, t->hsave_on ? bb.d_hsave.as<float>() : nullptr, t->tp.lwidth, fm ? 1 : t->tp.lmax_h,
             fm ? bb.d_fsave.as<float>() : nullptr);
    if (rc != DF_OK) return rc;
    // 2. z̄ = z / N, or z̄_i = z_i · wj_i after wj = w / W and the two sums
    const float inv_n = w ? 0.f : 1.f / (float)n_total;
    hipError_t e;
    if (w) {
        double* part = t->d_wpart.as<double>();
        e = launch_weight_norm(w, batch, w_total, part, wj, lp, st);
        if (e == hipSuccess) e = launch_weighted_lp_sum(w, t->d_wlp.as<const float>(), batch, part, lp, st);
        if (e != hipSuccess) return hip_err(e, "weight kernel launch");
        e = launch_scale_rows(zbar, snap, wj, P.d, batch, st);
    } else {
        e = launch_scale(zbar, snap, inv_n, batch * P.d, st);
    }
    if (e != hipSuccess) return hip_err(e, "scale kernel launch");
    // 3. reverse sweep, chain order
    if (t->tp.layerwise) {
        rc = lsweep(t, x, theta_raw, batch, inv_n, wj, flow, st);
        if (rc != DF_OK) return rc;
        e = launch_reduce_grads(partial, t->lgrid, t->tp.n_params, grad, st);
        return e == hipSuccess ? DF_OK : hip_err(e, "gradient reduction launch");
    }
    const int64_t ntiles = (batch + 15) / 16;
    const int grid = (int)std::min<int64_t>(t->grid, (ntiles + kTrainWaves - 1) / kTrainWaves);
    for (const SweepOp& op : t->tp.ops) {
        if (op.net < 0) {
            e = norm_adjoint(t, op.layer, zbar, batch, st);
            if (e != hipSuccess) return hip_err(e, "norm adjoint launch");
            continue;
        }
        TrainArgs a{};
        fill_layer_args(a, t, op.layer, op.phase, x, theta_raw, flow, batch);
        a.zbar = zbar;
        a.ebuf = bb.d_ebuf.as<float>();
        a.partial = partial;
        a.blob = c->d_blob.as<const uint8_t>();
        a.tblob = t->d_tblob.as<const uint8_t>();
        a.sblob = c->d_sblob.as<const uint8_t>();
        a.tsblob = t->d_tsblob.as<const uint8_t>();
        a.p_total = t->tp.n_params;
        a.inv_n = inv_n;
        a.wj = wj;
        a.net = t->tp.nets[op.net];
        e = launch_train_net(P.ht, t->tp.net_nh[op.net], t->tp.amode, a, (unsigned)grid, t->lds_max, st);
        if (e != hipSuccess) return hip_err(e, "train kernel launch");
    }
    // 4. fixed-order reduction of the workgroup partials
    e = launch_reduce_grads(partial, grid, t->tp.n_params, grad, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "gradient reduction launch");
}

// One step of an epoch on `st`: the mini-batch at the device cursor into the staging
// buffers, df_train_step on it (Σ logpdf into the trainer's own double), then the cursor
// moves on and leaves the step's Σ logpdf in step_lp.  Under df_train_set_debug a refused
// update returns before the advance.
int epoch_step(df_train* t, int64_t count, hipStream_t st) {
    const Plan& P = t->c->plan;
    const EpochKey& k = t->ekey;
    int64_t* cursor = t->d_cursor.as<int64_t>();
    float* ex = t->d_ex.as<float>();
    float* eth = P.n > 0 ? t->d_eth.as<float>() : nullptr;
    hipError_t e = launch_batch_gather(ex, eth, k.x_set, k.theta_set, P.d, P.n, k.n_samples, k.order, 0, cursor,
                                       k.batchsize, count, st);
    if (e != hipSuccess) return hip_err(e, "batch gather launch");
    int rc = df_train_gradient(t, ex, eth, count, count, nullptr, st);
    if (rc == DF_OK) rc = df_train_apply(t, st);
    if (rc != DF_OK) return rc;
    e = launch_cursor_advance(cursor, t->d_lpsum.as<const double>(), const_cast<double*>(k.step_lp), st);
    return e == hipSuccess ? DF_OK : hip_err(e, "cursor advance launch");
}

// The weighted step of an epoch (df_train_epoch_w): the weights gathered with x and θ,
// df_train_step_w on them, both sums to step_wsums.
int epoch_step_w(df_train* t, int64_t count, hipStream_t st) {
    const Plan& P = t->c->plan;
    const EpochKey& k = t->ekeyw;
    int64_t* cursor = t->d_cursor.as<int64_t>();
    float* ex = t->d_ex.as<float>();
    float* eth = P.n > 0 ? t->d_eth.as<float>() : nullptr;
    float* ew = t->d_ew.as<float>();
    hipError_t e = launch_batch_gather_w(ex, eth, ew, k.x_set, k.theta_set, k.w_set, P.d, P.n, k.n_samples, k.order,
                                         0, cursor, k.batchsize, count, st);
    if (e != hipSuccess) return hip_err(e, "batch gather launch");
    int rc = df_train_gradient_w(t, ex, eth, ew, count, 0.0, nullptr, st);
    if (rc == DF_OK) rc = df_train_apply(t, st);
    if (rc != DF_OK) return rc;
    e = launch_cursor_advance_w(cursor, t->d_wsums.as<const double>(), const_cast<double*>(k.step_lp), st);
    return e == hipSuccess ? DF_OK : hip_err(e, "cursor advance launch");
}

// Deleter of df_train_create_opt's scope guard: destroys the trainer and leaves last_error()
// as it found it.
struct DestroyTrainer {
    void operator()(df_train* t) const {
        const std::string m = last_error();
        df_train_destroy(t);
        set_err(DF_OK, m);
    }
};

// One step as a captured graph: staleness → drop; replay; else the body eagerly at first sight
// (it allocates every buffer it needs; stamped with the buffers' generations), captured on the
// trainer's private stream at the second, instantiated and launched.  body(stream) enqueues
// the step; what names it in the errors.  A capture that names reallocated buffers, an
// adjusted η (df_train_adjust bumps cap_gen) or the other θ convention is stale.
template <typename Body>
int run_captured(df_train* t, StepGraph& g, hipStream_t st, const char* what, Body&& body) {
    const int flow_now = theta_flow(t);
    t->c->params_owner = t;  // (a replayed step repacks without passing through repack())
    if (g.cap_gen != t->cap_gen || g.partial_gen != t->c->partial_gen || g.flow != flow_now) drop(g);
    auto where = [&](const char* call) { return std::string(call) + "(" + what + ")"; };
    if (!g.exec) {
        if (!g.seen) {
            const int rc = body(st);
            g.seen = 1;
            g.flow = flow_now;
            g.cap_gen = t->cap_gen;
            g.partial_gen = t->c->partial_gen;
            return rc;
        }
        if (!t->cap_stream && hipStreamCreateWithFlags(&t->cap_stream, hipStreamNonBlocking) != hipSuccess)
            return set_err(DF_ERR_HIP, "hipStreamCreate failed");
        hipError_t e = hipStreamBeginCapture(t->cap_stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return hip_err(e, "hipStreamBeginCapture");
        const int rc = body(t->cap_stream);
        hipGraph_t graph = nullptr;
        e = hipStreamEndCapture(t->cap_stream, &graph);
        if (rc != DF_OK || e != hipSuccess || !graph) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc != DF_OK ? rc : hip_err(e, "hipStreamEndCapture");
        }
        if (g.cap_gen != t->cap_gen || g.partial_gen != t->c->partial_gen) {  // a buffer moved while capturing
            (void)hipGraphDestroy(graph);
            return set_err(DF_ERR_HIP, "internal: training buffers reallocated during graph capture");
        }
        e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) {
            g.exec = nullptr;
            return hip_err(e, where("hipGraphInstantiate").c_str());
        }
    }
    const hipError_t e = hipGraphLaunch(g.exec, st);
    return e == hipSuccess ? DF_OK : hip_err(e, where("hipGraphLaunch").c_str());
}

// df_train_step_graph and df_train_step_graph_w (w != nullptr): the step behind one key of
// the trainer's graph cache.
int step_graph(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch, int64_t n_total,
               double w_total, double* sums, void* stream) {
    DeviceGuard gd(t->c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    // gradient + update + repack on a stream
    auto step = [&](hipStream_t s) {
        const int rc = w ? df_train_gradient_w(t, x, theta_raw, w, batch, w_total, sums, s)
                         : df_train_gradient(t, x, theta_raw, batch, n_total, sums, s);
        return rc != DF_OK ? rc : df_train_apply(t, s);
    };
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (t->debug) return step(st);  // the loss check synchronises: no capture while it is on
    TrainGraph* g = nullptr;
    for (TrainGraph& e : t->graphs)
        if (e.x == x && e.theta == theta_raw && e.lp == sums && e.batch == batch && e.n_total == n_total && e.w == w &&
            e.w_total == w_total)
            g = &e;
    if (!g) {
        if (t->graphs.size() >= 4) {  // keep the 4 most recently used keys
            auto lru = t->graphs.begin();
            for (auto it = t->graphs.begin(); it != t->graphs.end(); ++it)
                if (it->last_use < lru->last_use) lru = it;
            drop(lru->g);
            t->graphs.erase(lru);
        }
        t->graphs.push_back({x, theta_raw, sums, batch, n_total, {}, 0, w, w_total});
        g = &t->graphs.back();
    }
    g->last_use = ++t->use_clock;
    return run_captured(t, g->g, st, "train step", step);
}

}  // namespace

extern "C" {

int df_train_destroy(df_train* t) {
    if (!t) return DF_OK;
    df_chain* c = t->c;
    DeviceGuard gd(c->device);
    free_all(t);
    c->n_trainers--;
    // The chain keeps evaluating this trainer's parameters: its host copy follows them, so that
    // the next trainer plans its blobs from them and starts from them.  (One synchronisation:
    // destroy is not hot.  A trainer another one has repacked over leaves nothing behind.)
    int rc = DF_OK;
    if (c->params_owner == t) {
        c->params_owner = nullptr;
        const size_t nb = sizeof(float) * (size_t)t->tp.n_params;
        if (nb > 0 && t->d_params.get() && c->plan.trainables.size() == (size_t)t->tp.n_params) {
            hipError_t e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(c->plan.trainables.data(), t->d_params.get(), nb, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = hip_err(e, "df_train_destroy: reading the parameters back");
        }
    }
    delete t;
    return rc;
}

int df_train_create(df_train** out, df_chain* c, const df_adam* opt) {
    return df_train_create_ex(out, c, opt, DF_SWEEP_AUTO);
}

int df_train_create_ex(df_train** out, df_chain* c, const df_adam* opt, int sweep) {
    const df_adam a = opt ? *opt : df_adam{1e-3f, 0.9f, 0.999f, 1e-8f};
    const df_opt_rule rule{DF_OPT_ADAM, {a.eta, a.beta1, a.beta2, a.epsilon}};
    return df_train_create_opt(out, c, &rule, 1, sweep);
}

int df_train_create_opt(df_train** out, df_chain* c, const df_opt_rule* rules, int n_rules, int sweep) {
    if (!out || !c) return set_err(DF_ERR_INVALID, "null pointer");
    *out = nullptr;
    // 1. the host plan: nothing is allocated yet
    const Plan& P = c->plan;
    const TrainPlanOpts o{c->exact, c->no_wide, use_split(c), use_wsplit(c), sweep};
    TrainPlan plan;
    std::string err;
    int rc = build_train_plan(P, o, rules, n_rules, &plan, &err);
    if (rc != DF_OK) return set_err(rc, err);
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    // 2. the handle
    df_train* t = new (std::nothrow) df_train();
    if (!t) return set_err(DF_ERR_NOMEM, "host allocation failed");
    t->c = c;
    t->tp = std::move(plan);
    const TrainPlan& tp = t->tp;
    t->opt = tp.adam;
    t->och = tp.och;
    t->fmode = tp.fmode;
    if (const char* v = std::getenv("DF_SCORE_PER_NET")) t->score_per_net = v[0] == '1';
    c->n_trainers++;
    // 3. the device state: any return before release() destroys the handle
    std::unique_ptr<df_train, DestroyTrainer> guard(t);
    // LDS and resident grid of the net kernels
    for (const GNet& g : tp.nets) t->lds_max = std::max(t->lds_max, train_net_lds(P.ht, g));
    if (t->lds_max > 160 * 1024) return set_err(DF_ERR_UNSUPPORTED, "training kernel needs more than 160 KiB of LDS");
    hipError_t e = set_train_lds_limit(t->lds_max);
    if (e != hipSuccess) return hip_err(e, "hipFuncSetAttribute(train)");
    int occ = 1;
    for (size_t i = 0; i < tp.nets.size(); ++i) {
        int b = 1;
        if (train_net_occupancy(P.ht, tp.net_nh[i], tp.amode, t->lds_max, &b, tp.nets[i].split != 0) == hipSuccess &&
            b >= 1)
            occ = (i == 0) ? b : std::min(occ, b);
    }
    t->grid = std::max(1, c->grid_cus * occ);
    if (tp.layerwise) {
        e = lsweep_set_lds_limits();
        if (e != hipSuccess) return hip_err(e, "hipFuncSetAttribute(layer-wise training)");
        t->lgrid = std::max(1, c->grid_cus);
        t->grid = t->lgrid;  // partial rows
    }
    if (c->debug_launch)  // tuning aid (DF_DEBUG_LAUNCH=1): the resident grids on stderr
        std::fprintf(stderr, "[df] train: %s sweep, %d CUs (of %d), grid %d at %d workgroups per CU, lgrid %d\n",
                     tp.layerwise ? "layer-wise" : "fused", c->grid_cus, c->n_cu, t->grid, occ, t->lgrid);
    const size_t pb = sizeof(float) * (size_t)std::max<int64_t>(tp.n_params, 4);
    if (t->d_params.alloc(pb) != hipSuccess || t->d_m.alloc(pb) != hipSuccess || t->d_v.alloc(pb) != hipSuccess ||
        t->d_grad.alloc(pb) != hipSuccess || t->d_partial.alloc(pb * t->grid) != hipSuccess ||
        t->d_lpsum.alloc(sizeof(double)) != hipSuccess || t->d_bt.alloc(2 * sizeof(float)) != hipSuccess)
        return set_err(DF_ERR_NOMEM, "hipMalloc failed (training state)");
    // Optimisers.setup: βᵗ = β for the first update
    const float bt[2] = {t->opt.beta1, t->opt.beta2};
    if (hipMemcpy(t->d_bt.get(), bt, sizeof(bt), hipMemcpyHostToDevice) != hipSuccess)
        return set_err(DF_ERR_HIP, "hipMemcpy(Adam state)");
    // The trainer's blobs and every blob's repack map (TrainPlan::map_sources: the order repack()
    // launches).  A map that is switched off keeps its entry and its (16-byte) index arrays with n = 0,
    // which launches nothing, and the device allocations below keep the sequence they have
    // always had: where these buffers land on the device moves a small-batch step by 0.1 %
    // (profiles/train_host_refactor_ab.txt), so neither drop one nor reorder them.
    using TP = TrainPlan;
    const auto ms = tp.map_sources(P);
    t->maps.resize(TP::kMaps);
    auto dst = [&](int i) { return upload(*ms[i].dst, t->maps[i].dst); };
    auto src = [&](int i) { return upload(*ms[i].src, t->maps[i].src); };
    auto both = [&](int i) {
        const int rc2 = dst(i);
        return rc2 != DF_OK ? rc2 : src(i);
    };
    if ((rc = upload(tp.tblob, t->d_tblob)) != DF_OK || (rc = upload(tp.lblob, t->d_lblob)) != DF_OK ||
        (rc = both(TP::ML)) != DF_OK || (rc = dst(TP::MP)) != DF_OK || (rc = both(TP::MW)) != DF_OK ||
        (rc = both(TP::MWB)) != DF_OK || (rc = src(TP::MP)) != DF_OK || (rc = both(TP::MT)) != DF_OK ||
        (rc = both(TP::MS)) != DF_OK || (rc = both(TP::MWS)) != DF_OK ||
        (rc = upload(tp.lsblob, t->d_lsblob)) != DF_OK || (rc = both(TP::MLS)) != DF_OK ||
        (rc = upload(tp.tsblob, t->d_tsblob)) != DF_OK || (rc = both(TP::MTS)) != DF_OK)
        return rc;
    void* const blobs[TP::kMaps] = {c->d_blob.get(),   t->d_tblob.get(), c->d_wblob.get(),  // (after every upload)
                                    c->d_wbias.get(),  c->d_sblob.get(), c->d_wsblob.get(),
                                    t->d_lblob.get(),  t->d_tsblob.get(), t->d_lsblob.get()};
    for (int i = 0; i < TP::kMaps; ++i) {
        RepackMap& m = t->maps[i];
        m.blob = blobs[i];
        m.n = ms[i].on ? (int64_t)ms[i].dst->size() : 0;
        m.split = ms[i].split;
    }
    // The parameters the chain evaluates now: those of the live trainer that last repacked it,
    // else the host copy (df_chain_create, df_chain_set_weights, or the last owner's at its
    // df_train_destroy).
    const df_train* owner = c->params_owner;
    const size_t nb = sizeof(float) * (size_t)tp.n_params;
    if (owner && owner->tp.n_params != tp.n_params)
        return set_err(DF_ERR_HIP, "internal: the chain's trainers disagree on the parameter count");
    if (owner && hipDeviceSynchronize() != hipSuccess) return set_err(DF_ERR_HIP, "hipDeviceSynchronize");
    if (nb > 0 && (hipMemcpy(t->d_params.get(), owner ? owner->d_params.get() : (const void*)P.trainables.data(), nb,
                             owner ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemset(t->d_m.get(), 0, nb) != hipSuccess || hipMemset(t->d_v.get(), 0, nb) != hipSuccess ||
                   hipMemset(t->d_grad.get(), 0, nb) != hipSuccess))
        return set_err(DF_ERR_HIP, "initialising the training state failed");
    // (after every allocation a plain-Adam trainer makes: theirs keep their places)
    if (tp.chain_mode && (rc = setup_chain(t)) != DF_OK) return rc;
    // The blobs uploaded above were planned from the host copy, which is behind a live owner's
    // parameters: regather them (every map: tests/test_repack_closure.py shows the regather is
    // complete).  The chain's own blobs get the bytes they hold already.
    if (owner) {
        if ((rc = repack(t, nullptr)) != DF_OK) return rc;
        if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_err(e, "repack");
    }
    guard.release();
    *out = t;
    return DF_OK;
}

int df_train_num_params(const df_train* t, int64_t* count) {
    if (!t || !count) return set_err(DF_ERR_INVALID, "null pointer");
    *count = t->tp.n_params;
    return DF_OK;
}

int df_train_sweep(const df_train* t, int* form) {
    if (!t || !form) return set_err(DF_ERR_INVALID, "null pointer");
    if (!t->tp.layerwise) *form = DF_SWEEP_FUSED;
    else if (t->cap == 0)  // no gradient yet: the form ensure_capacity will try first
        *form = t->fmode ? DF_SWEEP_H0FREE
                         : (t->c->plan.uniform || t->tp.sweep_req == DF_SWEEP_RECOMPUTE) ? DF_SWEEP_RECOMPUTE
                                                                                                  : DF_SWEEP_KEPT;
    else if (h0free(t)) *form = DF_SWEEP_H0FREE;
    else *form = t->hsave_on ? DF_SWEEP_KEPT : DF_SWEEP_RECOMPUTE;
    if (t->tp.layerwise && t->tp.separate) *form |= DF_SWEEP_SEPARATE;
    return DF_OK;
}

int df_train_grad_ptr(df_train* t, float** grad_dev) {
    if (!t || !grad_dev) return set_err(DF_ERR_INVALID, "null pointer");
    *grad_dev = t->d_grad.as<float>();
    return DF_OK;
}

int df_train_set_theta_input(df_train* t, int mode) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (mode != DF_THETA_AUTO && mode != DF_THETA_RAW && mode != DF_THETA_GIVEN)
        return set_err(DF_ERR_INVALID, "θ input mode must be DF_THETA_AUTO, DF_THETA_RAW or DF_THETA_GIVEN");
    t->theta_input = mode;
    return DF_OK;
}

int df_train_gradient(df_train* t, const float* x, const float* theta_raw, int64_t batch, int64_t n_total,
                      double* logpdf_sum, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (n_total < batch || n_total < 1) return set_err(DF_ERR_INVALID, "n_total must be >= batch and >= 1");
    return gradient(t, x, theta_raw, nullptr, batch, n_total, 0.0, logpdf_sum, stream);
}

int df_train_gradient_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                        double w_total, double* wsums, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (!(w_total >= 0.0)) return set_err(DF_ERR_INVALID, "w_total must be 0 (this batch's own sum) or > 0");
    if (batch > 0 && !w) return set_err(DF_ERR_INVALID, "null weight array");
    DeviceGuard gd(t->c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    if (!wsums) {
        if (!t->d_wsums.get() && t->d_wsums.alloc(2 * sizeof(double)) != hipSuccess)
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (weighted sums)");
        wsums = t->d_wsums.as<double>();
    }
    if (batch == 0) {
        hipStream_t st = static_cast<hipStream_t>(stream);
        hipError_t e = hipMemsetAsync(t->d_grad.get(), 0, sizeof(float) * t->tp.n_params, st);
        if (e == hipSuccess) e = hipMemsetAsync(wsums, 0, 2 * sizeof(double), st);
        t->last_lp = wsums;
        t->last_ws = wsums;
        return e == hipSuccess ? DF_OK : hip_err(e, "hipMemsetAsync");
    }
    return gradient(t, x, theta_raw, w, batch, batch, w_total, wsums, stream);
}

int df_train_logpdf_grad(df_train* t, const float* x, const float* theta, float* logpdf_out, float* grad_x,
                         float* grad_theta, int64_t batch, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (t->tp.layerwise)
        return set_err(DF_ERR_UNSUPPORTED,
                       "df_train_logpdf_grad needs a trainer on the fused sweep; this chain trains layer-wise "
                       "(a conditioner with hidden width > 64, more than one hidden Dense, or more than 4 "
                       "transformed dims in a layer)");
    if (batch == 0) return DF_OK;
    DeviceGuard gd(t->c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    return score_sweep(t, x, theta, logpdf_out, grad_x, grad_theta, batch, -1, static_cast<hipStream_t>(stream));
}

}  // extern "C"

int df::api::score_sweep(df_train* t, const float* x, const float* theta, float* logpdf_out, float* grad_x,
                         float* grad_theta, int64_t batch, int flow_req, hipStream_t st) {
    void* const stream = st;
    if (!x) return set_err(DF_ERR_INVALID, "null input array");
    df_chain* c = t->c;
    const Plan& P = c->plan;
    if (P.n > 0 && !theta)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    const int tf = P.n == 0 ? 0 : flow_req >= 0 ? (flow_req == 1 && !c->has_bounds ? -1 : flow_req) : theta_flow(t);
    if (tf < 0) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds) for DF_THETA_RAW");
    const bool flow = tf == 1;
    if (P.n == 0) grad_theta = nullptr;
    if (!grad_x && !grad_theta) {  // logpdf alone: the inverse pass without the kept outputs
        if (!logpdf_out) return DF_OK;
        return run(c, MODE_LOGPDF, flow, x, theta, nullptr, nullptr, logpdf_out, nullptr, batch, stream);
    }
    if (t->score_grid == 0) {  // plan the launches: LDS against the workgroup's limit, resident grid
        std::vector<ScoreOp> plan;
        int occ = 0;
        for (size_t i = 0; i < t->tp.ops.size(); ++i) {
            const SweepOp& op = t->tp.ops[i];
            ScoreOp so{op.layer, op.net, -1, op.phase, 0};
            if (op.net >= 0) {
                so.lds = score_net_lds(t->tp.nets[op.net]);
                if (so.lds > kScoreLdsMax)
                    return set_err(DF_ERR_UNSUPPORTED,
                                   "df_train_logpdf_grad: a conditioner needs more than 160 KiB of LDS");
                // an RNVP layer's s-net and t-net (consecutive ops) of the same depth: one launch
                if (!t->score_per_net && op.phase == TR_PHASE_S && i + 1 < t->tp.ops.size() &&
                    t->tp.ops[i + 1].layer == op.layer && t->tp.ops[i + 1].net >= 0 &&
                    t->tp.net_nh[t->tp.ops[i + 1].net] == t->tp.net_nh[op.net] &&
                    so.lds + score_net_lds(t->tp.nets[t->tp.ops[i + 1].net]) <= kScoreLdsMax) {
                    so.net2 = t->tp.ops[i + 1].net;
                    so.lds += score_net_lds(t->tp.nets[so.net2]);
                    ++i;
                }
                int b = 0;
                hipError_t eo = score_net_occupancy(P.ht, t->tp.net_nh[so.net], t->tp.amode, so.net2 >= 0, so.lds, &b);
                if (eo != hipSuccess) return hip_err(eo, "hipOccupancyMaxActiveBlocksPerMultiprocessor(score)");
                occ = occ == 0 ? b : std::min(occ, b);
            }
            plan.push_back(so);
        }
        t->score_ops.swap(plan);
        t->score_grid = std::max(1, c->grid_cus * std::max(1, occ));
        if (c->debug_launch)
            std::fprintf(stderr, "[df] logpdf_grad: %zu launches (%s), %d workgroups of %d waves per CU, grid %d\n",
                         t->score_ops.size(), t->score_per_net ? "per net" : "per layer", occ, kScoreWaves,
                         t->score_grid);
    }
    int rc = ensure_capacity(t, batch);
    if (rc != DF_OK) return rc;
    float* snap = t->bb.d_snap.as<float>();
    const float* bounds = c->d_bounds.as<const float>();

    // 1. inverse pass keeping every layer's output (U[li] = snap[li], U[0] = z); lp per sample
    rc = run(c, MODE_LOGPDF, flow, x, theta, nullptr, nullptr, logpdf_out, nullptr, batch, stream, snap);
    if (rc != DF_OK) return rc;
    // 2. z̄ = ∂logpdf(MvNormal(0,I), z)/∂z = -z.  grad_x has z̄'s layout ([sample][d]): the
    //    sweep runs in it, and what is left after the last layer is ∂lp/∂x
    float* zbar = grad_x ? grad_x : t->bb.d_zbar.as<float>();
    hipError_t e = launch_scale(zbar, snap, -1.f, batch * P.d, st);
    if (e != hipSuccess) return hip_err(e, "scale kernel launch");
    // θ̄ accumulates in grad_theta ([sample][n]) over the nets that read θ
    if (grad_theta) {
        e = hipMemsetAsync(grad_theta, 0, sizeof(float) * (size_t)batch * P.n, st);
        if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    }
    // 3. reverse sweep, chain order
    const int64_t ntiles = (batch + 15) / 16;
    const int grid = (int)std::min<int64_t>(t->score_grid, (ntiles + kScoreWaves - 1) / kScoreWaves);
    for (const ScoreOp& op : t->score_ops) {
        if (op.net < 0) {
            e = norm_adjoint(t, op.layer, zbar, batch, st);
            if (e != hipSuccess) return hip_err(e, "norm adjoint launch");
            continue;
        }
        ScoreArgs a{};
        fill_layer_args(a, t, op.layer, op.phase, x, theta, flow, batch);
        a.zbar = zbar;
        a.thbar = grad_theta;
        a.ebuf = t->bb.d_ebuf.as<float>();
        a.blob = c->d_blob.as<const uint8_t>();
        a.tblob = t->d_tblob.as<const uint8_t>();
        a.net = t->tp.nets[op.net];
        if (op.net2 >= 0) a.net2 = t->tp.nets[op.net2];
        e = launch_score_net(P.ht, t->tp.net_nh[op.net], t->tp.amode, op.net2 >= 0, a, (unsigned)grid, op.lds, st);
        if (e != hipSuccess) return hip_err(e, "score kernel launch");
    }
    // 4. raw θ: the chain rule of normalize_input
    if (grad_theta && flow) {
        e = launch_score_theta_raw(grad_theta, bounds, bounds + P.n, P.n, batch, st);
        if (e != hipSuccess) return hip_err(e, "θ gradient scaling launch");
    }
    return DF_OK;
}

extern "C" {

int df_train_apply(df_train* t, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    DeviceGuard gd(t->c->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (t->debug && t->last_lp) {  // train!(...; debug=true), src/Flows.jl:404-409
        // (a weighted gradient left {Σ w·lp, W}: its loss is over W, and W <= 0 is refused too)
        double s[2] = {0.0, 0.0};
        const bool wt = t->last_ws != nullptr;
        hipError_t e = hipMemcpyAsync(s, t->last_lp, (wt ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_err(e, "debug loss read-back");
        const double l = wt ? (s[1] > 0.0 ? -s[0] / s[1] : std::nan(""))
                            : -s[0] / (double)(t->last_n > 0 ? t->last_n : 1);
        if (!std::isfinite(l)) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "non-finite training loss %g: parameters not updated", l);
            return set_err(DF_ERR_NONFINITE, msg);
        }
    }
    hipError_t e = hipSuccess;
    if (t->tp.chain_mode) {
        // Σ dx² per tensor for the ClipNorm (the rules before it applied on the fly), then
        // the whole chain per element in one kernel
        if (t->tp.och_clip >= 0) {
            e = launch_tensor_sumsq(t->d_grad.as<const float>(), t->d_params.as<const float>(),
                                    t->d_toff.as<const int32_t>(), (int)t->tp.toff.size() - 1, t->och, t->tp.och_clip,
                                    false,                                     t->d_sumsq.as<float>(), st);
            if (e != hipSuccess) return hip_err(e, "tensor norm kernel launch");
        }
        e = launch_opt_chain(t->d_params.as<float>(), t->d_grad.as<const float>(), t->d_m.as<float>(),
                             t->d_v.as<float>(), t->d_bt.as<float>(), t->d_sumsq.as<const float>(),
                             t->d_oblocks.as<const OptBlock>(), (int64_t)t->tp.oblocks.size(), t->och, st);
        if (e != hipSuccess) return hip_err(e, "optimiser chain kernel launch");
        return repack(t, st);
    }
    e = launch_adam(t->d_params.as<float>(), t->d_grad.as<const float>(), t->d_m.as<float>(), t->d_v.as<float>(),
                    t->tp.n_params, t->opt.eta, t->opt.beta1, t->opt.beta2, t->opt.epsilon, t->d_bt.as<float>(), st);
    if (e != hipSuccess) return hip_err(e, "Adam kernel launch");
    return repack(t, st);
}

int df_train_step(df_train* t, const float* x, const float* theta_raw, int64_t batch, double* logpdf_sum,
                  void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch == 0) return DF_OK;
    int rc = df_train_gradient(t, x, theta_raw, batch, batch, logpdf_sum, stream);
    return rc != DF_OK ? rc : df_train_apply(t, stream);
}

int df_train_step_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                    double* wsums, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch == 0) return DF_OK;
    int rc = df_train_gradient_w(t, x, theta_raw, w, batch, 0.0, wsums, stream);
    return rc != DF_OK ? rc : df_train_apply(t, stream);
}

int df_train_step_graph(df_train* t, const float* x, const float* theta_raw, int64_t batch, int64_t n_total,
                        double* logpdf_sum, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch == 0) return DF_OK;
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (n_total < batch) return set_err(DF_ERR_INVALID, "n_total must be >= batch and >= 1");
    return step_graph(t, x, theta_raw, nullptr, batch, n_total, 0.0, logpdf_sum, stream);
}

int df_train_step_graph_w(df_train* t, const float* x, const float* theta_raw, const float* w, int64_t batch,
                          double w_total, double* wsums, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch == 0) return DF_OK;
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (!(w_total >= 0.0)) return set_err(DF_ERR_INVALID, "w_total must be 0 (this batch's own sum) or > 0");
    if (!w) return set_err(DF_ERR_INVALID, "null weight array");
    return step_graph(t, x, theta_raw, w, batch, batch, w_total, wsums, stream);
}

int df_batch_gather(float* x_out, float* theta_out, const float* x_set, const float* theta_set, int d, int n,
                    int64_t n_samples, const int32_t* order, int64_t first, int64_t count, void* stream) {
    if (d < 1 || n < 0) return set_err(DF_ERR_INVALID, "df_batch_gather: d >= 1 and n >= 0");
    if (count < 0 || n_samples < 0) return set_err(DF_ERR_SHAPE, "negative sample count");
    if (n_samples >= (int64_t)1 << 31) return set_err(DF_ERR_SHAPE, "a resident set holds fewer than 2^31 samples");
    if (first < 0 || first + count > n_samples)
        return set_err(DF_ERR_INVALID, "df_batch_gather: [first, first + count) must lie inside [0, n_samples)");
    if (count == 0) return DF_OK;
    if (!x_out || !x_set || (n > 0 && (!theta_out || !theta_set))) return set_err(DF_ERR_INVALID, "null array");
    const hipError_t e = launch_batch_gather(x_out, theta_out, x_set, theta_set, d, n, n_samples, order, first,
                                             nullptr, 0, count, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DF_OK : hip_err(e, "batch gather launch");
}

// df_train_epoch, and df_train_epoch_w (weighted: w_set is read, the steps are epoch_step_w in
// the weighted graph slots, step_sums takes two doubles per step).
static int epoch(df_train* t, const float* x_set, const float* theta_set, const float* w_set, bool weighted,
                 int64_t n_samples, const int32_t* order, int64_t batchsize, double* step_logpdf_sum,
                 int64_t* steps_done, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (steps_done) *steps_done = 0;
    if (batchsize <= 0) return set_err(DF_ERR_INVALID, "batchsize must be >= 1");
    if (n_samples < 0) return set_err(DF_ERR_SHAPE, "negative sample count");
    if (n_samples == 0) return DF_OK;
    if (n_samples >= (int64_t)1 << 31) return set_err(DF_ERR_SHAPE, "a resident set holds fewer than 2^31 samples");
    if (!x_set) return set_err(DF_ERR_INVALID, "null input array");
    if (weighted && !w_set) return set_err(DF_ERR_INVALID, "null weight array");
    df_chain* c = t->c;
    const Plan& P = c->plan;
    if (P.n > 0 && !theta_set)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    if (theta_flow(t) < 0)
        return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds) for DF_THETA_RAW");
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!t->d_cursor.get() && t->d_cursor.alloc(16) != hipSuccess)
        return set_err(DF_ERR_NOMEM, "hipMalloc failed (epoch cursor)");
    int64_t* cursor = t->d_cursor.as<int64_t>();

    // the one synchronisation of the call: an order is checked before any step is enqueued
    if (order) {
        int* d_bad = reinterpret_cast<int*>(cursor + 1);
        int bad = 0;
        hipError_t e = launch_order_range(order, n_samples, d_bad, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_err(e, "order check");
        if (bad > 0) {
            char msg[128];
            std::snprintf(msg, sizeof msg, "df_train_epoch: %d of the %lld order entries lie outside [0, n_samples)",
                          bad, (long long)n_samples);
            return set_err(DF_ERR_INVALID, msg);
        }
    }

    // staging for one mini-batch; the captured steps name it and everything in the key
    const int64_t full = std::min(batchsize, n_samples);
    const EpochKey key{x_set, theta_set, order, step_logpdf_sum, n_samples, batchsize, w_set};
    StepGraph* const eg = weighted ? t->egw : t->eg;
    int64_t* const eg_count = weighted ? t->egw_count : t->eg_count;
    EpochKey& ekey = weighted ? t->ekeyw : t->ekey;
    if (full > t->ecap) {
        for (StepGraph& g : t->eg) drop(g);
        for (StepGraph& g : t->egw) drop(g);
        t->ecap = 0;
        if (t->d_ex.alloc(sizeof(float) * (size_t)full * P.d) != hipSuccess ||
            (P.n > 0 && t->d_eth.alloc(sizeof(float) * (size_t)full * P.n) != hipSuccess))
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (mini-batch staging)");
        t->ecap = full;
    }
    if (weighted && full > t->ewcap) {  // (the weights' staging comes with the first weighted epoch)
        for (StepGraph& g : t->egw) drop(g);
        t->ewcap = 0;
        if (t->d_ew.alloc(sizeof(float) * (size_t)t->ecap) != hipSuccess)
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (mini-batch staging)");
        t->ewcap = t->ecap;
    }
    if (!(key == ekey))
        for (int k = 0; k < 2; ++k) drop(eg[k]);
    ekey = key;

    hipError_t e = hipMemsetAsync(cursor, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    const int64_t steps = (n_samples + batchsize - 1) / batchsize;
    for (int64_t i = 0; i < steps; ++i) {
        const int64_t count = std::min(batchsize, n_samples - i * batchsize);
        // as df_train_step_graph runs its step; a slot captured for another count is dropped first.
        // Debug mode: the per-step loss check synchronises, so the steps run eagerly
        const int slot = count == full ? 0 : 1;
        if (eg_count[slot] != count) drop(eg[slot]);
        eg_count[slot] = count;
        auto step = [&](hipStream_t on) { return weighted ? epoch_step_w(t, count, on) : epoch_step(t, count, on); };
        const int rc = t->debug ? step(st) : run_captured(t, eg[slot], st, "epoch step", step);
        if (rc != DF_OK) {
            if (steps_done) *steps_done = i;
            return rc;
        }
    }
    if (steps_done) *steps_done = steps;
    return DF_OK;
}

int df_train_epoch(df_train* t, const float* x_set, const float* theta_set, int64_t n_samples, const int32_t* order,
                   int64_t batchsize, double* step_logpdf_sum, int64_t* steps_done, void* stream) {
    return epoch(t, x_set, theta_set, nullptr, false, n_samples, order, batchsize, step_logpdf_sum, steps_done, stream);
}

int df_train_epoch_w(df_train* t, const float* x_set, const float* theta_set, const float* w_set, int64_t n_samples,
                     const int32_t* order, int64_t batchsize, double* step_wsums, int64_t* steps_done, void* stream) {
    return epoch(t, x_set, theta_set, w_set, true, n_samples, order, batchsize, step_wsums, steps_done, stream);
}

int df_batch_gather_w(float* x_out, float* theta_out, float* w_out, const float* x_set, const float* theta_set,
                      const float* w_set, int d, int n, int64_t n_samples, const int32_t* order, int64_t first,
                      int64_t count, void* stream) {
    if (d < 1 || n < 0) return set_err(DF_ERR_INVALID, "df_batch_gather_w: d >= 1 and n >= 0");
    if (count < 0 || n_samples < 0) return set_err(DF_ERR_SHAPE, "negative sample count");
    if (n_samples >= (int64_t)1 << 31) return set_err(DF_ERR_SHAPE, "a resident set holds fewer than 2^31 samples");
    if (first < 0 || first + count > n_samples)
        return set_err(DF_ERR_INVALID, "df_batch_gather_w: [first, first + count) must lie inside [0, n_samples)");
    if (count == 0) return DF_OK;
    if (!x_out || !x_set || !w_out || !w_set || (n > 0 && (!theta_out || !theta_set)))
        return set_err(DF_ERR_INVALID, "null array");
    const hipError_t e = launch_batch_gather_w(x_out, theta_out, w_out, x_set, theta_set, w_set, d, n, n_samples, order,
                                               first, nullptr, 0, count, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DF_OK : hip_err(e, "batch gather launch");
}

static int logpdf_wsum(df_chain* c, bool flow, const float* x, const float* theta, const float* w, int64_t batch,
                       double* wsums, void* stream) {
    if (!c) return set_err(DF_ERR_INVALID, "null chain");
    if (!wsums) return set_err(DF_ERR_INVALID, "null sum output");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        const hipError_t e = hipMemsetAsync(wsums, 0, 2 * sizeof(double), st);
        return e == hipSuccess ? DF_OK : hip_err(e, "hipMemsetAsync");
    }
    if (!w) return set_err(DF_ERR_INVALID, "null weight array");
    if (batch > c->wlp_cap) {
        c->wlp_cap = 0;
        const int64_t cap = std::max<int64_t>(batch, 1024);
        if (c->d_wlp.alloc(sizeof(float) * cap) != hipSuccess ||
            c->d_wlp_part.alloc(sizeof(double) * wsum_parts(cap)) != hipSuccess)
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (weighted logpdf workspace)");
        c->wlp_cap = cap;
    }
    float* lp = c->d_wlp.as<float>();
    double* part = c->d_wlp_part.as<double>();
    const int rc = run(c, MODE_LOGPDF, flow, x, theta, nullptr, nullptr, lp, nullptr, batch, stream);
    if (rc != DF_OK) return rc;
    hipError_t e = launch_weighted_lp_sum(w, lp, batch, part, wsums, st);
    if (e == hipSuccess) e = launch_weighted_lp_sum(w, nullptr, batch, part, wsums + 1, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "weighted sum launch");
}

int df_flow_logpdf_wsum(df_chain* c, const float* x, const float* theta_raw, const float* w, int64_t batch,
                        double* wsums, void* stream) {
    return logpdf_wsum(c, true, x, theta_raw, w, batch, wsums, stream);
}

int df_chain_logpdf_wsum(df_chain* c, const float* x, const float* theta, const float* w, int64_t batch,
                         double* wsums, void* stream) {
    return logpdf_wsum(c, false, x, theta, w, batch, wsums, stream);
}

int df_train_set_debug(df_train* t, int on) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    t->debug = on != 0;
    return DF_OK;
}

int df_train_get_params(df_train* t, float* host_out, int64_t count) {
    if (!t || (!host_out && count > 0)) return set_err(DF_ERR_INVALID, "null pointer");
    if (count != t->tp.n_params) return set_err(DF_ERR_SHAPE, "count must equal df_train_num_params");
    DeviceGuard gd(t->c->device);
    if (count == 0) return DF_OK;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, t->d_params.get(), sizeof(float) * count, hipMemcpyDeviceToHost);
    return e == hipSuccess ? DF_OK : hip_err(e, "hipMemcpy(params)");
}

int df_train_set_params(df_train* t, const float* host_in, int64_t count) {
    if (!t || (!host_in && count > 0)) return set_err(DF_ERR_INVALID, "null pointer");
    if (count != t->tp.n_params) return set_err(DF_ERR_SHAPE, "count must equal df_train_num_params");
    DeviceGuard gd(t->c->device);
    if (count == 0) return DF_OK;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(t->d_params.get(), host_in, sizeof(float) * count, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_err(e, "hipMemcpy(params)");
    int rc = repack(t, nullptr);
    if (rc != DF_OK) return rc;
    e = hipDeviceSynchronize();
    return e == hipSuccess ? DF_OK : hip_err(e, "repack");
}

int df_train_adjust(df_train* t, float eta) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (!(eta >= 0.f)) return set_err(DF_ERR_INVALID, "invalid learning rate (η >= 0)");
    t->och.p[t->tp.och_eta][0] = eta;
    if (t->och.kind[t->tp.och_eta] == DF_OPT_ADAM) t->opt.eta = eta;
    t->cap_gen++;  // η is a kernel argument of the captured steps: they are re-captured
    return DF_OK;
}

int df_train_num_tensors(const df_train* t, int64_t* count) {
    if (!t || !count) return set_err(DF_ERR_INVALID, "null pointer");
    *count = (int64_t)t->tp.toff.size() - 1;
    return DF_OK;
}

int df_train_tensor_offsets(const df_train* t, int64_t* offsets_out, int64_t count_plus_1) {
    if (!t || !offsets_out) return set_err(DF_ERR_INVALID, "null pointer");
    if (count_plus_1 != (int64_t)t->tp.toff.size())
        return set_err(DF_ERR_SHAPE, "count_plus_1 must equal df_train_num_tensors + 1");
    for (size_t k = 0; k < t->tp.toff.size(); ++k) offsets_out[k] = t->tp.toff[k];
    return DF_OK;
}

int df_train_grad_norms(df_train* t, float* out_dev, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    const int nt = (int)t->tp.toff.size() - 1;
    if (nt == 0) return DF_OK;
    if (!out_dev) return set_err(DF_ERR_INVALID, "null output array");
    DeviceGuard gd(t->c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    const int rc = ensure_toff(t);
    if (rc != DF_OK) return rc;
    const hipError_t e =
        launch_tensor_sumsq(t->d_grad.as<const float>(), t->d_params.as<const float>(), t->d_toff.as<const int32_t>(),
                            nt, t->och, 0, true, out_dev, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DF_OK : hip_err(e, "tensor norm kernel launch");
}

}  // extern "C"

namespace df {
namespace api {
int train_device(const df_train* t) { return t ? t->c->device : -1; }
double* train_last_lpsum(df_train* t) { return t ? const_cast<double*>(t->last_lp) : nullptr; }
}  // namespace api
}  // namespace df
