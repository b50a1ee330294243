// df_train_capi.hip — the training entry points of the C ABI (df_train_*).
//
// Host side of one train! step (src/Flows.jl:396-414); the device work is in
// df_train.hip / df_train_impl.h, the inverse pass with per-layer outputs in
// the specialised chain kernel (df_uniform_impl.h, ChainArgs::snap).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "df_handle.h"
#include "df_ltrain.h"
#include "df_pack.h"
#include "df_train.h"

using namespace df;
using namespace df::api;

namespace {

struct SweepOp {
    int layer;   // index in plan.layers
    int net;     // index in df_train::nets, -1 for a NormalizationLayer
    int phase;   // TR_PHASE_S / TR_PHASE_T
};

// One launch of df_train_logpdf_grad's sweep.
struct ScoreOp {
    int layer;   // index in plan.layers
    int net;     // index in df_train::nets (pair: the s-net), -1 for a NormalizationLayer
    int net2;    // pair: the t-net, else -1
    int phase;
    size_t lds;
};

int round16(int v) { return (v + 15) / 16 * 16; }

int pow2_tiles(int rows) {
    int t = 1;
    while (16 * t < rows) t *= 2;
    return t;
}

// Layer-wise path: one packed GEMM operand (W or Wᵀ) of one Dense.
struct LOp {
    int mt = 0;              // output row tiles (power of two <= 16)
    int nkq = 0;             // k-quads of the contraction
    int chunk_kq = 1;        // k-quads per LDS chunk
    int64_t frag = 0;        // byte offset in the layer-wise blob
    int64_t bias = -1;       // float offset of the padded bias (forward only)
    int64_t sfrag = -1;      // SPLIT planes [c][m][p][lane][8] in the split blob (Wᵀ of hidden-256 Denses)
};

struct LDense {
    int in_dim = 0, out_dim = 0, act = 0;
    int w_off = 0, b_off = -1;
    LOp fwd, bwd;            // acc = W·in (out rows) ; acc = Wᵀ·δ (in rows)
};

struct LNet {
    std::vector<LDense> dn;  // Dense(in,h,σ0), hidden..., Dense(h,out,σo)
    bool pre = false;        // a hidden σ needs its pre-activation for σ' (softplus, logcosh, swish):
                             // the sweep recomputes the net and stores σ'(x) beside H
};

// every activation the plan accepts has a derivative rule (df_train_impl.h act_grad/act_dx)
bool act_trainable(int a) { return a >= DF_ACT_IDENTITY && a <= DF_ACT_SWISH; }

bool act_needs_pre(int a) { return a == DF_ACT_SOFTPLUS || a == DF_ACT_LOGCOSH || a == DF_ACT_SWISH; }

}  // namespace

// One captured train step (df_train_step_graph): valid while the buffers it
// names are the ones it was captured with.
struct TrainGraph {
    const void* x = nullptr;
    const void* theta = nullptr;
    const void* lp = nullptr;
    int64_t batch = 0, n_total = 0, cap_gen = -1, partial_gen = -1;
    int flow = -1;                    // the θ convention it was recorded with (θ normalised in-kernel or not)
    int seen = 0;                     // eager runs with this key (captured on the second)
    hipGraphExec_t exec = nullptr;
    uint64_t last_use = 0;
};

// One captured step of df_train_epoch (gather, gradient, update, cursor advance): slot 0 the
// full batch, slot 1 the epoch's partial last batch.  Valid while the epoch's key
// (df_train::ekey) and the buffers it names stand.
struct EpochGraph {
    int64_t count = 0, cap_gen = -1, partial_gen = -1;
    int flow = -1;
    int seen = 0;                     // eager runs of this step (captured on the second)
    hipGraphExec_t exec = nullptr;
};

// What a captured epoch step names besides the trainer's own buffers.
struct EpochKey {
    const float* x_set = nullptr;
    const float* theta_set = nullptr;
    const int32_t* order = nullptr;
    const double* step_lp = nullptr;
    int64_t n_samples = 0, batchsize = 0;
    bool operator==(const EpochKey& o) const {
        return x_set == o.x_set && theta_set == o.theta_set && order == o.order && step_lp == o.step_lp &&
               n_samples == o.n_samples && batchsize == o.batchsize;
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
    df_adam opt{};
    DevBuf d_bt;                      // device βᵗ of the next update (Adam), [β1ᵗ, β2ᵗ]
    int64_t cap_gen = 0;              // bumped when the batch-sized buffers are reallocated
    hipStream_t cap_stream = nullptr; // capture stream of df_train_step_graph
    std::vector<TrainGraph> graphs;
    uint64_t use_clock = 0;
    int64_t P = 0;
    int amode = 0;                    // fused kernel activation mode (trn::AM_*)
    std::vector<GNet> nets;
    std::vector<int> net_nh;
    std::vector<SweepOp> ops;
    std::vector<uint8_t> tblob;
    std::vector<int32_t> tdst, tsrc;
    DevBuf d_params, d_m, d_v, d_grad, d_partial, d_lpsum;  // float [P] (d_partial: [grid][P]); double Σ logpdf
    DevBuf d_tblob;
    // every packed blob's regather from d_params, in launch order (df_train_create_ex)
    std::vector<RepackMap> maps;
    BatchBufs bb;
    bool debug = false;               // df_train_set_debug: refuse updates on a non-finite loss
    int theta_input = DF_THETA_AUTO;  // df_train_set_theta_input
    const double* last_lp = nullptr;  // Σ logpdf written by the last df_train_gradient
    int64_t last_n = 0;               // ... and the n_total it was taken over
    int64_t cap = 0;       // batch capacity of bb
    int grid = 0;          // workgroups of a full net launch (resident on the device)
    size_t lds_max = 0;
    // df_train_logpdf_grad (score_net_kernel), planned on the first call: one launch per
    // RNVP layer (both nets) where that fits, else per net; resident workgroups
    std::vector<ScoreOp> score_ops;
    int score_grid = 0;
    bool score_per_net = false;       // DF_SCORE_PER_NET=1 at df_train_create: per-net launches only (A/B)
    // layer-wise path (hidden width > 64, deep or wide-output conditioners)
    bool layerwise = false;
    std::vector<LNet> lnets;
    std::vector<uint8_t> lblob;      // fragments (W and Wᵀ) then padded biases
    std::vector<int32_t> ldst, lsrc; // repack map (float index ← trainables index)
    std::vector<uint8_t> tsblob;     // SPLIT W1ᵀ planes of the fused path (GNet::st_src)
    std::vector<int32_t> tsdst, tssrc; // repack map (byte offset ← trainables index·4 + plane)
    std::vector<uint8_t> lsblob;     // SPLIT planes of the layer-wise Wᵀ operands (LOp::sfrag)
    std::vector<int32_t> lsdst, lssrc; // repack map (byte offset ← trainables index·4 + plane)
    DevBuf d_tsblob, d_lsblob, d_lblob;
    int lgrid = 0;                   // workgroups of the dW kernels (partial rows)
    int lwidth = 16;                 // widest activation row (floats)
    int lmax_h = 1;                  // activation buffers needed (hidden Denses + 1)
    bool any_pre = false;
    bool hsave_on = false;           // bb.d_hsave is in use
    // H0-free sweep (round 5; wide SPLIT chains of relu hidden-256 nets, DF_SWEEP_H0FREE): the
    // inverse pass keeps each net's features vcat(θ, u)[axis_nn] ([layer·2 + net][B][32])
    // and H1 only (d_hsave with one slot per net); the split dW1 recomputes H0 from the
    // features and writes its relu mask (d_hmask, 1 KiB per 32 samples) for the W1ᵀδ1 epilogue
    bool fmode = false;
    int sweep_req = DF_SWEEP_AUTO;   // df_train_create_ex: the requested form (df_sweep_form)
    bool separate = false;           // DF_SWEEP_SEPARATE: unmerged dW / front launches
    // The parameter tensors (one Dense weight or bias each) as slices of the flat vectors:
    // tensor k is [toff[k], toff[k+1]).  On the device (d_toff) once a kernel needs them.
    std::vector<int32_t> toff;
    DevBuf d_toff;
    // Optimiser chain (df_train_create_opt).  A chain that is exactly [Adam] is not one:
    // chain_mode stays false and df_train_apply launches adam_kernel with `opt`.
    bool chain_mode = false;
    OptChain och{};
    int och_clip = -1;               // index of the chain's ClipNorm (-1: none): the rules before it
                                     //   run inside the Σ dx² kernel too
    int och_eta = -1;                // the rule df_train_adjust sets η of: the Adam, else the first Descent
    DevBuf d_sumsq, d_oblocks;       // float [tensors] Σ dx²; OptBlock [n_oblocks] of the update kernel
    int64_t n_oblocks = 0;
    // df_train_epoch: the mini-batch staging buffers ((d, ecap) and (n, ecap), sized at the
    // first use of a batchsize, only growing), the device cursor (int64 step index, then the
    // int count of order_range_kernel) and the two captured steps, in slots of their own
    DevBuf d_ex, d_eth, d_cursor;
    int64_t ecap = 0;
    EpochKey ekey;
    EpochGraph eg[2];
};

namespace {

// the H0-free sweep is planned and its buffers fit (ensure_capacity)
bool h0free(const df_train* t) { return t->fmode && t->hsave_on && t->bb.d_fsave.get(); }

// The captured graphs and their stream (the device buffers free themselves with the handle).
void free_all(df_train* t) {
    for (TrainGraph& g : t->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    t->graphs.clear();
    for (EpochGraph& g : t->eg) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        g = EpochGraph{};
    }
    if (t->cap_stream) (void)hipStreamDestroy(t->cap_stream);
    t->cap_stream = nullptr;
}

// Append the SPLIT planes [c][m][p][lane][8] of a Wᵀ (rows × kdim, mt row tiles, 32 k per
// chunk; Wᵀ[i, k] = W[k, i] with W column-major, leading dimension ldw, at w_off of the
// trainables) to blob, and (byte offset ← trainables index·4 + plane) to its repack map.
// Returns the planes' byte offset in blob.
int64_t pack_wt_planes(const Plan& P, int rows, int kdim, int mt, int chunks, int64_t w_off, int ldw,
                       std::vector<uint8_t>& blob, std::vector<int32_t>& dst, std::vector<int32_t>& src) {
    const int64_t base = (int64_t)blob.size();
    blob.resize(blob.size() + (size_t)chunks * mt * 3072, 0);
    pack::ParamSink<uint8_t> sink(blob, dst, src, pack::ParamSink<uint8_t>::PLANES);
    pack::for_each_plane_frag(0, chunks, 0, mt, pack::k_plane_hidden, [&](int64_t pos, int i, int k, int p) {
        if (i >= rows || k >= kdim) return;
        const int32_t from = (int32_t)(w_off + k + (int64_t)ldw * i);
        sink.plane(base + pos, p, {from, P.trainables[from]});
    });
    return base;
}

// Pack A = W (transposed = false: rows = out, k = in) or Wᵀ (rows = in, k = out)
// as fragments [kq][m][lane][4]: A[16m + (lane&15)][16kq + 4(lane>>4) + r].
LOp pack_lop(df_train* t, const Plan& P, const LDense& D, bool transposed) {
    LOp op;
    const int rows = transposed ? D.in_dim : D.out_dim;
    const int kdim = transposed ? D.out_dim : D.in_dim;
    op.mt = pow2_tiles(rows);
    op.nkq = (kdim + 15) / 16;
    op.chunk_kq = std::max(1, kLChunkBytes / (op.mt * 1024));
    op.frag = (int64_t)t->lblob.size();
    const size_t bytes = (size_t)op.nkq * op.mt * 1024;
    t->lblob.resize(t->lblob.size() + bytes, 0);
    pack::ParamSink<uint8_t> sink(t->lblob, t->ldst, t->lsrc, pack::ParamSink<uint8_t>::WORDS);
    pack::for_each_f32_frag(0, op.nkq, op.mt, pack::k_hidden_quad, [&](int64_t q, int i, int k) {
        if (i >= rows || k >= kdim) return;
        const int orow = transposed ? k : i, icol = transposed ? i : k;  // W[orow, icol]
        const int32_t src = (int32_t)(D.w_off + orow + (int64_t)D.out_dim * icol);
        sink.f32(op.frag + 4 * q, {src, P.trainables[src]});
    });
    // SPLIT planes of a hidden-256 Wᵀ (the ldense_kernel SPLIT instances), and of a first
    // Dense's W0ᵀ over a 256-wide hidden layer (≤ 64 conditioner inputs: the x̄ product
    // of the SPLIT W1ᵀδ1 epilogue)
    if (transposed && (op.mt == 16 || (op.mt <= 4 && op.nkq == 16)) && op.nkq % 2 == 0 && !t->c->exact)
        op.sfrag = pack_wt_planes(P, rows, kdim, op.mt, op.nkq / 2, D.w_off, D.out_dim, t->lsblob, t->lsdst, t->lssrc);
    return op;
}

void pack_lbias(df_train* t, const Plan& P, const LDense& D, LOp& op) {
    if (D.b_off < 0) return;
    op.bias = (int64_t)t->lblob.size() / 4;
    t->lblob.resize(t->lblob.size() + (size_t)op.mt * 64, 0);
    float* f = reinterpret_cast<float*>(t->lblob.data()) + op.bias;
    for (int r = 0; r < D.out_dim; ++r) {
        f[r] = P.trainables[D.b_off + r];
        t->ldst.push_back((int32_t)(op.bias + r));
        t->lsrc.push_back(D.b_off + r);
    }
}

int build_lnets(df_train* t) {
    const Plan& P = t->c->plan;
    t->ops.clear();
    t->lnets.clear();
    for (int li = 0; li < P.n_layers; ++li) {
        const DevLayer& L = P.layers[li];
        if (L.kind == DF_LAYER_NORM) {
            t->ops.push_back({li, -1, TR_PHASE_T});
            continue;
        }
        auto add = [&](int d0, int nd, int phase) -> int {
            LNet net;
            for (int k = 0; k < nd; ++k) {
                const DevDense& DD = P.denses[d0 + k];
                if (!act_trainable(DD.act))
                    return set_err(DF_ERR_UNSUPPORTED, "unknown activation");
                LDense D;
                D.in_dim = DD.in_dim;
                D.out_dim = DD.n_out;
                D.act = DD.act;
                D.w_off = DD.w_off;
                D.b_off = DD.b_off;
                D.fwd = pack_lop(t, P, D, false);
                pack_lbias(t, P, D, D.fwd);
                D.bwd = pack_lop(t, P, D, true);
                t->lwidth = std::max({t->lwidth, 16 * D.fwd.mt, 16 * D.bwd.mt});
                if (k + 1 < nd && act_needs_pre(D.act)) net.pre = true;
                net.dn.push_back(D);
            }
            t->lmax_h = std::max(t->lmax_h, nd - 1);
            t->any_pre = t->any_pre || net.pre;
            t->lnets.push_back(net);
            t->ops.push_back({li, (int)t->lnets.size() - 1, phase});
            return DF_OK;
        };
        int rc = DF_OK;
        if (L.kind == DF_LAYER_RNVP) rc = add(L.s_dense0, L.s_ndense, TR_PHASE_S);
        if (rc == DF_OK) rc = add(L.t_dense0, L.t_ndense, TR_PHASE_T);
        if (rc != DF_OK) return rc;
    }
    t->lblob.resize(t->lblob.size() + 16, 0);
    return DF_OK;
}

// Transposed fragments of one net (W0ᵀ, W_hᵀ) appended to t->tblob with
// their trainables index map.
void pack_transposed(df_train* t, const Plan& P, GNet& g, const DevDense& D0, const DevDense* D1, int ht) {
    const int h = g.h_true;
    const size_t base = t->tblob.size();
    g.t_src = (int64_t)base;
    g.off_w0t = 0;
    g.off_ht = ht * 1024;
    const int bytes = ht * 1024 + (D1 ? ht * ht * 1024 : 0);
    g.t_bytes = bytes;
    t->tblob.resize(base + bytes, 0);
    float* f = reinterpret_cast<float*>(t->tblob.data() + base);
    const int64_t f0 = (int64_t)base / 4;
    auto put = [&](int64_t q, int64_t src) {
        f[q] = P.trainables[src];
        t->tdst.push_back((int32_t)(f0 + q));
        t->tsrc.push_back((int32_t)src);
    };
    // W0ᵀ: [kq][lane (i,g)][r] = W0[16kq + 4g + r, i]
    for (int kq = 0; kq < ht; ++kq)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int i = lane & 15, a = 16 * kq + 4 * (lane >> 4) + r;
                if (a < h && i < g.n_in) put((int64_t)(kq * 64 + lane) * 4 + r, D0.w_off + a + (int64_t)h * i);
            }
    if (D1) {  // W1ᵀ: [kq][m][lane (i,g)][r] = W1[16kq + 4g + r, 16m + i]
        const int64_t o = g.off_ht / 4;
        for (int kq = 0; kq < ht; ++kq)
            for (int m = 0; m < ht; ++m)
                for (int lane = 0; lane < 64; ++lane)
                    for (int r = 0; r < 4; ++r) {
                        const int a = 16 * kq + 4 * (lane >> 4) + r, b = 16 * m + (lane & 15);
                        if (a < h && b < h)
                            put(o + ((int64_t)(kq * ht + m) * 64 + lane) * 4 + r, D1->w_off + a + (int64_t)h * b);
                    }
    }
}

int build_nets(df_train* t) {
    const Plan& P = t->c->plan;
    if (!P.uniform || !P.outv)
        return set_err(DF_ERR_UNSUPPORTED,
                       "training needs every conditioner in the default _dflt_net shape (hidden width <= 64) "
                       "with <= 4 transformed dims per layer");
    const int ht = P.ht;
    for (int li = 0; li < P.n_layers; ++li) {
        const DevLayer& L = P.layers[li];
        if (L.kind == DF_LAYER_NORM) {
            t->ops.push_back({li, -1, TR_PHASE_T});
            continue;
        }
        const ULayer& U = P.ulayers[li];
        auto add = [&](const UNet& u0, int d0, int nd, int phase) -> int {
            if (u0.nh > 1) return set_err(DF_ERR_UNSUPPORTED, "training supports n_sublayers <= 2 (one hidden Dense)");
            const DevDense& D0 = P.denses[d0];
            const DevDense* D1 = u0.nh == 1 ? &P.denses[d0 + 1] : nullptr;
            const DevDense& DO = P.denses[d0 + nd - 1];
            for (int k = 0; k < nd; ++k)
                if (!act_trainable(P.denses[d0 + k].act))
                    return set_err(DF_ERR_UNSUPPORTED, "unknown activation");
            GNet g{};
            g.u = u0;
            g.n_in = D0.in_dim;
            g.h_true = D0.n_out;
            // the net's bytes inside its stage: [off_w0, end of the output GEMV block)
            int lo = u0.off_w0;
            lo = std::min(lo, u0.off_b0);
            if (u0.nh) lo = std::min(lo, u0.off_h);
            lo = std::min(lo, u0.off_out);
            const int hi = u0.off_out + round16((u0.n_out * 16 * ht + 4) * 4);
            g.fwd_src = P.stages[u0.stage].src_off + lo;
            g.fwd_bytes = round16(hi - lo);
            g.u.off_w0 -= lo;
            g.u.off_b0 -= lo;
            if (u0.nh) g.u.off_h -= lo;
            g.u.off_out -= lo;
            g.w_off[0] = D0.w_off;
            g.b_off[0] = D0.b_off;
            g.w_off[1] = D1 ? D1->w_off : D0.w_off;
            g.b_off[1] = D1 ? D1->b_off : -1;
            g.w_off[2] = DO.w_off;
            g.b_off[2] = DO.b_off;
            g.p_begin = D0.w_off;
            int end = 0;
            for (int k = 0; k < nd; ++k) {
                const DevDense& D = P.denses[d0 + k];
                end = std::max(end, D.w_off + D.in_dim * D.n_out);
                if (D.b_off >= 0) end = std::max(end, D.b_off + D.n_out);
            }
            g.p_count = end - g.p_begin;
            pack_transposed(t, P, g, D0, D1, ht);
            // SPLIT: the net's region of the chain's SPLIT blob and its W1ᵀ planes
            if (use_split(t->c) && D1 && t->amode == trn::AM_RELU && (ht == 2 || ht == 4)) {
                const ULayer& SU = P.sulayers[li];
                const UNet& s0 = (phase == TR_PHASE_S) ? SU.s : SU.t;
                const int slo = s0.off_w0;
                const int shi = s0.off_out + round16((s0.n_out * 16 * ht + 4) * 4);
                g.split = 1;
                g.su = s0;
                g.su.off_w0 -= slo;
                g.su.off_h -= slo;
                g.su.off_out -= slo;
                g.sfwd_src = P.sstages[s0.stage].src_off + slo;
                g.sfwd_bytes = round16(shi - slo);
                g.st_bytes = (ht / 2) * ht * 3072;
                g.st_src = pack_wt_planes(P, g.h_true, g.h_true, ht, ht / 2, D1->w_off, g.h_true, t->tsblob, t->tsdst,
                                          t->tssrc);
            }
            t->nets.push_back(g);
            t->net_nh.push_back(u0.nh);
            t->ops.push_back({li, (int)t->nets.size() - 1, phase});
            return DF_OK;
        };
        int rc = DF_OK;
        if (L.kind == DF_LAYER_RNVP) rc = add(U.s, L.s_dense0, L.s_ndense, TR_PHASE_S);
        if (rc == DF_OK) rc = add(U.t, L.t_dense0, L.t_ndense, TR_PHASE_T);
        if (rc != DF_OK) return rc;
    }
    t->tblob.resize(t->tblob.size() + 16, 0);
    return DF_OK;
}

// The H0-free sweep (df_train::fmode) applies when the inverse pass runs on the wide SPLIT
// kernel and every conditioner is its shape: Dense(≤ 32, 256, relu), Dense(256, 256, relu),
// Dense(256, ≤ 32), with the fused front and the split dW1.
bool fmode_eligible(const df_train* t) {
    const df_chain* c = t->c;
    const Plan& P = c->plan;
    if (!t->layerwise || !P.wide || c->no_wide || !use_wsplit(c) || c->exact || P.uniform) return false;
    if (t->sweep_req != DF_SWEEP_AUTO && t->sweep_req != DF_SWEEP_H0FREE && t->sweep_req != DF_SWEEP_LAYERWISE)
        return false;
    for (const LNet& N : t->lnets) {
        if (N.pre || N.dn.size() != 3) return false;
        const LDense &D0 = N.dn[0], &D1 = N.dn[1], &D2 = N.dn[2];
        if (D0.act != DF_ACT_RELU || D1.act != DF_ACT_RELU) return false;
        if (D0.in_dim > 32 || D0.out_dim != 256 || D1.in_dim != 256 || D1.out_dim != 256) return false;
        // (the feature rows the split dW0 / H0 recompute read are 32 floats: 16 · bwd.mt <= 32)
        if (D2.fwd.mt > 2 || D0.bwd.mt > 2 || D1.bwd.sfrag < 0) return false;
    }
    return true;
}

int ensure_capacity(df_train* t, int64_t batch) {
    if (batch <= t->cap) return DF_OK;
    t->cap_gen++;  // captured train steps name the old buffers
    const Plan& P = t->c->plan;
    t->bb = BatchBufs{};  // every old buffer goes before the new ones are sized (hipMemGetInfo below)
    BatchBufs& bb = t->bb;
    t->cap = 0;
    const int64_t cap = std::max<int64_t>(batch, 1024);
    const int ew = t->layerwise ? 32 : 4;  // exp(-s) row width
    auto nomem = [] { return set_err(DF_ERR_NOMEM, "hipMalloc failed (training activations)"); };
    if (bb.d_snap.alloc(sizeof(float) * P.n_layers * cap * P.d) != hipSuccess ||
        bb.d_zbar.alloc(sizeof(float) * cap * P.d) != hipSuccess ||
        bb.d_ebuf.alloc(sizeof(float) * cap * ew) != hipSuccess)
        return nomem();
    if (t->layerwise) {
        const size_t row = sizeof(float) * (size_t)cap * t->lwidth;
        for (DevBuf* b : {&bb.d_lyp[0], &bb.d_lyp[1], &bb.d_lbp[0], &bb.d_lbp[1], &bb.d_lx})
            if (b->alloc(row) != hipSuccess) return nomem();
        // keep the inverse pass's hidden activations when the chain runs on the generic
        // kernel and they fit (else the sweep recomputes them)
        t->hsave_on = false;
        if (!P.uniform && t->sweep_req != DF_SWEEP_RECOMPUTE) {
            // fmode: H1 only, plus the 32-float feature rows and the relu-mask buffer; else
            // H0 and H1 of every net.  Whatever does not fit falls back: fmode → kept H0/H1
            // → recompute (the sweep's forms, struct df_train)
            size_t free_b = 0, total_b = 0;
            const bool info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
            auto try_keep = [&](bool fm) {
                const size_t hbytes = row * (size_t)P.n_layers * 2 * (fm ? 1 : t->lmax_h);
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
        for (int k = 0; k <= t->lmax_h; ++k) {
            DevBuf h, dl, dv;
            const bool pre = t->any_pre && k < t->lmax_h;
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
    return DF_OK;
}

// The per-layer arguments every sweep kernel takes: LDenseArgs, TrainArgs and ScoreArgs
// name them alike.
template <typename Args>
void fill_layer_args(Args& a, const df_train* t, int layer, int phase, const float* x, const float* theta, bool flow,
                     int64_t batch) {
    const df_chain* c = t->c;
    const Plan& P = c->plan;
    const DevLayer& L = P.layers[layer];
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
hipError_t norm_adjoint(const df_train* t, int layer, float* zbar, int64_t batch, hipStream_t st) {
    const Plan& P = t->c->plan;
    const DevLayer& L = P.layers[layer];
    const float* xmn = t->c->d_params.as<const float>() + L.norm_off;
    return launch_norm_adjoint(zbar, xmn, xmn + P.d, L.alpha, L.beta, P.d, batch, st);
}

// Dynamic LDS declared for the three kernel families of the layer-wise sweep
// (df_train_create_ex), and the most any accepted shape asks of each:
//   ldense      f32 fragments: two chunk buffers of <= kLChunkBytes (chunk_kq·mt·1024 <= 32 KiB),
//               64 KiB; SPLIT planes: two chunks of mt·3072 B, mt = 16: 96 KiB.  The XBAR forms
//               add the resident W0ᵀ and test the sum against the limit themselves (xbar_apart).
//   couple_bwd  both fragment sets, 2·ht·mto·1024 with ht <= 16: 64 KiB at mto = 2; at mto = 1
//               32 KiB + front_dwo_lds(16) = 51,200 B: 83,968 B.
//   sweep       the larger of the dW staging (kLdwLdsMax, 80 KiB) and its front: 83,968 B.
// So no accepted shape reaches the check in LSweep::launch.
constexpr size_t kLdenseLdsLimit = 160 * 1024;
constexpr size_t kCoupleBwdLdsLimit = 160 * 1024;
constexpr size_t kSweepLdsLimit = 160 * 1024;

// LDS of an ldense launch: the operand's chunk buffers, two when it spans several chunks.
size_t ldense_lds_bytes(const LOp& op, bool split) {
    if (split) return (size_t)(op.nkq / 2 > 1 ? 2 : 1) * op.mt * 3072;
    const int nchunks = (op.nkq + op.chunk_kq - 1) / op.chunk_kq;
    return (size_t)(nchunks > 1 ? 2 : 1) * std::min(op.nkq, op.chunk_kq) * op.mt * 1024;
}

// The couple_bwd front of one net: its arguments, instance and LDS.
struct Front {
    LDenseArgs a;
    int ht, mto;
    size_t lds;
};

// The dW products of one net, by how they launch.
struct DwJobs {
    LdwArgs h0{};                // fmode: the split dW1 that recomputes H0 and writes its relu
    bool has_h0 = false;         //   mask, launched before the W1ᵀδ1 product that reads the mask
    std::vector<LdwArgs> split;  // the other split 256×256 products: each its own launch, first
    std::vector<LdwArgs> rest;   // merged into one launch with the next net's front, or one each
};

// What the steps of one layer-wise sweep share (lsweep).
struct LSweep {
    df_train* t;
    df_chain* c;
    const float* x;
    const float* theta;
    int64_t batch;
    float inv_n;
    bool flow;
    hipStream_t st;
    unsigned dgrid;           // workgroups of the Dense kernels
    const uint8_t* lb;        // the layer-wise blob: fragments
    const float* lbf;         //   ... and padded biases
    const uint8_t* lsb;       // its SPLIT planes
    bool lsplit;              // the chain's arithmetic, fixed at df_chain_create
    bool fm;                  // H0-free sweep (struct df_train)
    int par = 0;              // buffer parity of the current net
    bool front_done = false;  // this net's couple_bwd ran in the previous merged launch
    int rc = DF_OK;           // the first error: nothing launches after it

    void fail(int code, const char* msg) {
        if (rc == DF_OK) rc = set_err(code, msg);
    }
    // Every launch of the sweep goes through one of these two.
    template <typename Launch>
    void launch(const char* where, Launch&& go) {
        if (rc != DF_OK) return;
        const hipError_t e = go();
        if (e != hipSuccess) rc = hip_err(e, where);
    }
    // ... with dynamic LDS: the request is held against what the kernel family declares
    template <typename Launch>
    void launch(const char* where, const char* family, size_t lds, size_t limit, Launch&& go) {
        if (lds > limit)
            fail(DF_ERR_UNSUPPORTED, (std::string("layer-wise training: a ") + family +
                                      " launch needs more LDS than its kernels declare").c_str());
        launch(where, go);
    }
    void ldense(int mt, int in_kind, int epi, const LDenseArgs& a, size_t lds) {
        launch("layer-wise dense launch", "ldense", lds, kLdenseLdsLimit,
               [&] { return launch_ldense(mt, in_kind, epi, a, dgrid, lds, st); });
    }
    void gather(const LDenseArgs& a, int rows) {
        launch("layer-wise dense launch", [&] { return launch_gather_features(a, rows, st); });
    }
    void ldw(const LdwArgs& w, const char* where) {
        launch(where, [&] { return launch_ldw(w, (unsigned)t->lgrid, st); });
    }

    bool keeps(const SweepOp& op) const { return t->hsave_on && !t->lnets[op.net].pre; }
    static int net_slot(const SweepOp& op) { return 2 * op.layer + (op.phase == TR_PHASE_T ? 1 : 0); }
    // fmode: the net's feature rows [B][32] (written by the inverse pass)
    float* fbuf(const SweepOp& op) const { return t->bb.d_fsave.as<float>() + (int64_t)net_slot(op) * batch * 32; }
    // whether the net's backward front is the fused couple_bwd kernel (kept activations,
    // <= 32 outputs, hidden <= 256)
    bool fused_front(const SweepOp& op) const {
        const LNet& N = t->lnets[op.net];
        const int nd = (int)N.dn.size();
        return nd >= 2 && keeps(op) && N.dn[nd - 1].fwd.mt <= 2 && N.dn[0].bwd.mt <= 4;
    }
    // H_k of a net: kept by the inverse pass, or recomputed into the shared buffers
    float* Hbuf(const SweepOp& op, int k) const {
        float* hsave = t->bb.d_hsave.as<float>();
        const int64_t W = t->lwidth;
        if (fm) return k == 1 ? hsave + (int64_t)net_slot(op) * batch * W : nullptr;  // H1 only
        return keeps(op) ? hsave + ((int64_t)net_slot(op) * t->lmax_h + k) * batch * W : t->bb.d_lh[k].as<float>();
    }
    // ȳ and the δ of the last hidden Dense alternate between two buffers from net to
    // net: a merged launch writes net i+1's while net i's dW products read net i's
    float* ybuf(int p) const { return t->bb.d_lyp[p].as<float>(); }
    float* dbuf(const SweepOp& op, int k, int p) const {
        return k == (int)t->lnets[op.net].dn.size() - 2 ? t->bb.d_lbp[p].as<float>() : t->bb.d_ld[k].as<float>();
    }
    const uint8_t* sfrag_of(const LOp& op, int in_kind, int epi) const {
        return (lsplit && op.sfrag >= 0 && ldense_split_supported(op.mt, in_kind, epi)) ? lsb + op.sfrag : nullptr;
    }
    // σ' argument of Dense k's output: H_k, or the stored σ'(x_k)
    void dact(const SweepOp& op, int k, LDenseArgs& a) const {
        const LNet& N = t->lnets[op.net];
        a.hprev = N.pre ? t->bb.d_lv[k].as<float>() : Hbuf(op, k);
        a.dact = N.pre ? trn::kDactStored : N.dn[k].act;
    }
    LDenseArgs base_args(const SweepOp& op) const {
        LDenseArgs b{};
        fill_layer_args(b, t, op.layer, op.phase, x, theta, flow, batch);
        b.n_in = t->lnets[op.net].dn[0].in_dim;
        b.zbar = t->bb.d_zbar.as<float>();
        b.ebuf = t->bb.d_ebuf.as<float>();
        b.inv_n = inv_n;
        b.ld_in = b.ld_out = b.ld_h = b.ld_x = t->lwidth;
        return b;
    }
    // one Dense product on operand op
    void dense(const LOp& op, int in_kind, int epi, LDenseArgs a) {
        a.wfrag = lb + op.frag;
        a.bias = (op.bias >= 0 && (epi == LEPI_ACT || epi == LEPI_COUPLE)) ? lbf + op.bias : nullptr;
        a.nkq = op.nkq;
        a.chunk_kq = op.chunk_kq;
        a.sfrag = sfrag_of(op, in_kind, epi);
        ldense(op.mt, in_kind, epi, a, ldense_lds_bytes(op, a.sfrag != nullptr));
    }
    // couple_bwd: output Dense + pullback → ȳ, then δ_last = (W_outᵀ ȳ) ⊙ σ'(H)
    Front front(const SweepOp& op, int p) const {
        const LNet& N = t->lnets[op.net];
        const int nd = (int)N.dn.size();
        const LDense& DO = N.dn[nd - 1];
        Front f{base_args(op), DO.bwd.mt, DO.fwd.mt, (size_t)2 * DO.bwd.mt * DO.fwd.mt * 1024};
        LDenseArgs& a = f.a;
        a.act = DO.act;
        a.in = Hbuf(op, nd - 2);
        a.wfrag = lb + DO.fwd.frag;
        a.bias = DO.fwd.bias >= 0 ? lbf + DO.fwd.bias : nullptr;
        a.nkq = DO.fwd.nkq;
        a.w2frag = lb + DO.bwd.frag;
        a.nkq2 = DO.bwd.nkq;
        a.out = ybuf(p);
        a.out2 = dbuf(op, nd - 2, p);
        a.dact = N.dn[nd - 2].act;
        if (front_dwo(DO.fwd.mt)) {  // the output Dense's dW / db come from the front (partial rows: lgrid)
            a.dwo_partial = t->d_partial.as<float>();
            a.dwo_p_total = t->P;
            a.dwo_w_off = DO.w_off;
            a.dwo_b_off = DO.b_off;
            a.dwo_m_true = DO.out_dim;
            a.dwo_n_true = DO.in_dim;
            f.lds += front_dwo_lds(DO.bwd.mt);
        }
        return f;
    }
};

// forward (recompute): H_k = σ(W_k · in + b_k), then the output Dense + coupling pullback → ȳ
void recompute_forward(LSweep& s, const SweepOp& op, const LDenseArgs& b, bool fused) {
    df_train* t = s.t;
    const LNet& N = t->lnets[op.net];
    const int nd = (int)N.dn.size();
    const bool keep = s.keeps(op);
    float* lx = t->bb.d_lx.as<float>();
    for (int k = 0; k < nd - (fused ? 1 : 0); ++k) {
        LDenseArgs a = b;
        a.act = N.dn[k].act;
        if (k + 1 < nd && keep) {
            if (k == 0 && !s.fm) {  // (fmode: the inverse pass kept the features)
                a.xsave = lx;
                s.gather(a, 16 * N.dn[0].bwd.mt);
            }
            continue;
        }
        if (k == 0) {
            a.xsave = lx;
            if (nd == 1) {  // a single-Dense conditioner: its input is the gathered features
                s.gather(a, 16 * N.dn[0].bwd.mt);
                a.in = lx;
            }
        } else {
            a.in = s.Hbuf(op, k - 1);
        }
        if (k + 1 < nd) {
            a.out = s.Hbuf(op, k);
            a.dsave = N.pre ? t->bb.d_lv[k].as<float>() : nullptr;
            s.dense(N.dn[k].fwd, k == 0 ? LIN_GATHER : LIN_BUF, LEPI_ACT, a);
        } else {
            a.out = s.ybuf(s.par);
            s.dense(N.dn[k].fwd, LIN_BUF, LEPI_COUPLE, a);
        }
    }
}

// dW = δ · inᵀ, db = Σ δ of every Dense of a net (per-workgroup partials), classified by
// how they launch (DwJobs)
void dw_jobs(LSweep& s, const SweepOp& op, bool fused, DwJobs& out) {
    df_train* t = s.t;
    const Plan& P = s.c->plan;
    const LNet& N = t->lnets[op.net];
    const int nd = (int)N.dn.size();
    const int W = t->lwidth;
    for (int k = 0; k < nd; ++k) {
        const LDense& D = N.dn[k];
        if (k + 1 == nd && fused && front_dwo(D.fwd.mt)) continue;  // (the front's)
        LdwArgs w{};
        w.da = (k + 1 == nd) ? s.ybuf(s.par) : s.dbuf(op, k, s.par);
        w.lda = W;
        w.m_true = D.out_dim;
        w.mta = D.fwd.mt;
        w.xb = (k == 0) ? (s.fm ? s.fbuf(op) : t->bb.d_lx.as<float>()) : s.Hbuf(op, k - 1);
        w.ldb = (k == 0 && s.fm) ? 32 : W;
        w.n_true = D.in_dim;
        w.ntb = D.bwd.mt;
        w.partial = t->d_partial.as<float>();
        w.p_total = t->P;
        w.w_off = D.w_off;
        w.b_off = D.b_off;
        w.batch = s.batch;
        if (!ldw_shape(w.mta, w.ntb, &w.wm, &w.bm, &w.bn)) {
            s.fail(DF_ERR_UNSUPPORTED, "dW tiling");
            return;
        }
        // hidden-256 × hidden-256 dW on bf16x3 split products (ldw_split_body)
        w.split = (s.lsplit && w.mta == 16 && w.ntb == 16 && w.bm == kLdwBM && w.bn == kLdwBN) ? 1 : 0;
        if (s.fm && k == 1) {  // dW1 with H0 recomputed from the features (and its relu mask)
            if (!w.split || nd != 3) {
                s.fail(DF_ERR_INVALID, "internal: H0-free sweep without the split dW1");
                return;
            }
            const WLayer& WL = P.wslayers[op.layer];
            const WNet& WN = op.phase == TR_PHASE_T ? WL.t : WL.s;
            const DevStage& S0 = P.wsstages[WN.stage0];
            w.xb = nullptr;
            w.feat = s.fbuf(op);
            w.w0s = s.c->d_wsblob.as<const uint8_t>() + S0.src_off;
            w.b0 = s.c->d_wbias.as<const float>() + WN.b0;
            w.hmask = t->bb.d_hmask.as<uint32_t>();
            out.h0 = w;
            out.has_h0 = true;
        } else if (w.split) {
            out.split.push_back(w);
        } else {
            out.rest.push_back(w);
        }
    }
}

// δ0 = (W1ᵀ δ1) ⊙ σ'(H0) with x̄ = W0ᵀ δ0 in its epilogue.  Returns false when W0ᵀ does not
// fit beside the W1ᵀ chunk buffers: δ0 alone ran, and x̄ is left to its own product.
bool w1t_delta_xbar(LSweep& s, const LNet& N, LDenseArgs& a) {
    const LOp &lo = N.dn[1].bwd, &w0 = N.dn[0].bwd;
    a.w0t = s.lb + w0.frag;
    a.w0t_mt = w0.mt;
    a.w0t_nkq = w0.nkq;
    const int xepi = s.fm ? LEPI_DACT_XBAR_MASK : LEPI_DACT_XBAR;
    a.sfrag = s.sfrag_of(lo, LIN_BUF, xepi);
    if (s.fm && !a.sfrag) {
        s.fail(DF_ERR_INVALID, "internal: H0-free sweep without the split W1ᵀδ1");
        return true;
    }
    // x̄ on split products when the W1ᵀδ1 product is SPLIT and W0ᵀ has planes
    a.w0s = (a.sfrag && w0.sfrag >= 0 && a.w0t_nkq <= 16) ? s.lsb + w0.sfrag : nullptr;
    const size_t wbytes = ldense_lds_bytes(lo, a.sfrag != nullptr);
    auto w0_bytes = [&]() {
        return a.w0s ? (size_t)(a.w0t_nkq / 2) * a.w0t_mt * 3072 : (size_t)a.w0t_mt * a.w0t_nkq * 1024;
    };
    // W0ᵀ stays resident beside the W1ᵀ chunk buffers: with more than 32
    // conditioner inputs its split planes (or even its f32 fragments, at 64
    // inputs) do not fit; then the f32 fragments, or x̄ = W0ᵀδ0 as its own
    // product after the δ0 kernel
    if (wbytes + w0_bytes() + 64 > kLdenseLdsLimit) a.w0s = nullptr;
    const size_t lds = wbytes + w0_bytes() + 64;  // + z̄ column table
    a.wfrag = s.lb + lo.frag;
    a.nkq = lo.nkq;
    a.chunk_kq = lo.chunk_kq;
    if (lds <= kLdenseLdsLimit) {
        s.ldense(lo.mt, LIN_BUF, xepi, a, lds);
        return true;
    }
    if (s.fm) {
        s.fail(DF_ERR_INVALID, "internal: H0-free sweep with a wide first Dense");
        return true;
    }
    a.w0t = nullptr;
    s.dense(lo, LIN_BUF, LEPI_DACT, a);
    return false;
}

// backward: δ_{k-1} = (W_kᵀ δ_k) ⊙ σ'(H_{k-1}) down to δ_0, then x̄ = W0ᵀ δ_0 → z̄ (identity
// dims).  Behind the fused front, couple_bwd gives ȳ and the δ of the last hidden Dense in one
// pass over H (unless the previous merged launch ran it), and the W1ᵀ product carries x̄ in
// its epilogue.
void backward(LSweep& s, const SweepOp& op, const LDenseArgs& b, bool fused, const DwJobs& jobs) {
    df_train* t = s.t;
    const LNet& N = t->lnets[op.net];
    const int nd = (int)N.dn.size();
    if (fused && !s.front_done) {
        const Front f = s.front(op, s.par);
        // (a front that writes dW partial rows runs on every row's workgroup)
        const unsigned fgrid = front_dwo(f.mto) ? (unsigned)t->lgrid : s.dgrid;
        s.launch("layer-wise dense launch", "couple_bwd", f.lds, kCoupleBwdLdsLimit,
                 [&] { return launch_couple_bwd(f.ht, f.mto, f.a, fgrid, f.lds, s.st); });
    }
    if (jobs.has_h0) s.ldw(jobs.h0, "layer-wise dense launch");
    const float* gcur = fused ? s.dbuf(op, nd - 2, s.par) : s.ybuf(s.par);
    bool xbar_done = false;  // x̄ came out of the W1ᵀ δ1 launch
    for (int k = nd - (fused ? 2 : 1); k >= 1; --k) {
        LDenseArgs a = b;
        a.in = gcur;
        s.dact(op, k - 1, a);
        if (s.fm && k == 1) {  // σ'(H0) from the mask the split dW1 just wrote
            a.hprev = nullptr;
            a.hmask = t->bb.d_hmask.as<uint32_t>();
        }
        a.out = s.dbuf(op, k - 1, s.par);
        if (fused && k == 1)
            xbar_done = w1t_delta_xbar(s, N, a);
        else
            s.dense(N.dn[k].bwd, LIN_BUF, LEPI_DACT, a);
        gcur = a.out;
    }
    if (!xbar_done) {
        LDenseArgs a = b;
        a.in = gcur;
        s.dense(N.dn[0].bwd, LIN_BUF, LEPI_XBAR, a);
    }
}

// The dW products of net op oi after its backward: the split 256×256 ones as their own
// launches (one wave per SIMD, ldw_split_kernel), the rest merged with the next net's front
// when that net is the next op and runs the fused front (its front reads only z̄ after this
// net's W1ᵀδ1 kernel, the kept H, and writes the other parity's ȳ / δ_last)
void weight_grads(LSweep& s, size_t oi, DwJobs& jobs) {
    df_train* t = s.t;
    s.front_done = false;
    for (const LdwArgs& w : jobs.split) s.ldw(w, "split dW kernel launch");
    std::vector<LdwArgs>& rest = jobs.rest;
    if (t->separate || rest.size() > 3) {  // DF_SWEEP_SEPARATE
        for (const LdwArgs& w : rest) s.ldw(w, "dW kernel launch");
        return;
    }
    SweepJob j{};
    // narrow (HBM-bound) products first, the hidden×hidden one last: even
    // workgroups run them in this order, odd ones in reverse
    std::stable_sort(rest.begin(), rest.end(), [](const LdwArgs& p, const LdwArgs& q) {
        return ldw_staging_samples(p) > ldw_staging_samples(q);
    });
    j.nw = (int)rest.size();
    for (int k = 0; k < j.nw; ++k) {
        j.w[k] = rest[k];
        j.ws[k] = ldw_staging_samples(rest[k]);
    }
    int ht = 0, mto = 1;
    size_t lds = ldw_lds_bytes();
    if (oi + 1 < t->ops.size() && t->ops[oi + 1].net >= 0 && s.fused_front(t->ops[oi + 1])) {
        const Front f = s.front(t->ops[oi + 1], s.par ^ 1);
        if (sweep_supported(f.ht, f.mto)) {
            j.front = f.a;
            j.has_front = 1;
            ht = f.ht;
            mto = f.mto;
            lds = std::max(lds, f.lds);
        }
    }
    s.launch("merged sweep launch", "sweep", lds, kSweepLdsLimit,
             [&] { return launch_sweep(ht, mto, j, (unsigned)t->lgrid, lds, s.st); });
    s.front_done = j.has_front != 0;
}

// Reverse sweep of the layer-wise path (chain order; see df_ltrain.h).
int lsweep(df_train* t, const float* x, const float* theta, int64_t batch, float inv_n, bool flow, hipStream_t st) {
    df_chain* c = t->c;
    const int64_t ntiles = (batch + 15) / 16;
    const unsigned dgrid =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(c->grid_cus, (ntiles + kWavesPerBlock * kLTiles - 1) /
                                                                              (kWavesPerBlock * kLTiles)));
    LSweep s{};
    s.t = t;
    s.c = c;
    s.x = x;
    s.theta = theta;
    s.batch = batch;
    s.inv_n = inv_n;
    s.flow = flow;
    s.st = st;
    s.dgrid = dgrid;
    s.lb = t->d_lblob.as<const uint8_t>();
    s.lbf = t->d_lblob.as<const float>();
    s.lsb = t->d_lsblob.as<const uint8_t>();
    s.lsplit = !c->exact;
    s.fm = h0free(t);
    for (size_t oi = 0; oi < t->ops.size() && s.rc == DF_OK; ++oi) {
        const SweepOp& op = t->ops[oi];
        if (op.net < 0) {
            s.launch("norm adjoint launch",
                     [&] { return norm_adjoint(t, op.layer, t->bb.d_zbar.as<float>(), batch, st); });
            s.front_done = false;
            continue;
        }
        const bool fused = s.fused_front(op);
        if (s.fm && !fused) {
            s.fail(DF_ERR_INVALID, "internal: H0-free sweep without the fused front");
            break;
        }
        const LDenseArgs b = s.base_args(op);
        recompute_forward(s, op, b, fused);
        // (built before the backward: fmode's split dW1 runs inside it)
        DwJobs jobs;
        dw_jobs(s, op, fused, jobs);
        backward(s, op, b, fused, jobs);
        weight_grads(s, oi, jobs);
        s.par ^= 1;
    }
    return s.rc;
}

// The rules of df_train_create_opt, validated (include/densityflows_hip.h: limits and values)
// into the kernels' OptChain.  clip: index of the ClipNorm; eta_rule: the rule
// df_train_adjust writes; adam: the chain's Adam (its β seed and advance βᵗ).
int check_rules(const df_opt_rule* rules, int n_rules, OptChain& och, int& clip, int& eta_rule, df_adam& adam) {
    if (!rules && n_rules > 0) return set_err(DF_ERR_INVALID, "null pointer");
    if (n_rules < 1) return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: no rule (a chain needs an Adam or a Descent)");
    if (n_rules > kOptMaxRules) return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: more than 8 rules");
    int i_adam = -1, i_descent = -1;
    clip = -1;
    och = OptChain{};
    och.n = n_rules;
    for (int r = 0; r < n_rules; ++r) {
        const float* p = rules[r].p;
        och.kind[r] = rules[r].kind;
        switch (rules[r].kind) {
            case DF_OPT_ADAM:
                if (i_adam >= 0) return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: more than one Adam");
                if (!(p[0] >= 0.f) || !(p[1] >= 0.f && p[1] < 1.f) || !(p[2] >= 0.f && p[2] < 1.f) || !(p[3] >= 0.f))
                    return set_err(DF_ERR_INVALID, "invalid Adam hyper-parameters");
                i_adam = r;
                adam = df_adam{p[0], p[1], p[2], p[3]};
                for (int k = 0; k < 4; ++k) och.p[r][k] = p[k];
                break;
            case DF_OPT_DESCENT:
                if (!(p[0] >= 0.f)) return set_err(DF_ERR_INVALID, "invalid Descent learning rate (η >= 0)");
                if (i_descent < 0) i_descent = r;
                och.p[r][0] = p[0];
                break;
            case DF_OPT_CLIP_GRAD:
                if (!(p[0] > 0.f)) return set_err(DF_ERR_INVALID, "invalid ClipGrad bound (δ > 0)");
                och.p[r][0] = p[0];
                break;
            case DF_OPT_CLIP_NORM:
                if (clip >= 0) return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: more than one ClipNorm");
                if (i_adam >= 0)
                    return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: ClipNorm after Adam (it stands before it)");
                if (!(p[0] > 0.f)) return set_err(DF_ERR_INVALID, "invalid ClipNorm bound (ω > 0)");
                clip = r;
                och.p[r][0] = p[0];
                break;
            case DF_OPT_WEIGHT_DECAY:
                if (!(p[0] >= 0.f)) return set_err(DF_ERR_INVALID, "invalid WeightDecay factor (λ >= 0)");
                och.p[r][0] = p[0];
                break;
            default:
                return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: unknown rule (df_opt_kind)");
        }
    }
    if (i_adam < 0 && i_descent < 0)
        return set_err(DF_ERR_UNSUPPORTED, "OptimiserChain: no terminal rule (a chain needs an Adam or a Descent)");
    eta_rule = i_adam >= 0 ? i_adam : i_descent;
    return DF_OK;
}

// Every Dense weight and bias as a slice of the flat trainables, in increasing order.
// False unless they tile [0, P) exactly.
bool tensor_table(const Plan& P, std::vector<int32_t>& toff) {
    std::vector<std::pair<int32_t, int32_t>> sl;  // (offset, count)
    for (const DevDense& D : P.denses) {
        sl.push_back({D.w_off, D.in_dim * D.n_out});
        if (D.b_off >= 0) sl.push_back({D.b_off, D.n_out});
    }
    std::sort(sl.begin(), sl.end());
    toff.assign(1, 0);
    for (const auto& s : sl) {
        if (s.first != toff.back() || s.second <= 0) return false;
        toff.push_back(s.first + s.second);
    }
    return (int64_t)toff.back() == (int64_t)P.trainables.size();
}

int ensure_toff(df_train* t) { return t->d_toff.get() ? DF_OK : upload(t->toff, t->d_toff); }

// Device state of an optimiser chain: the tensor offsets, Σ dx² per tensor and the update
// kernel's workgroup → tensor table (built once: no workgroup spans two tensors).
int setup_chain(df_train* t) {
    std::vector<OptBlock> blocks;
    const int nt = (int)t->toff.size() - 1;
    for (int k = 0; k < nt; ++k)
        for (int32_t b = t->toff[k]; b < t->toff[k + 1]; b += kOptThreads)
            blocks.push_back({b, std::min<int32_t>(kOptThreads, t->toff[k + 1] - b), k});
    t->n_oblocks = (int64_t)blocks.size();
    int rc = ensure_toff(t);
    if (rc == DF_OK) rc = upload(blocks, t->d_oblocks);
    if (rc != DF_OK) return rc;
    const size_t sb = sizeof(float) * (size_t)std::max(nt, 4);
    if (t->d_sumsq.alloc(sb) != hipSuccess) return set_err(DF_ERR_NOMEM, "hipMalloc failed (optimiser chain)");
    if (hipMemset(t->d_sumsq.get(), 0, sb) != hipSuccess) return set_err(DF_ERR_HIP, "hipMemset(optimiser chain)");
    return DF_OK;
}

}  // namespace

extern "C" {

int df_train_destroy(df_train* t) {
    if (!t) return DF_OK;
    DeviceGuard gd(t->c->device);
    free_all(t);
    t->c->n_trainers--;
    delete t;
    return DF_OK;
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
    OptChain och{};
    int clip = -1, eta_rule = -1;
    df_adam adam{1e-3f, 0.9f, 0.999f, 1e-8f};
    int rc0 = check_rules(rules, n_rules, och, clip, eta_rule, adam);
    if (rc0 != DF_OK) return rc0;
    const int form = sweep & ~DF_SWEEP_SEPARATE;
    if (form < DF_SWEEP_AUTO || form > DF_SWEEP_LAYERWISE || (sweep & ~(DF_SWEEP_SEPARATE | 7)))
        return set_err(DF_ERR_INVALID, "unknown sweep form");
    if (form == DF_SWEEP_FUSED && (sweep & DF_SWEEP_SEPARATE))
        return set_err(DF_ERR_INVALID, "DF_SWEEP_SEPARATE applies to the layer-wise forms");
    df_train* t = new (std::nothrow) df_train();
    if (!t) return set_err(DF_ERR_NOMEM, "host allocation failed");
    t->c = c;
    t->sweep_req = form;
    t->separate = (sweep & DF_SWEEP_SEPARATE) != 0;
    if (const char* v = std::getenv("DF_SCORE_PER_NET")) t->score_per_net = v[0] == '1';
    t->opt = adam;
    t->och = och;
    t->och_clip = clip;
    t->och_eta = eta_rule;
    t->chain_mode = !(och.n == 1 && och.kind[0] == DF_OPT_ADAM);
    const Plan& P = c->plan;
    t->P = (int64_t)P.trainables.size();
    if (!tensor_table(P, t->toff)) {
        delete t;
        return set_err(DF_ERR_INVALID, "internal: the Dense tensors do not tile the flat trainables");
    }
    t->amode = P.relu_only ? trn::AM_RELU : trn::AM_Y;
    for (const DevDense& D : P.denses)
        if (act_needs_pre(D.act) && !P.relu_only) t->amode = trn::AM_PRE;
    // fused per-net kernel when every conditioner fits its registers, else layer-wise
    int rc = (form == DF_SWEEP_AUTO || form == DF_SWEEP_FUSED) ? build_nets(t) : DF_ERR_UNSUPPORTED;
    if (rc == DF_ERR_UNSUPPORTED && form != DF_SWEEP_FUSED) {
        t->nets.clear();
        t->net_nh.clear();
        t->ops.clear();
        t->tblob.clear();
        t->tdst.clear();
        t->tsrc.clear();
        t->tsblob.clear();
        t->tsdst.clear();
        t->tssrc.clear();
        t->layerwise = true;
        rc = build_lnets(t);
    }
    if (rc != DF_OK) {
        delete t;
        return rc;
    }
    DeviceGuard gd(c->device);
    if (!gd.ok) {
        delete t;
        return set_err(DF_ERR_HIP, "hipSetDevice failed");
    }
    c->n_trainers++;
    // LDS and resident grid of the net kernels
    for (size_t i = 0; i < t->nets.size(); ++i) t->lds_max = std::max(t->lds_max, train_net_lds(P.ht, t->nets[i]));
    if (t->lds_max > 160 * 1024) {
        df_train_destroy(t);
        return set_err(DF_ERR_UNSUPPORTED, "training kernel needs more than 160 KiB of LDS");
    }
    hipError_t e = set_train_lds_limit(t->lds_max);
    if (e != hipSuccess) {
        df_train_destroy(t);
        return hip_err(e, "hipFuncSetAttribute(train)");
    }
    int occ = 1;
    for (size_t i = 0; i < t->nets.size(); ++i) {
        int b = 1;
        if (train_net_occupancy(P.ht, t->net_nh[i], t->amode, t->lds_max, &b, t->nets[i].split != 0) == hipSuccess &&
            b >= 1)
            occ = (i == 0) ? b : std::min(occ, b);
    }
    t->grid = std::max(1, c->grid_cus * occ);
    if (t->layerwise) {
        // (the limits LSweep::launch holds every request against; derivation at the constants)
        e = set_ldense_lds_limit(kLdenseLdsLimit);
        if (e == hipSuccess) e = set_couple_bwd_lds_limit(kCoupleBwdLdsLimit);
        if (e == hipSuccess) e = set_sweep_lds_limit(kSweepLdsLimit);
        if (e != hipSuccess) {
            df_train_destroy(t);
            return hip_err(e, "hipFuncSetAttribute(layer-wise training)");
        }
        t->lgrid = std::max(1, c->grid_cus);
        t->grid = t->lgrid;  // partial rows
        t->fmode = fmode_eligible(t);
        // an explicit form the chain cannot take: the H0-free sweep's shape, or kept
        // activations of a chain whose inverse pass (the specialised kernel) keeps none
        if ((form == DF_SWEEP_H0FREE && !t->fmode) || (form == DF_SWEEP_KEPT && P.uniform)) {
            df_train_destroy(t);
            return set_err(DF_ERR_UNSUPPORTED, form == DF_SWEEP_H0FREE
                                                   ? "DF_SWEEP_H0FREE needs wide SPLIT nets Dense(<=32,256,relu), "
                                                     "Dense(256,256,relu), Dense(256,<=32)"
                                                   : "DF_SWEEP_KEPT needs a chain on the generic or wide kernel");
        }
    }
    if (c->debug_launch)  // tuning aid (DF_DEBUG_LAUNCH=1): the resident grids on stderr
        std::fprintf(stderr, "[df] train: %s sweep, %d CUs (of %d), grid %d at %d workgroups per CU, lgrid %d\n",
                     t->layerwise ? "layer-wise" : "fused", c->grid_cus, c->n_cu, t->grid, occ, t->lgrid);
    const size_t pb = sizeof(float) * (size_t)std::max<int64_t>(t->P, 4);
    if (t->d_params.alloc(pb) != hipSuccess || t->d_m.alloc(pb) != hipSuccess || t->d_v.alloc(pb) != hipSuccess ||
        t->d_grad.alloc(pb) != hipSuccess || t->d_partial.alloc(pb * t->grid) != hipSuccess ||
        t->d_lpsum.alloc(sizeof(double)) != hipSuccess || t->d_bt.alloc(2 * sizeof(float)) != hipSuccess) {
        df_train_destroy(t);
        return set_err(DF_ERR_NOMEM, "hipMalloc failed (training state)");
    }
    {  // Optimisers.setup: βᵗ = β for the first update
        const float bt[2] = {t->opt.beta1, t->opt.beta2};
        if (hipMemcpy(t->d_bt.get(), bt, sizeof(bt), hipMemcpyHostToDevice) != hipSuccess) {
            df_train_destroy(t);
            return set_err(DF_ERR_HIP, "hipMemcpy(Adam state)");
        }
    }
    // The trainer's blobs and every blob's repack map, the table in the order repack() launches.
    // A map that is switched off keeps its entry and its (16-byte) index arrays with n = 0,
    // which launches nothing, and the device allocations below keep the sequence they have
    // always had: where these buffers land on the device moves a small-batch step by 0.1 %
    // (profiles/train_host_refactor_ab.txt), so neither drop one nor reorder them.
    enum { MP, MT, MW, MWB, MS, MWS, ML, MTS, MLS, kMaps };
    struct MapSrc {
        const std::vector<int32_t>*dst, *src;
        bool on, split;
    };
    const MapSrc ms[kMaps] = {{&P.pack_dst, &P.pack_src, true, false},
                              {&t->tdst, &t->tsrc, !t->tdst.empty(), false},
                              {&P.wpack_dst, &P.wpack_src, P.wide != 0, false},
                              {&P.wbias_dst, &P.wbias_src, P.wide != 0, false},
                              {&P.spack_dst, &P.spack_src, P.split != 0, true},
                              {&P.wspack_dst, &P.wspack_src, P.wsplit != 0, true},
                              {&t->ldst, &t->lsrc, !t->ldst.empty(), false},
                              {&t->tsdst, &t->tssrc, !t->tsdst.empty(), true},
                              {&t->lsdst, &t->lssrc, !t->lsdst.empty(), true}};
    t->maps.resize(kMaps);
    auto dst = [&](int i) { return upload(*ms[i].dst, t->maps[i].dst); };
    auto src = [&](int i) { return upload(*ms[i].src, t->maps[i].src); };
    auto both = [&](int i) {
        const int rc2 = dst(i);
        return rc2 != DF_OK ? rc2 : src(i);
    };
    if ((rc = upload(t->tblob, t->d_tblob)) != DF_OK || (rc = upload(t->lblob, t->d_lblob)) != DF_OK ||
        (rc = both(ML)) != DF_OK || (rc = dst(MP)) != DF_OK || (rc = both(MW)) != DF_OK ||
        (rc = both(MWB)) != DF_OK || (rc = src(MP)) != DF_OK || (rc = both(MT)) != DF_OK ||
        (rc = both(MS)) != DF_OK || (rc = both(MWS)) != DF_OK ||
        (rc = upload(t->lsblob, t->d_lsblob)) != DF_OK || (rc = both(MLS)) != DF_OK ||
        (rc = upload(t->tsblob, t->d_tsblob)) != DF_OK || (rc = both(MTS)) != DF_OK) {
        std::string m = last_error();
        df_train_destroy(t);
        return set_err(rc, m);
    }
    void* const blobs[kMaps] = {c->d_blob.get(),  t->d_tblob.get(), c->d_wblob.get(),  c->d_wbias.get(), c->d_sblob.get(),
                                c->d_wsblob.get(), t->d_lblob.get(), t->d_tsblob.get(), t->d_lsblob.get()};
    for (int i = 0; i < kMaps; ++i) {
        RepackMap& m = t->maps[i];
        m.blob = blobs[i];
        m.n = ms[i].on ? (int64_t)ms[i].dst->size() : 0;
        m.split = ms[i].split;
    }
    if (t->P > 0 && (hipMemcpy(t->d_params.get(), P.trainables.data(), sizeof(float) * t->P, hipMemcpyHostToDevice) !=
                         hipSuccess ||
                     hipMemset(t->d_m.get(), 0, sizeof(float) * t->P) != hipSuccess ||
                     hipMemset(t->d_v.get(), 0, sizeof(float) * t->P) != hipSuccess ||
                     hipMemset(t->d_grad.get(), 0, sizeof(float) * t->P) != hipSuccess)) {
        df_train_destroy(t);
        return set_err(DF_ERR_HIP, "initialising the training state failed");
    }
    // (after every allocation a plain-Adam trainer makes: theirs keep their places)
    if (t->chain_mode && (rc = setup_chain(t)) != DF_OK) {
        std::string m = last_error();
        df_train_destroy(t);
        return set_err(rc, m);
    }
    *out = t;
    return DF_OK;
}

int df_train_num_params(const df_train* t, int64_t* count) {
    if (!t || !count) return set_err(DF_ERR_INVALID, "null pointer");
    *count = t->P;
    return DF_OK;
}

int df_train_sweep(const df_train* t, int* form) {
    if (!t || !form) return set_err(DF_ERR_INVALID, "null pointer");
    if (!t->layerwise) *form = DF_SWEEP_FUSED;
    else if (t->cap == 0)  // no gradient yet: the form ensure_capacity will try first
        *form = t->fmode ? DF_SWEEP_H0FREE
                         : (t->c->plan.uniform || t->sweep_req == DF_SWEEP_RECOMPUTE) ? DF_SWEEP_RECOMPUTE : DF_SWEEP_KEPT;
    else if (h0free(t)) *form = DF_SWEEP_H0FREE;
    else *form = t->hsave_on ? DF_SWEEP_KEPT : DF_SWEEP_RECOMPUTE;
    if (t->layerwise && t->separate) *form |= DF_SWEEP_SEPARATE;
    return DF_OK;
}

int df_train_grad_ptr(df_train* t, float** grad_dev) {
    if (!t || !grad_dev) return set_err(DF_ERR_INVALID, "null pointer");
    *grad_dev = t->d_grad.as<float>();
    return DF_OK;
}

}  // extern "C"

namespace {
// Whether the kernels normalise θ for this trainer (df_theta_input); DF_THETA_RAW
// without bounds on a conditional chain is an error (-1).
int theta_flow(const df_train* t) {
    const df_chain* c = t->c;
    if (c->plan.n == 0) return 0;
    switch (t->theta_input) {
    case DF_THETA_GIVEN: return 0;
    case DF_THETA_RAW: return c->has_bounds ? 1 : -1;
    default: return c->has_bounds ? 1 : 0;
    }
}
}  // namespace

extern "C" {

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
    df_chain* c = t->c;
    const Plan& P = c->plan;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* lp = logpdf_sum ? logpdf_sum : t->d_lpsum.as<double>();  // where this gradient writes Σ logpdf
    t->last_lp = lp;
    t->last_n = n_total;
    if (batch == 0) {
        hipError_t e = hipMemsetAsync(t->d_grad.get(), 0, sizeof(float) * t->P, st);
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
    if (rc != DF_OK) return rc;
    const BatchBufs& bb = t->bb;
    float *snap = bb.d_snap.as<float>(), *zbar = bb.d_zbar.as<float>();
    float *partial = t->d_partial.as<float>(), *grad = t->d_grad.as<float>();

    // 1. inverse pass keeping every layer's output (U[li] = snap[li], U[0] = z)
    const bool fm = h0free(t);  // H0-free sweep (features + H1 kept)
    rc = run(c, MODE_LOGPDF, flow, x, theta_raw, nullptr, nullptr, nullptr, lp, batch,
             stream, snap, t->hsave_on ? bb.d_hsave.as<float>() : nullptr, t->lwidth, fm ? 1 : t->lmax_h,
             fm ? bb.d_fsave.as<float>() : nullptr);
    if (rc != DF_OK) return rc;
    // 2. z̄ = z / N
    const float inv_n = 1.f / (float)n_total;
    hipError_t e = launch_scale(zbar, snap, inv_n, batch * P.d, st);
    if (e != hipSuccess) return hip_err(e, "scale kernel launch");
    // 3. reverse sweep, chain order
    if (t->layerwise) {
        rc = lsweep(t, x, theta_raw, batch, inv_n, flow, st);
        if (rc != DF_OK) return rc;
        e = launch_reduce_grads(partial, t->lgrid, t->P, grad, st);
        return e == hipSuccess ? DF_OK : hip_err(e, "gradient reduction launch");
    }
    const int64_t ntiles = (batch + 15) / 16;
    const int grid = (int)std::min<int64_t>(t->grid, (ntiles + kTrainWaves - 1) / kTrainWaves);
    for (const SweepOp& op : t->ops) {
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
        a.p_total = t->P;
        a.inv_n = inv_n;
        a.net = t->nets[op.net];
        e = launch_train_net(P.ht, t->net_nh[op.net], t->amode, a, (unsigned)grid, t->lds_max, st);
        if (e != hipSuccess) return hip_err(e, "train kernel launch");
    }
    // 4. fixed-order reduction of the workgroup partials
    e = launch_reduce_grads(partial, grid, t->P, grad, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "gradient reduction launch");
}

int df_train_logpdf_grad(df_train* t, const float* x, const float* theta, float* logpdf_out, float* grad_x,
                         float* grad_theta, int64_t batch, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (t->layerwise)
        return set_err(DF_ERR_UNSUPPORTED,
                       "df_train_logpdf_grad needs a trainer on the fused sweep; this chain trains layer-wise "
                       "(a conditioner with hidden width > 64, more than one hidden Dense, or more than 4 "
                       "transformed dims in a layer)");
    if (batch == 0) return DF_OK;
    if (!x) return set_err(DF_ERR_INVALID, "null input array");
    df_chain* c = t->c;
    const Plan& P = c->plan;
    if (P.n > 0 && !theta)
        return set_err(DF_ERR_SHAPE, "dimensions θ must match (n, dims...) with n number of trained parameters");
    const int tf = theta_flow(t);
    if (tf < 0) return set_err(DF_ERR_INVALID, "θ bounds not set (df_chain_set_theta_bounds) for DF_THETA_RAW");
    const bool flow = tf == 1;
    if (P.n == 0) grad_theta = nullptr;
    DeviceGuard gd(c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!grad_x && !grad_theta) {  // logpdf alone: the inverse pass without the kept outputs
        if (!logpdf_out) return DF_OK;
        return run(c, MODE_LOGPDF, flow, x, theta, nullptr, nullptr, logpdf_out, nullptr, batch, stream);
    }
    if (t->score_grid == 0) {  // plan the launches: LDS against the workgroup's limit, resident grid
        std::vector<ScoreOp> plan;
        int occ = 0;
        for (size_t i = 0; i < t->ops.size(); ++i) {
            const SweepOp& op = t->ops[i];
            ScoreOp so{op.layer, op.net, -1, op.phase, 0};
            if (op.net >= 0) {
                so.lds = score_net_lds(t->nets[op.net]);
                if (so.lds > kScoreLdsMax)
                    return set_err(DF_ERR_UNSUPPORTED,
                                   "df_train_logpdf_grad: a conditioner needs more than 160 KiB of LDS");
                // an RNVP layer's s-net and t-net (consecutive ops) of the same depth: one launch
                if (!t->score_per_net && op.phase == TR_PHASE_S && i + 1 < t->ops.size() &&
                    t->ops[i + 1].layer == op.layer && t->ops[i + 1].net >= 0 &&
                    t->net_nh[t->ops[i + 1].net] == t->net_nh[op.net] &&
                    so.lds + score_net_lds(t->nets[t->ops[i + 1].net]) <= kScoreLdsMax) {
                    so.net2 = t->ops[i + 1].net;
                    so.lds += score_net_lds(t->nets[so.net2]);
                    ++i;
                }
                int b = 0;
                hipError_t eo = score_net_occupancy(P.ht, t->net_nh[so.net], t->amode, so.net2 >= 0, so.lds, &b);
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
        a.net = t->nets[op.net];
        if (op.net2 >= 0) a.net2 = t->nets[op.net2];
        e = launch_score_net(P.ht, t->net_nh[op.net], t->amode, op.net2 >= 0, a, (unsigned)grid, op.lds, st);
        if (e != hipSuccess) return hip_err(e, "score kernel launch");
    }
    // 4. raw θ: the chain rule of normalize_input
    if (grad_theta && flow) {
        e = launch_score_theta_raw(grad_theta, bounds, bounds + P.n, P.n, batch, st);
        if (e != hipSuccess) return hip_err(e, "θ gradient scaling launch");
    }
    return DF_OK;
}

int df_train_apply(df_train* t, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    DeviceGuard gd(t->c->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (t->debug && t->last_lp) {  // train!(...; debug=true), src/Flows.jl:404-409
        double s = 0.0;
        hipError_t e = hipMemcpyAsync(&s, t->last_lp, sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_err(e, "debug loss read-back");
        const double l = -s / (double)(t->last_n > 0 ? t->last_n : 1);
        if (!std::isfinite(l)) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "non-finite training loss %g: parameters not updated", l);
            return set_err(DF_ERR_NONFINITE, msg);
        }
    }
    hipError_t e = hipSuccess;
    if (t->chain_mode) {
        // Σ dx² per tensor for the ClipNorm (the rules before it applied on the fly), then
        // the whole chain per element in one kernel
        if (t->och_clip >= 0) {
            e = launch_tensor_sumsq(t->d_grad.as<const float>(), t->d_params.as<const float>(),
                                    t->d_toff.as<const int32_t>(), (int)t->toff.size() - 1, t->och, t->och_clip, false,
                                    t->d_sumsq.as<float>(), st);
            if (e != hipSuccess) return hip_err(e, "tensor norm kernel launch");
        }
        e = launch_opt_chain(t->d_params.as<float>(), t->d_grad.as<const float>(), t->d_m.as<float>(),
                             t->d_v.as<float>(), t->d_bt.as<float>(), t->d_sumsq.as<const float>(),
                             t->d_oblocks.as<const OptBlock>(), t->n_oblocks, t->och, st);
        if (e != hipSuccess) return hip_err(e, "optimiser chain kernel launch");
        return repack(t, st);
    }
    e = launch_adam(t->d_params.as<float>(), t->d_grad.as<const float>(), t->d_m.as<float>(), t->d_v.as<float>(),
                    t->P, t->opt.eta, t->opt.beta1, t->opt.beta2, t->opt.epsilon, t->d_bt.as<float>(), st);
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

int df_train_step_graph(df_train* t, const float* x, const float* theta_raw, int64_t batch, int64_t n_total,
                        double* logpdf_sum, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (batch == 0) return DF_OK;
    if (batch < 0) return set_err(DF_ERR_SHAPE, "negative batch size");
    if (n_total < batch) return set_err(DF_ERR_INVALID, "n_total must be >= batch and >= 1");
    DeviceGuard gd(t->c->device);
    if (!gd.ok) return set_err(DF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t now = ++t->use_clock;
    TrainGraph* g = nullptr;
    for (TrainGraph& e : t->graphs)
        if (e.x == x && e.theta == theta_raw && e.lp == logpdf_sum && e.batch == batch && e.n_total == n_total) g = &e;
    if (t->debug) {  // the loss check synchronises: no capture while it is on
        int rc = df_train_gradient(t, x, theta_raw, batch, n_total, logpdf_sum, stream);
        return rc != DF_OK ? rc : df_train_apply(t, stream);
    }
    const int flow_now = theta_flow(t);
    if (g && (g->cap_gen != t->cap_gen || g->partial_gen != t->c->partial_gen ||
              g->flow != flow_now)) {  // stale buffers, or θ now read the other way
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        g->exec = nullptr;
        g->seen = 0;
    }
    if (g && g->exec) {  // replay
        g->last_use = now;
        hipError_t e = hipGraphLaunch(g->exec, st);
        return e == hipSuccess ? DF_OK : hip_err(e, "hipGraphLaunch(train step)");
    }
    if (!g || g->seen == 0) {  // first sight of this key: eager (allocates every buffer it needs)
        if (!g) {
            if (t->graphs.size() >= 4) {  // keep the 4 most recently used keys
                auto lru = t->graphs.begin();
                for (auto it = t->graphs.begin(); it != t->graphs.end(); ++it)
                    if (it->last_use < lru->last_use) lru = it;
                if (lru->exec) (void)hipGraphExecDestroy(lru->exec);
                t->graphs.erase(lru);
            }
            TrainGraph ng;
            ng.x = x;
            ng.theta = theta_raw;
            ng.lp = logpdf_sum;
            ng.batch = batch;
            ng.n_total = n_total;
            t->graphs.push_back(ng);
            g = &t->graphs.back();
        }
        int rc = df_train_gradient(t, x, theta_raw, batch, n_total, logpdf_sum, stream);
        if (rc == DF_OK) rc = df_train_apply(t, stream);
        g->seen = 1;
        g->flow = flow_now;
        g->cap_gen = t->cap_gen;
        g->partial_gen = t->c->partial_gen;
        g->last_use = now;
        return rc;
    }
    // second sight: capture gradient + Adam + repack on a private stream, then replay
    if (!t->cap_stream && hipStreamCreateWithFlags(&t->cap_stream, hipStreamNonBlocking) != hipSuccess)
        return set_err(DF_ERR_HIP, "hipStreamCreate failed");
    hipError_t e = hipStreamBeginCapture(t->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hip_err(e, "hipStreamBeginCapture");
    int rc = df_train_gradient(t, x, theta_raw, batch, n_total, logpdf_sum, t->cap_stream);
    if (rc == DF_OK) rc = df_train_apply(t, t->cap_stream);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(t->cap_stream, &graph);
    if (rc != DF_OK || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc != DF_OK ? rc : hip_err(e, "hipStreamEndCapture");
    }
    if (g->cap_gen != t->cap_gen || g->partial_gen != t->c->partial_gen) {  // a buffer moved while capturing
        (void)hipGraphDestroy(graph);
        return set_err(DF_ERR_HIP, "internal: training buffers reallocated during graph capture");
    }
    e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) {
        g->exec = nullptr;
        return hip_err(e, "hipGraphInstantiate(train step)");
    }
    g->last_use = now;
    e = hipGraphLaunch(g->exec, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "hipGraphLaunch(train step)");
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

}  // extern "C"

namespace {

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

void drop(EpochGraph& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    g = EpochGraph{};
}

// epoch_step as df_train_step_graph runs its step: eagerly at first sight (every buffer the
// step needs is allocated then), captured on the trainer's private stream at the second,
// replayed from then on; a capture that names reallocated buffers, an adjusted η or the
// other θ convention is dropped first.
int epoch_step_graph(df_train* t, EpochGraph& g, int64_t count, hipStream_t st) {
    const int flow_now = theta_flow(t);
    if (g.count != count || g.cap_gen != t->cap_gen || g.partial_gen != t->c->partial_gen || g.flow != flow_now)
        drop(g);
    if (g.exec) {
        const hipError_t e = hipGraphLaunch(g.exec, st);
        return e == hipSuccess ? DF_OK : hip_err(e, "hipGraphLaunch(epoch step)");
    }
    if (!g.seen) {
        const int rc = epoch_step(t, count, st);
        g.seen = 1;
        g.count = count;
        g.flow = flow_now;
        g.cap_gen = t->cap_gen;
        g.partial_gen = t->c->partial_gen;
        return rc;
    }
    if (!t->cap_stream && hipStreamCreateWithFlags(&t->cap_stream, hipStreamNonBlocking) != hipSuccess)
        return set_err(DF_ERR_HIP, "hipStreamCreate failed");
    hipError_t e = hipStreamBeginCapture(t->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hip_err(e, "hipStreamBeginCapture");
    const int rc = epoch_step(t, count, t->cap_stream);
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
        return hip_err(e, "hipGraphInstantiate(epoch step)");
    }
    e = hipGraphLaunch(g.exec, st);
    return e == hipSuccess ? DF_OK : hip_err(e, "hipGraphLaunch(epoch step)");
}

}  // namespace

extern "C" {

int df_train_epoch(df_train* t, const float* x_set, const float* theta_set, int64_t n_samples, const int32_t* order,
                   int64_t batchsize, double* step_logpdf_sum, int64_t* steps_done, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    if (steps_done) *steps_done = 0;
    if (batchsize <= 0) return set_err(DF_ERR_INVALID, "batchsize must be >= 1");
    if (n_samples < 0) return set_err(DF_ERR_SHAPE, "negative sample count");
    if (n_samples == 0) return DF_OK;
    if (n_samples >= (int64_t)1 << 31) return set_err(DF_ERR_SHAPE, "a resident set holds fewer than 2^31 samples");
    if (!x_set) return set_err(DF_ERR_INVALID, "null input array");
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
    const EpochKey key{x_set, theta_set, order, step_logpdf_sum, n_samples, batchsize};
    if (full > t->ecap) {
        for (EpochGraph& g : t->eg) drop(g);
        t->ecap = 0;
        if (t->d_ex.alloc(sizeof(float) * (size_t)full * P.d) != hipSuccess ||
            (P.n > 0 && t->d_eth.alloc(sizeof(float) * (size_t)full * P.n) != hipSuccess))
            return set_err(DF_ERR_NOMEM, "hipMalloc failed (mini-batch staging)");
        t->ecap = full;
    }
    if (!(key == t->ekey))
        for (EpochGraph& g : t->eg) drop(g);
    t->ekey = key;

    hipError_t e = hipMemsetAsync(cursor, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return hip_err(e, "hipMemsetAsync");
    const int64_t steps = (n_samples + batchsize - 1) / batchsize;
    for (int64_t i = 0; i < steps; ++i) {
        const int64_t count = std::min(batchsize, n_samples - i * batchsize);
        // debug mode: the per-step loss check synchronises, so the steps run eagerly
        const int rc = t->debug ? epoch_step(t, count, st) : epoch_step_graph(t, t->eg[count == full ? 0 : 1], count, st);
        if (rc != DF_OK) {
            if (steps_done) *steps_done = i;
            return rc;
        }
    }
    if (steps_done) *steps_done = steps;
    return DF_OK;
}

int df_train_set_debug(df_train* t, int on) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    t->debug = on != 0;
    return DF_OK;
}

int df_train_get_params(df_train* t, float* host_out, int64_t count) {
    if (!t || (!host_out && count > 0)) return set_err(DF_ERR_INVALID, "null pointer");
    if (count != t->P) return set_err(DF_ERR_SHAPE, "count must equal df_train_num_params");
    DeviceGuard gd(t->c->device);
    if (count == 0) return DF_OK;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, t->d_params.get(), sizeof(float) * count, hipMemcpyDeviceToHost);
    return e == hipSuccess ? DF_OK : hip_err(e, "hipMemcpy(params)");
}

int df_train_set_params(df_train* t, const float* host_in, int64_t count) {
    if (!t || (!host_in && count > 0)) return set_err(DF_ERR_INVALID, "null pointer");
    if (count != t->P) return set_err(DF_ERR_SHAPE, "count must equal df_train_num_params");
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
    t->och.p[t->och_eta][0] = eta;
    if (t->och.kind[t->och_eta] == DF_OPT_ADAM) t->opt.eta = eta;
    t->cap_gen++;  // η is a kernel argument of the captured steps: they are re-captured
    return DF_OK;
}

int df_train_num_tensors(const df_train* t, int64_t* count) {
    if (!t || !count) return set_err(DF_ERR_INVALID, "null pointer");
    *count = (int64_t)t->toff.size() - 1;
    return DF_OK;
}

int df_train_tensor_offsets(const df_train* t, int64_t* offsets_out, int64_t count_plus_1) {
    if (!t || !offsets_out) return set_err(DF_ERR_INVALID, "null pointer");
    if (count_plus_1 != (int64_t)t->toff.size())
        return set_err(DF_ERR_SHAPE, "count_plus_1 must equal df_train_num_tensors + 1");
    for (size_t k = 0; k < t->toff.size(); ++k) offsets_out[k] = t->toff[k];
    return DF_OK;
}

int df_train_grad_norms(df_train* t, float* out_dev, void* stream) {
    if (!t) return set_err(DF_ERR_INVALID, "null trainer");
    const int nt = (int)t->toff.size() - 1;
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
