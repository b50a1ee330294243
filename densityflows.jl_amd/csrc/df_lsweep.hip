// df_lsweep.hip — the reverse sweep of the layer-wise training path (df_ltrain.h): the
// launches of one df_train_gradient on a chain whose conditioners the fused per-net kernel
// cannot hold.  Host code only; the kernels are in df_ltrain.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "df_trainer.h"

using namespace df;
using namespace df::api;

namespace {

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
    const float* wj;          // weighted loss: j̄ per sample (nullptr: inv_n)
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

    bool keeps(const SweepOp& op) const { return t->hsave_on && !t->tp.lnets[op.net].pre; }
    static int net_slot(const SweepOp& op) { return 2 * op.layer + (op.phase == TR_PHASE_T ? 1 : 0); }
    // fmode: the net's feature rows [B][32] (written by the inverse pass)
    float* fbuf(const SweepOp& op) const { return t->bb.d_fsave.as<float>() + (int64_t)net_slot(op) * batch * 32; }
    // whether the net's backward front is the fused couple_bwd kernel (kept activations,
    // <= 32 outputs, hidden <= 256)
    bool fused_front(const SweepOp& op) const {
        const LNet& N = t->tp.lnets[op.net];
        const int nd = (int)N.dn.size();
        return nd >= 2 && keeps(op) && N.dn[nd - 1].fwd.mt <= 2 && N.dn[0].bwd.mt <= 4;
    }
    // H_k of a net: kept by the inverse pass, or recomputed into the shared buffers
    float* Hbuf(const SweepOp& op, int k) const {
        float* hsave = t->bb.d_hsave.as<float>();
        const int64_t W = t->tp.lwidth;
        if (fm) return k == 1 ? hsave + (int64_t)net_slot(op) * batch * W : nullptr;  // H1 only
        return keeps(op) ? hsave + ((int64_t)net_slot(op) * t->tp.lmax_h + k) * batch * W : t->bb.d_lh[k].as<float>();
    }
    // ȳ and the δ of the last hidden Dense alternate between two buffers from net to
    // net: a merged launch writes net i+1's while net i's dW products read net i's
    float* ybuf(int p) const { return t->bb.d_lyp[p].as<float>(); }
    float* dbuf(const SweepOp& op, int k, int p) const {
        return k == (int)t->tp.lnets[op.net].dn.size() - 2 ? t->bb.d_lbp[p].as<float>() : t->bb.d_ld[k].as<float>();
    }
    const uint8_t* sfrag_of(const LOp& op, int in_kind, int epi) const {
        return (lsplit && op.sfrag >= 0 && ldense_split_supported(op.mt, in_kind, epi)) ? lsb + op.sfrag : nullptr;
    }
    // σ' argument of Dense k's output: H_k, or the stored σ'(x_k)
    void dact(const SweepOp& op, int k, LDenseArgs& a) const {
        const LNet& N = t->tp.lnets[op.net];
        a.hprev = N.pre ? t->bb.d_lv[k].as<float>() : Hbuf(op, k);
        a.dact = N.pre ? trn::kDactStored : N.dn[k].act;
    }
    LDenseArgs base_args(const SweepOp& op) const {
        LDenseArgs b{};
        fill_layer_args(b, t, op.layer, op.phase, x, theta, flow, batch);
        b.n_in = t->tp.lnets[op.net].dn[0].in_dim;
        b.zbar = t->bb.d_zbar.as<float>();
        b.ebuf = t->bb.d_ebuf.as<float>();
        b.inv_n = inv_n;
        b.wj = wj;
        b.ld_in = b.ld_out = b.ld_h = b.ld_x = t->tp.lwidth;
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
        const LNet& N = t->tp.lnets[op.net];
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
            a.dwo_p_total = t->tp.n_params;
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
    const LNet& N = t->tp.lnets[op.net];
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
    const LNet& N = t->tp.lnets[op.net];
    const int nd = (int)N.dn.size();
    const int W = t->tp.lwidth;
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
        w.p_total = t->tp.n_params;
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
    const LNet& N = t->tp.lnets[op.net];
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
    if (t->tp.separate || rest.size() > 3) {  // DF_SWEEP_SEPARATE
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
    if (oi + 1 < t->tp.ops.size() && t->tp.ops[oi + 1].net >= 0 && s.fused_front(t->tp.ops[oi + 1])) {
        const Front f = s.front(t->tp.ops[oi + 1], s.par ^ 1);
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

}  // namespace

hipError_t lsweep_set_lds_limits() {
    hipError_t e = set_ldense_lds_limit(kLdenseLdsLimit);
    if (e == hipSuccess) e = set_couple_bwd_lds_limit(kCoupleBwdLdsLimit);
    if (e == hipSuccess) e = set_sweep_lds_limit(kSweepLdsLimit);
    return e;
}

// Reverse sweep of the layer-wise path (chain order; see df_ltrain.h).
int lsweep(df_train* t, const float* x, const float* theta, int64_t batch, float inv_n, const float* wj, bool flow,
           hipStream_t st) {
    df_chain* c = t->c;
    const int64_t ntiles = (batch + 15) / 16;
    const unsigned dgrid =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(c->grid_cus, (ntiles + kWavesPerBlock * kLTiles - 1) /
                                                                              (kWavesPerBlock * kLTiles)));
    LSweep s{t, c, x, theta, batch, inv_n, flow, st, dgrid, t->d_lblob.as<const uint8_t>(),
             t->d_lblob.as<const float>(), t->d_lsblob.as<const uint8_t>(), !c->exact, h0free(t), wj};
    for (size_t oi = 0; oi < t->tp.ops.size() && s.rc == DF_OK; ++oi) {
        const SweepOp& op = t->tp.ops[oi];
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
