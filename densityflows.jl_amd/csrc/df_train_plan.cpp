// df_train_plan.cpp — build_train_plan: everything df_train_create_opt decides before its
// first device call.  Host arithmetic only (g++, like df_plan.cpp): the rules, the sweep
// form, the fused nets or the layer-wise nets with every packed blob and repack map.
#include "df_train_plan.h"

#include <algorithm>

#include "df_pack.h"

namespace df {
namespace {

int round16(int v) { return (v + 15) / 16 * 16; }

int pow2_tiles(int rows) {
    int t = 1;
    while (16 * t < rows) t *= 2;
    return t;
}

// every activation the plan accepts has a derivative rule (df_train_impl.h act_grad/act_dx)
bool act_trainable(int a) { return a >= DF_ACT_IDENTITY && a <= DF_ACT_SWISH; }

bool act_needs_pre(int a) { return a == DF_ACT_SOFTPLUS || a == DF_ACT_LOGCOSH || a == DF_ACT_SWISH; }

int fail(std::string* err, int code, const char* msg) {
    *err = msg;
    return code;
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
LOp pack_lop(TrainPlan& t, const Plan& P, const LDense& D, bool transposed, bool exact) {
    LOp op;
    const int rows = transposed ? D.in_dim : D.out_dim;
    const int kdim = transposed ? D.out_dim : D.in_dim;
    op.mt = pow2_tiles(rows);
    op.nkq = (kdim + 15) / 16;
    op.chunk_kq = std::max(1, kLChunkBytes / (op.mt * 1024));
    op.frag = (int64_t)t.lblob.size();
    const size_t bytes = (size_t)op.nkq * op.mt * 1024;
    t.lblob.resize(t.lblob.size() + bytes, 0);
    pack::ParamSink<uint8_t> sink(t.lblob, t.ldst, t.lsrc, pack::ParamSink<uint8_t>::WORDS);
    pack::for_each_f32_frag(0, op.nkq, op.mt, pack::k_hidden_quad, [&](int64_t q, int i, int k) {
        if (i >= rows || k >= kdim) return;
        const int orow = transposed ? k : i, icol = transposed ? i : k;  // W[orow, icol]
        const int32_t src = (int32_t)(D.w_off + orow + (int64_t)D.out_dim * icol);
        sink.f32(op.frag + 4 * q, {src, P.trainables[src]});
    });
    // SPLIT planes of a hidden-256 Wᵀ (the ldense_kernel SPLIT instances), and of a first
    // Dense's W0ᵀ over a 256-wide hidden layer (≤ 64 conditioner inputs: the x̄ product
    // of the SPLIT W1ᵀδ1 epilogue)
    if (transposed && (op.mt == 16 || (op.mt <= 4 && op.nkq == 16)) && op.nkq % 2 == 0 && !exact)
        op.sfrag = pack_wt_planes(P, rows, kdim, op.mt, op.nkq / 2, D.w_off, D.out_dim, t.lsblob, t.lsdst, t.lssrc);
    return op;
}

void pack_lbias(TrainPlan& t, const Plan& P, const LDense& D, LOp& op) {
    if (D.b_off < 0) return;
    op.bias = (int64_t)t.lblob.size() / 4;
    t.lblob.resize(t.lblob.size() + (size_t)op.mt * 64, 0);
    float* f = reinterpret_cast<float*>(t.lblob.data()) + op.bias;
    for (int r = 0; r < D.out_dim; ++r) {
        f[r] = P.trainables[D.b_off + r];
        t.ldst.push_back((int32_t)(op.bias + r));
        t.lsrc.push_back(D.b_off + r);
    }
}

int build_lnets(TrainPlan& t, const Plan& P, const TrainPlanOpts& o, std::string* err) {
    for (int li = 0; li < P.n_layers; ++li) {
        const DevLayer& L = P.layers[li];
        if (L.kind == DF_LAYER_NORM) {
            t.ops.push_back({li, -1, TR_PHASE_T});
            continue;
        }
        auto add = [&](int d0, int nd, int phase) -> int {
            LNet net;
            for (int k = 0; k < nd; ++k) {
                const DevDense& DD = P.denses[d0 + k];
                if (!act_trainable(DD.act)) return fail(err, DF_ERR_UNSUPPORTED, "unknown activation");
                LDense D{DD.in_dim, DD.n_out, DD.act, DD.w_off, DD.b_off, {}, {}};
                D.fwd = pack_lop(t, P, D, false, o.exact);
                pack_lbias(t, P, D, D.fwd);
                D.bwd = pack_lop(t, P, D, true, o.exact);
                t.lwidth = std::max({t.lwidth, 16 * D.fwd.mt, 16 * D.bwd.mt});
                if (k + 1 < nd && act_needs_pre(D.act)) net.pre = true;
                net.dn.push_back(D);
            }
            t.lmax_h = std::max(t.lmax_h, nd - 1);
            t.any_pre = t.any_pre || net.pre;
            t.lnets.push_back(net);
            t.ops.push_back({li, (int)t.lnets.size() - 1, phase});
            return DF_OK;
        };
        int rc = DF_OK;
        if (L.kind == DF_LAYER_RNVP) rc = add(L.s_dense0, L.s_ndense, TR_PHASE_S);
        if (rc == DF_OK) rc = add(L.t_dense0, L.t_ndense, TR_PHASE_T);
        if (rc != DF_OK) return rc;
    }
    t.lblob.resize(t.lblob.size() + 16, 0);
    return DF_OK;
}

// Transposed fragments of one net (W0ᵀ, W_hᵀ) appended to t.tblob with
// their trainables index map.
void pack_transposed(TrainPlan& t, const Plan& P, GNet& g, const DevDense& D0, const DevDense* D1, int ht) {
    const int h = g.h_true;
    const size_t base = t.tblob.size();
    g.t_src = (int64_t)base;
    g.off_w0t = 0;
    g.off_ht = ht * 1024;
    const int bytes = ht * 1024 + (D1 ? ht * ht * 1024 : 0);
    g.t_bytes = bytes;
    t.tblob.resize(base + bytes, 0);
    float* f = reinterpret_cast<float*>(t.tblob.data() + base);
    const int64_t f0 = (int64_t)base / 4;
    auto put = [&](int64_t q, int64_t src) {
        f[q] = P.trainables[src];
        t.tdst.push_back((int32_t)(f0 + q));
        t.tsrc.push_back((int32_t)src);
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

int build_nets(TrainPlan& t, const Plan& P, const TrainPlanOpts& o, std::string* err) {
    if (!P.uniform || !P.outv)
        return fail(err, DF_ERR_UNSUPPORTED,
                    "training needs every conditioner in the default _dflt_net shape (hidden width <= 64) "
                    "with <= 4 transformed dims per layer");
    const int ht = P.ht;
    for (int li = 0; li < P.n_layers; ++li) {
        const DevLayer& L = P.layers[li];
        if (L.kind == DF_LAYER_NORM) {
            t.ops.push_back({li, -1, TR_PHASE_T});
            continue;
        }
        const ULayer& U = P.ulayers[li];
        auto add = [&](const UNet& u0, int d0, int nd, int phase) -> int {
            if (u0.nh > 1)
                return fail(err, DF_ERR_UNSUPPORTED, "training supports n_sublayers <= 2 (one hidden Dense)");
            const DevDense& D0 = P.denses[d0];
            const DevDense* D1 = u0.nh == 1 ? &P.denses[d0 + 1] : nullptr;
            const DevDense& DO = P.denses[d0 + nd - 1];
            for (int k = 0; k < nd; ++k)
                if (!act_trainable(P.denses[d0 + k].act)) return fail(err, DF_ERR_UNSUPPORTED, "unknown activation");
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
            if (o.split && D1 && t.amode == trn::AM_RELU && (ht == 2 || ht == 4)) {
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
                g.st_src = pack_wt_planes(P, g.h_true, g.h_true, ht, ht / 2, D1->w_off, g.h_true, t.tsblob, t.tsdst,
                                          t.tssrc);
            }
            t.nets.push_back(g);
            t.net_nh.push_back(u0.nh);
            t.ops.push_back({li, (int)t.nets.size() - 1, phase});
            return DF_OK;
        };
        int rc = DF_OK;
        if (L.kind == DF_LAYER_RNVP) rc = add(U.s, L.s_dense0, L.s_ndense, TR_PHASE_S);
        if (rc == DF_OK) rc = add(U.t, L.t_dense0, L.t_ndense, TR_PHASE_T);
        if (rc != DF_OK) return rc;
    }
    t.tblob.resize(t.tblob.size() + 16, 0);
    return DF_OK;
}

// The H0-free sweep (TrainPlan::fmode) applies when the inverse pass runs on the wide SPLIT
// kernel and every conditioner is its shape: Dense(≤ 32, 256, relu), Dense(256, 256, relu),
// Dense(256, ≤ 32), with the fused front and the split dW1.
bool fmode_eligible(const TrainPlan& t, const Plan& P, const TrainPlanOpts& o) {
    if (!t.layerwise || !P.wide || o.no_wide || !o.wsplit || o.exact || P.uniform) return false;
    if (t.sweep_req != DF_SWEEP_AUTO && t.sweep_req != DF_SWEEP_H0FREE && t.sweep_req != DF_SWEEP_LAYERWISE)
        return false;
    for (const LNet& N : t.lnets) {
        if (N.pre || N.dn.size() != 3) return false;
        const LDense &D0 = N.dn[0], &D1 = N.dn[1], &D2 = N.dn[2];
        if (D0.act != DF_ACT_RELU || D1.act != DF_ACT_RELU) return false;
        if (D0.in_dim > 32 || D0.out_dim != 256 || D1.in_dim != 256 || D1.out_dim != 256) return false;
        // (the feature rows the split dW0 / H0 recompute read are 32 floats: 16 · bwd.mt <= 32)
        if (D2.fwd.mt > 2 || D0.bwd.mt > 2 || D1.bwd.sfrag < 0) return false;
    }
    return true;
}

// The rules of df_train_create_opt, validated (include/densityflows_hip.h: limits and values) into the
// kernels' OptChain, with och_clip, och_eta and the chain's Adam (its β seed and advance βᵗ).
int check_rules(const df_opt_rule* rules, int n_rules, TrainPlan& t, std::string* err) {
    if (!rules && n_rules > 0) return fail(err, DF_ERR_INVALID, "null pointer");
    if (n_rules < 1)
        return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: no rule (a chain needs an Adam or a Descent)");
    if (n_rules > kOptMaxRules) return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: more than 8 rules");
    int i_adam = -1, i_descent = -1;
    OptChain& och = t.och;
    och.n = n_rules;
    for (int r = 0; r < n_rules; ++r) {
        const float* p = rules[r].p;
        och.kind[r] = rules[r].kind;
        switch (rules[r].kind) {
            case DF_OPT_ADAM:
                if (i_adam >= 0) return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: more than one Adam");
                if (!(p[0] >= 0.f) || !(p[1] >= 0.f && p[1] < 1.f) || !(p[2] >= 0.f && p[2] < 1.f) || !(p[3] >= 0.f))
                    return fail(err, DF_ERR_INVALID, "invalid Adam hyper-parameters");
                i_adam = r;
                t.adam = df_adam{p[0], p[1], p[2], p[3]};
                for (int k = 0; k < 4; ++k) och.p[r][k] = p[k];
                break;
            case DF_OPT_DESCENT:
                if (!(p[0] >= 0.f)) return fail(err, DF_ERR_INVALID, "invalid Descent learning rate (η >= 0)");
                if (i_descent < 0) i_descent = r;
                och.p[r][0] = p[0];
                break;
            case DF_OPT_CLIP_GRAD:
                if (!(p[0] > 0.f)) return fail(err, DF_ERR_INVALID, "invalid ClipGrad bound (δ > 0)");
                och.p[r][0] = p[0];
                break;
            case DF_OPT_CLIP_NORM:
                if (t.och_clip >= 0) return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: more than one ClipNorm");
                if (i_adam >= 0)
                    return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: ClipNorm after Adam (it stands before it)");
                if (!(p[0] > 0.f)) return fail(err, DF_ERR_INVALID, "invalid ClipNorm bound (ω > 0)");
                t.och_clip = r;
                och.p[r][0] = p[0];
                break;
            case DF_OPT_WEIGHT_DECAY:
                if (!(p[0] >= 0.f)) return fail(err, DF_ERR_INVALID, "invalid WeightDecay factor (λ >= 0)");
                och.p[r][0] = p[0];
                break;
            default:
                return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: unknown rule (df_opt_kind)");
        }
    }
    if (i_adam < 0 && i_descent < 0)
        return fail(err, DF_ERR_UNSUPPORTED, "OptimiserChain: no terminal rule (a chain needs an Adam or a Descent)");
    t.och_eta = i_adam >= 0 ? i_adam : i_descent;
    t.chain_mode = !(och.n == 1 && och.kind[0] == DF_OPT_ADAM);
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

}  // namespace

int build_train_plan(const Plan& P, const TrainPlanOpts& o, const df_opt_rule* rules, int n_rules, TrainPlan* out,
                     std::string* err) {
    TrainPlan t;
    int rc = check_rules(rules, n_rules, t, err);
    if (rc != DF_OK) return rc;
    const int form = o.sweep & ~DF_SWEEP_SEPARATE;
    if (form < DF_SWEEP_AUTO || form > DF_SWEEP_LAYERWISE || (o.sweep & ~(DF_SWEEP_SEPARATE | 7)))
        return fail(err, DF_ERR_INVALID, "unknown sweep form");
    if (form == DF_SWEEP_FUSED && (o.sweep & DF_SWEEP_SEPARATE))
        return fail(err, DF_ERR_INVALID, "DF_SWEEP_SEPARATE applies to the layer-wise forms");
    t.sweep_req = form;
    t.separate = (o.sweep & DF_SWEEP_SEPARATE) != 0;
    t.n_params = (int64_t)P.trainables.size();
    if (!tensor_table(P, t.toff))
        return fail(err, DF_ERR_INVALID, "internal: the Dense tensors do not tile the flat trainables");
    t.amode = P.relu_only ? trn::AM_RELU : trn::AM_Y;
    for (const DevDense& D : P.denses)
        if (act_needs_pre(D.act) && !P.relu_only) t.amode = trn::AM_PRE;
    // the update kernel's workgroup → tensor table (built once: no workgroup spans two tensors)
    if (t.chain_mode)
        for (int k = 0; k + 1 < (int)t.toff.size(); ++k)
            for (int32_t b = t.toff[k]; b < t.toff[k + 1]; b += kOptThreads)
                t.oblocks.push_back({b, std::min<int32_t>(kOptThreads, t.toff[k + 1] - b), k});
    // fused per-net kernel when every conditioner fits its registers, else layer-wise: a
    // fused attempt that fails is a value of its own, dropped whole
    rc = DF_ERR_UNSUPPORTED;
    if (form == DF_SWEEP_AUTO || form == DF_SWEEP_FUSED) {
        TrainPlan fused = t;
        rc = build_nets(fused, P, o, err);
        if (rc == DF_OK) t = std::move(fused);
    }
    if (rc == DF_ERR_UNSUPPORTED && form != DF_SWEEP_FUSED) {
        t.layerwise = true;
        rc = build_lnets(t, P, o, err);
    }
    if (rc != DF_OK) return rc;
    t.fmode = fmode_eligible(t, P, o);
    // an explicit form the chain cannot take: the H0-free sweep's shape, or kept
    // activations of a chain whose inverse pass (the specialised kernel) keeps none
    if (t.layerwise && form == DF_SWEEP_H0FREE && !t.fmode)
        return fail(err, DF_ERR_UNSUPPORTED,
                    "DF_SWEEP_H0FREE needs wide SPLIT nets Dense(<=32,256,relu), Dense(256,256,relu), Dense(256,<=32)");
    if (t.layerwise && form == DF_SWEEP_KEPT && P.uniform)
        return fail(err, DF_ERR_UNSUPPORTED, "DF_SWEEP_KEPT needs a chain on the generic or wide kernel");
    *out = std::move(t);
    return DF_OK;
}

}  // namespace df
