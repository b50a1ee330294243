// df_score_impl.h — per-sample input gradients of logpdf through the conditioner nets.
//
// ∂lp_j/∂x_j and ∂lp_j/∂θ_j for lp = logpdf(MvNormal(0,I), z) + ldj (what Zygote gets from
// rrule(RNVP_backward)'s ū, src/affine/RNVP.jl:137-141; NICE.jl:102-111).  The sweep is
// the trainer's (df_train_impl.h), chain order over the kept layer outputs U[li], with
// the seed z̄ = -z, j̄ = 1 and nothing summed over the batch.  Every wave owns 16-sample
// tiles (persistent grid).  Per tile and net:
//   forward recompute   x → A0 = σ0(W0 x + b0) [→ A1 = σh(W1 A0 + b1)] → y = σo(W3 h + b3)
//                       on the exact-f32 fragments (GNet::u), the trainer's device functions;
//   coupling pullback   s-net: s̄ = -z̄_af·z_af - 1       (z_af = U[li]_af)
//                       t-net: t̄ = -z̄_af·exp(-s)  (NICE: t̄ = -z̄_af),
//                              then ū_af = z̄_af·exp(-s);
//   back-propagation    δ = (Wᵀ ȳ) ⊙ σ' on v_mfma_f32_16x16x4_f32, each accumulator the next
//                       B operand (W_outᵀ from the forward fragment, W_hᵀ and W0ᵀ from the
//                       trainer's transposed fragments);
//   x̄ = W0ᵀ δ0         the cotangent of vcat(θ, u)[axis_nn]: a row whose state slot is a
//                       dimension adds into z̄ of that (identity) dim, a row whose slot is a
//                       θ adds into θ̄ of that θ.
// Two launch forms.  PAIR (an RNVP layer whose two nets have the same depth): one launch
// per layer holds both nets in LDS, gathers the features, z̄ and U[li] once, runs the
// s-net then the t-net (exp(-s) stays in registers) and writes x̄ of both in one store.
// Otherwise one launch per net, the s-net's exp(-s) going through ebuf, as the trainer.
// A sample's z̄ and θ̄ rows are read and written only by the 4 lanes (j, g = 0..3) that hold
// it, each its own columns; launches are stream-ordered, so the result is bitwise
// reproducible.  Lanes past the batch neither load nor store.  No dW / db, no LDS
// transposes, no workgroup reduction, no atomics: after the weights are in LDS a wave
// never synchronises with another.
#pragma once

#include "df_train_impl.h"

namespace df {

#ifndef DF_SCORE_WAVES_PER_EU
#define DF_SCORE_WAVES_PER_EU 3
#endif

// One conditioner net over one 16-sample tile: recompute, pullback, back-propagation.
//   sph: the s-net (aux = z_af; ee ← exp(-s));  else the t-net (aux = exp(-s) of an RNVP
//   layer, ee ← aux; NICE: ee ← 1).
// x̄ = W0ᵀ δ0 is ADDED to xb, so the t-net's call continues the s-net's accumulator.
template <int HT, int NH, int AM>
__device__ __forceinline__ void score_net_tile(const uint8_t* fwl, const uint8_t* twl, const GNet& G,
                                               const float (&w3a)[HT], bool x4, int n_af, bool valid, bool sph,
                                               bool rnvp, const float (&xin)[1][4], const float (&zb)[4],
                                               const float (&aux)[4], float (&ee)[4], f32x4& xb) {
    using namespace trn;
    constexpr bool RELU = (AM == AM_RELU);
    constexpr bool PRE = (AM == AM_PRE);
    const UNet& N = G.u;
    const int lane = threadIdx.x & 63, g = lane >> 4;
    // ---- forward recompute ----
    f32x4 A0[1][HT], A1[1][HT];
    constexpr int NP = PRE ? HT : 1;
    f32x4 D0[NP], D1[NP];  // AM_PRE: σ'(pre) of the first / hidden Dense
    uni::dense_first<HT, 1>(fwl, N, xin, A0);
    if constexpr (PRE) {
        uni::bias_act<HT, 1, false>(fwl + N.off_b0, DF_ACT_IDENTITY, A0, !N.fold0);
        act_keep_grad<HT>(N.act0, A0[0], D0);
    } else {
        uni::bias_act<HT, 1, RELU>(fwl + N.off_b0, N.act0, A0, !N.fold0);
    }
    if constexpr (NH == 1) {
        uni::dense_hidden<HT, 1>(fwl + N.off_h, A0, A1);
        if constexpr (PRE) {
            uni::bias_act<HT, 1, false>(fwl + N.off_h + HT * HT * 1024, DF_ACT_IDENTITY, A1);
            act_keep_grad<HT>(N.acth, A1[0], D1);
        } else {
            uni::bias_act<HT, 1, RELU>(fwl + N.off_h + HT * HT * 1024, N.acth, A1);
        }
    }
    const f32x4(&H)[1][HT] = NH ? A1 : A0;
    f32x4 o[1];
    float dfo[4] = {1.f, 1.f, 1.f, 1.f};  // AM_PRE: σo'(pre) of the output Dense
    if constexpr (PRE) {
        uni::out_valu<HT, 1, true>(fwl, N, H, o);  // pre-activation (no σo)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = o[0][k];
            const float y = (N.act_out == DF_ACT_IDENTITY) ? x : impl::act_fn(N.act_out, x);
            dfo[k] = act_dx(N.act_out, x, y);
            o[0][k] = y;
        }
    } else {
        uni::out_valu<HT, 1, RELU>(fwl, N, H, o);
    }

    // ---- coupling pullback → ȳ (every lane group holds all outputs of sample j) ----
    float dout[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        dout[k] = 0.f;
        ee[k] = 1.f;
        if (k < n_af && valid) {
            if (sph) {
                ee[k] = expf(-o[0][k]);
                dout[k] = -zb[k] * aux[k] - 1.f;  // s̄ = -z̄_af·z_af - j̄
            } else {
                if (rnvp) ee[k] = aux[k];
                dout[k] = -zb[k] * ee[k];         // t̄ = -z̄_af·exp(-s)
            }
            if (PRE) {
                if (N.act_out != DF_ACT_IDENTITY) dout[k] = dout[k] * dfo[k];
            } else if (!RELU && N.act_out != DF_ACT_IDENTITY) {
                dout[k] = dout[k] * act_grad(N.act_out, o[0][k]);
            }
        }
    }

    // ---- output Dense: h̄ = W3ᵀ ȳ, δ = h̄ ⊙ σ'(h) ----
    f32x4 hb[1][HT];
    {
        const float bk = g == 0 ? dout[0] : g == 1 ? dout[1] : g == 2 ? dout[2] : dout[3];
#pragma unroll
        for (int m = 0; m < HT; ++m) hb[0][m] = mfma4(w3a[m], bk, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    if constexpr (PRE) {
        const f32x4(&DH)[NP] = NH ? D1 : D0;
#pragma unroll
        for (int m = 0; m < HT; ++m) hb[0][m] = hb[0][m] * DH[m];
    } else {
        mul_act_grad<HT, RELU>(NH ? N.acth : N.act0, H[0], hb[0]);
    }

    // ---- hidden Dense: δ0 = (W1ᵀ δ) ⊙ σ'(A0) ----
    f32x4 d0[1][HT];
    if constexpr (NH == 1) {
        uni::dense_hidden<HT, 1>(twl + G.off_ht, hb, d0);
        if constexpr (PRE) {
#pragma unroll
            for (int m = 0; m < HT; ++m) d0[0][m] = d0[0][m] * D0[m];
        } else {
            mul_act_grad<HT, RELU>(N.act0, A0[0], d0[0]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < HT; ++m) d0[0][m] = hb[0][m];
    }

    // ---- first Dense: x̄ = W0ᵀ δ0; added to xb: lane (g, j) holds x̄[4g + r][j] in register r ----
    if (x4) {
        // Block b = lane >> 2 takes samples 4(b & 3).. over the hidden rows of lane group
        // g = b >> 2 — exactly the δ0 values lane (g, j) holds — with W0ᵀ[i][h] from the
        // fragment of lane (g, i), i < 4 (at slot i + 4g of the compacted copy).  Each lane
        // group ends with its partial sums of rows 0..3; the caller adds the four groups.
#pragma unroll
        for (int kq = 0; kq < HT; ++kq) {
            const f32x4 w = impl::lds4(twl + G.off_w0t + kq * 1024 + ((lane & 3) + 4 * g) * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) xb = mfma4x4(w[r], d0[0][kq][r], xb);
        }
    } else {
#pragma unroll
        for (int kq = 0; kq < HT; ++kq) {
            const f32x4 w = impl::lds4(twl + G.off_w0t + kq * 1024 + lane * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) xb = mfma4(w[r], d0[0][kq][r], xb);
        }
    }
}

template <int HT, int NH, int AM, bool PAIR>
__global__ void __launch_bounds__(kScoreThreads, DF_SCORE_WAVES_PER_EU) score_net_kernel(ScoreArgs a) {
    constexpr int NT = kScoreThreads;
    constexpr int INP = 16 * HT;
    constexpr int NN = PAIR ? 2 : 1;  // nets of this launch: (s, t) or one
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const GNet& G = a.net;
    const GNet& G2 = PAIR ? a.net2 : a.net;
    uint8_t* fw[NN];
    uint8_t* tw[NN];
    fw[0] = smem;
    tw[0] = smem + G.fwd_bytes;
    if constexpr (PAIR) {
        fw[1] = tw[0] + G.t_bytes;
        tw[1] = fw[1] + G2.fwd_bytes;
    }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int d = a.d, n = a.n, n_af = a.n_af;
    const bool sph = PAIR || (a.phase == TR_PHASE_S);  // the (first) net of this launch is an s-net
    const bool rnvp = PAIR || (a.kind == DF_LAYER_RNVP);
    // ≤ 4 conditioner inputs: x̄ on v_mfma_f32_4x4x1_16b_f32 (score_net_tile)
    const bool x4 = G.n_in <= 4;

#pragma unroll
    for (int k = 0; k < NN; ++k) {  // the nets' forward and transposed fragments → LDS
        const GNet& Gk = k ? G2 : G;
        const f32x4* src = reinterpret_cast<const f32x4*>(a.blob + Gk.fwd_src);
        for (int i = tid; i < Gk.fwd_bytes / 16; i += NT) reinterpret_cast<f32x4*>(fw[k])[i] = src[i];
        const f32x4* srt = reinterpret_cast<const f32x4*>(a.tblob + Gk.t_src);
        int t0 = 0;
        if (x4) {
            // W0ᵀ for the 4x4x1 x̄, which takes the fragments of lanes (lane & 3) + 16g: those 16
            // per k-quad go to slots (lane & 3) + 4g, one 256-byte run (train_net_kernel's copy)
            const int w0 = Gk.off_w0t / 16;
            for (int i = tid; i < HT * 16; i += NT) {
                const int kq = i >> 4, c = i & 15;
                reinterpret_cast<f32x4*>(tw[k])[w0 + kq * 64 + c] = srt[w0 + kq * 64 + (c & 3) + 16 * (c >> 2)];
            }
            t0 = Gk.off_ht / 16;  // W_hᵀ follows W0ᵀ (pack_transposed)
        }
        for (int i = t0 + tid; i < Gk.t_bytes / 16; i += NT) reinterpret_cast<f32x4*>(tw[k])[i] = srt[i];
    }
    __syncthreads();

    // h̄ = W_outᵀ ȳ: A = W_out[g][16m + j] (a loop-invariant float per row tile, 0 for
    // g >= n_af), B = ȳ[g] of sample j — the k = 4 slots are the ≤ 4 outputs
    float w3a[NN][HT];
#pragma unroll
    for (int k = 0; k < NN; ++k)
#pragma unroll
        for (int m = 0; m < HT; ++m)
            w3a[k][m] = (g < n_af)
                            ? reinterpret_cast<const float*>(fw[k] + (k ? G2 : G).u.off_out)[g * INP + 16 * m + j]
                            : 0.f;

    // Loop-invariant gather tables of this lane (a layer's two nets read the same features):
    // conditioner feature k = 4r + g of vcat(θ, u)[axis_nn] (kind 0 zero, 1 θ, 2 u, 3 the
    // folded bias's 1), the x̄ targets of row f = 4g + r (a z̄ column for an identity dim, a
    // θ̄ column for a θ, none otherwise) and the transformed dims (z̄ columns).  One byte
    // per r (0xff: none).
    int xcode[4];
    uint32_t zxp8 = 0, thp8 = 0, afp8 = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        xcode[r] = 0;
        if (r < G.u.ks) {
            const int slot = a.feat[4 * r + g];
            if (slot < n) xcode[r] = 1 << 8 | slot;
            else if (slot < n + d) xcode[r] = 2 << 8 | (slot - n);
            else if (slot == n + d + 3) xcode[r] = 3 << 8;  // folded first-Dense bias (df_plan.cpp pass 1c)
        }
        const int f = 4 * g + r;
        const int fs = (f < G.n_in) ? a.feat[f] : -1;
        zxp8 |= (uint32_t)((fs >= n && fs < n + d) ? fs - n : 0xff) << (8 * r);
        thp8 |= (uint32_t)((a.thbar && fs >= 0 && fs < n) ? fs : 0xff) << (8 * r);
        afp8 |= (uint32_t)((r < n_af) ? a.af[r] - n : 0xff) << (8 * r);
    }
    auto zxc = [&](int r) { return (int)((zxp8 >> (8 * r)) & 0xffu); };
    auto thc = [&](int r) { return (int)((thp8 >> (8 * r)) & 0xffu); };
    auto afc = [&](int r) { return (int)((afp8 >> (8 * r)) & 0xffu); };

    const int64_t ntiles = (a.batch + 15) / 16;
    const int64_t pstride = (int64_t)gridDim.x * kScoreWaves;
    for (int64_t p = (int64_t)blockIdx.x * kScoreWaves + wave; p < ntiles; p += pstride) {
        const int64_t s = p * 16 + j;
        const bool valid = s < a.batch;
        // The weights in LDS are loop-invariant: behind an offset the compiler cannot see
        // through, their loads stay at their uses instead of being hoisted out of the tile
        // loop into registers held across it (HT = 4 then spills).
        int zo = 0;
        asm volatile("" : "+v"(zo));

        // ---- conditioner input, features k = 4r + g of vcat(θ, u)[axis_nn] ----
        float xin[1][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kind = xcode[r] >> 8, off = xcode[r] & 0xff;
            float v = 0.f;
            if (valid && kind == 1) {
                v = a.theta[s * n + off];
                if (a.tmin) {  // normalize_input (Data.jl:213-218)
                    const float lo = a.tmin[off], diff = a.tmax[off] - lo;
                    v = (diff == 0.f) ? 0.f : (v - lo) / diff;
                }
            }
            if (valid && kind == 2) v = a.u_in[s * d + off];
            if (valid && kind == 3) v = 1.f;
            xin[0][r] = v;
        }
        // z̄ of the transformed dims and u_out of those dims (an s-net) or exp(-s) (a t-net
        // launched alone); z̄ / θ̄ of the x̄ targets: issued here, used after the MFMA chains
        float zb[4], aux[4], zxv[4], thv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool af_ok = valid && afc(r) != 0xff;
            zb[r] = af_ok ? a.zbar[s * d + afc(r)] : 0.f;
            aux[r] = 1.f;
            if (af_ok) {
                if (sph) aux[r] = a.u_out[s * d + afc(r)];
                else if (rnvp) aux[r] = a.ebuf[s * 4 + r];
            }
            zxv[r] = (valid && zxc(r) != 0xff) ? a.zbar[s * d + zxc(r)] : 0.f;
            thv[r] = (valid && thc(r) != 0xff) ? a.thbar[s * n + thc(r)] : 0.f;
        }

        float ee[4];
        f32x4 xb = f32x4{0.f, 0.f, 0.f, 0.f};
        score_net_tile<HT, NH, AM>(fw[0] + zo, tw[0] + zo, G, w3a[0], x4, n_af, valid, sph, rnvp, xin, zb, aux, ee,
                                   xb);
        if constexpr (PAIR) {  // the t-net with the s-net's exp(-s)
            float es[4] = {ee[0], ee[1], ee[2], ee[3]};
            score_net_tile<HT, NH, AM>(fw[1] + zo, tw[1] + zo, G2, w3a[1], x4, n_af, valid, false, true, xin, zb, es,
                                       ee, xb);
        } else if (sph && g == 0 && valid) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n_af) a.ebuf[s * 4 + k] = ee[k];
        }
        if (x4) {  // the 4x4x1 x̄ left each lane group its partial sums of rows 0..3
#pragma unroll
            for (int r = 0; r < 4; ++r) xb[r] = uni::xgroup_sum(xb[r]);
        }
        if (valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (zxc(r) != 0xff) a.zbar[s * d + zxc(r)] = zxv[r] + xb[r];
                if (thc(r) != 0xff) a.thbar[s * n + thc(r)] = thv[r] + xb[r];
            }
            if ((PAIR || !sph) && rnvp && g == 0) {  // ū_af = z̄_af·exp(-s)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (afc(k) != 0xff) a.zbar[s * d + afc(k)] = zb[k] * ee[k];
            }
        }
    }
}

template <int HT, int NH, int AM, bool PAIR>
void* score_kernel_ptr() {
    return reinterpret_cast<void*>(&score_net_kernel<HT, NH, AM, PAIR>);
}

}  // namespace df
