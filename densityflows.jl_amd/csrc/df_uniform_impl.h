// df_uniform_impl.h — the specialised fused kernel for chains whose coupling
// layers all use the reference's default conditioner shape (_dflt_net,
// src/Layers.jl:33-50): Dense(in, H, σ), nh × Dense(H, H, σ), Dense(H, out),
// with H = 16·HT exactly, in <= 16, and each net resident in ONE LDS stage.
// Same numerics and data flow as the generic kernel (df_chain_impl.h) with
// every width known at compile time: no per-tile guards, ping-pong
// accumulators instead of register copies, compact per-net descriptors.
#pragma once

#include <type_traits>

#include "df_chain_impl.h"

namespace df {
namespace uni {


using impl::lds4;
using impl::mfma4;
using impl::Stager;

// relu(x) = max(0, x) as ONE v_max_i32 on the bit pattern: non-negative floats
// order like their integer images; negative floats (and -0) map to +0; a NaN
// with the sign bit clear propagates as in Julia.  A NaN with the sign bit set orders
// below zero and becomes +0, where Julia's max returns NaN — and such NaNs do occur:
// from an x86 host (0f0/0f0), and on the device from x - t and -s, which flip the sign
// of the NaN they are handed.  A NaN sample can therefore leave with finite transformed
// dims (tests/test_gpu_nonfinite.py).  The IEEE maximum (one v_maximum3_f32,
// impl::relu of the generic kernel) propagates both, but measured +0.3 % cycles per
// launch on the config-2 SPLIT kernel, outside the parent's run-to-run spread.
__device__ __forceinline__ float relu_fast(float x) {
    return __int_as_float(__builtin_elementwise_max(__float_as_int(x), 0));
}

// Σ over the 4 lane groups of a wave (lanes l, l^16, l^32, l^48) without LDS:
// gfx950 v_permlane16_swap / v_permlane32_swap.  Every lane gets the bitwise
// identical total ((p0+p1)+(p2+p3), commutations only).
__device__ __forceinline__ float xgroup_sum(float p) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
    const float q = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(q), __float_as_uint(q), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}


// acc = W·x, x = the state features vcat(θ,z)[axis_nn] (<= 16 of them).
// Compact fragments: [m][r < ks][lane] f32, k = 4r + lane_group.
// KS > 0: the chain-wide k-step count is a compile-time constant (FAST variant).
template <int HT, int TT, int KS = 0>
__device__ __forceinline__ void dense_first(const uint8_t* buf, const UNet& N, const float (&xin)[TT][4],
                                            f32x4 (&acc)[TT][HT]) {
    const int lane = threadIdx.x & 63;
    const float* wb = reinterpret_cast<const float*>(buf + N.off_w0) + lane;
    const int ks = KS > 0 ? KS : N.ks;
    if constexpr (KS > 0) {  // first k-step starts from an inline-zero accumulator
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const float w = wb[m * KS * 64];
#pragma unroll
            for (int t = 0; t < TT; ++t) acc[t][m] = mfma4(w, xin[t][0], f32x4{0.f, 0.f, 0.f, 0.f});
        }
#pragma unroll
        for (int r = 1; r < KS; ++r)
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const float w = wb[(m * KS + r) * 64];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][m] = mfma4(w, xin[t][r], acc[t][m]);
            }
        return;
    }
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int m = 0; m < HT; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r < ks) {
#pragma unroll
            for (int m = 0; m < HT; ++m) {
                const float w = wb[(m * ks + r) * 64];
#pragma unroll
                for (int t = 0; t < TT; ++t) acc[t][m] = mfma4(w, xin[t][r], acc[t][m]);
            }
        }
    }
}

// out = W·in over a full H×H Dense (fragments [kq][m][lane][4] at wb).
// m-tiles are processed in pairs: two interleaved accumulator chains (64
// cycles apart >= the 40-cycle MFMA dependency latency) and only 2×2
// fragment registers in flight (next k-quad prefetched).
template <int HT, int TT>
__device__ __forceinline__ void dense_hidden(const uint8_t* wb, const f32x4 (&in)[TT][HT], f32x4 (&out)[TT][HT]) {
    const int lane = threadIdx.x & 63;
    wb += lane * 16;
    constexpr int MB = HT < 2 ? HT : 2;
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int m = 0; m < HT; ++m) out[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m0 = 0; m0 < HT; m0 += MB) {
        f32x4 w[2][MB];
#pragma unroll
        for (int mm = 0; mm < MB; ++mm) w[0][mm] = lds4(wb + (m0 + mm) * 1024);
#pragma unroll
        for (int kq = 0; kq < HT; ++kq) {
            const int cb = kq & 1;
            if (kq + 1 < HT) {
#pragma unroll
                for (int mm = 0; mm < MB; ++mm) w[cb ^ 1][mm] = lds4(wb + ((kq + 1) * HT + m0 + mm) * 1024);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mm = 0; mm < MB; ++mm)
#pragma unroll
                    for (int t = 0; t < TT; ++t)
                        out[t][m0 + mm] = mfma4(w[cb][mm][r], in[t][kq][r], out[t][m0 + mm]);
        }
    }
}

// v = σ.(v .+ b)  — bias after the product (Flux: W*x .+ b).  add_bias false:
// the bias is already the last term of the MFMA chain (folded first Dense).
template <int HT, int TT, bool RELU>
__device__ __forceinline__ void bias_act(const uint8_t* bb, int act, f32x4 (&v)[TT][HT], bool add_bias = true) {
    const int g = (threadIdx.x & 63) >> 4;
    if (add_bias) {
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const f32x4 b = lds4(bb + ((16 * m + 4 * g) << 2));
#pragma unroll
            for (int t = 0; t < TT; ++t) v[t][m] = v[t][m] + b;
        }
    }
    if (RELU || act == DF_ACT_RELU) {
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
            for (int m = 0; m < HT; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[t][m][r] = relu_fast(v[t][m][r]);
    } else if (act != DF_ACT_IDENTITY) {
        if (!RELU) {
#pragma unroll
            for (int t = 0; t < TT; ++t)
#pragma unroll
                for (int m = 0; m < HT; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[t][m][r] = impl::act_fn(act, v[t][m][r]);
        }
    }
}

// Final Dense, <= 4 outputs, as a VALU GEMV; every lane ends with all outputs.
// NO > 0: the output count is a compile-time constant (FAST variant).
template <int HT, int TT, bool RELU, int NO = 0>
__device__ __forceinline__ void out_valu(const uint8_t* buf, const UNet& N, const f32x4 (&h)[TT][HT],
                                         f32x4 (&o)[TT]) {
    const int g = (threadIdx.x & 63) >> 4;
    const uint8_t* w3 = buf + N.off_out;
    constexpr int INP = 16 * HT;
    const int n_out = NO > 0 ? NO : N.n_out;
    const float* b3 = reinterpret_cast<const float*>(w3) + n_out * INP;
#pragma unroll
    for (int t = 0; t < TT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oo = 0; oo < 4; ++oo) {
        if (oo < n_out) {
            float p[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) p[t] = 0.f;
#pragma unroll
            for (int kq = 0; kq < HT; ++kq) {
                const f32x4 w = lds4(w3 + ((oo * INP + 16 * kq + 4 * g) << 2));
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int t = 0; t < TT; ++t) p[t] = __builtin_fmaf(w[r], h[t][kq][r], p[t]);
            }
            const float bo = b3[oo];
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                const float v = xgroup_sum(p[t]) + bo;
                o[t][oo] = (RELU || N.act_out == DF_ACT_IDENTITY) ? v : impl::act_fn(N.act_out, v);
            }
        }
    }
}

// Final Dense, NO <= 4 outputs known at compile time (FAST variant), as a VALU
// GEMV whose lane-group reduction is a transpose: two v_permlane16_swap pair up
// outputs (0,1) and (2,3), one v_permlane32_swap completes them, so lane group g
// ends with output g — the transformed dim it updates — instead of every lane
// holding all outputs.  Sums associate as ((p0+p1)+(p2+p3)) over the groups,
// bitwise xgroup_sum's order; the bias is added after the product as in out_valu.
template <int HT, int TT, int NO>
__device__ __forceinline__ void out_valu_t(const uint8_t* buf, const UNet& N, const f32x4 (&h)[TT][HT],
                                           float (&y)[TT]) {
    static_assert(NO >= 1 && NO <= 4, "FAST tails: 1..4 outputs");
    const int g = (threadIdx.x & 63) >> 4;
    const uint8_t* w3 = buf + N.off_out;
    constexpr int INP = 16 * HT;
    float p[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int oo = 0; oo < 4; ++oo) p[t][oo] = 0.f;
#pragma unroll
    for (int oo = 0; oo < NO; ++oo)
#pragma unroll
        for (int kq = 0; kq < HT; ++kq) {
            const f32x4 w = lds4(w3 + ((oo * INP + 16 * kq + 4 * g) << 2));
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < TT; ++t) p[t][oo] = __builtin_fmaf(w[r], h[t][kq][r], p[t][oo]);
        }
    const float bo = reinterpret_cast<const float*>(w3)[NO * INP + (g < NO ? g : 0)];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[t][0]), __float_as_uint(p[t][1]), false, false);
        const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // rows: p0 g01, p1 g01, p0 g23, p1 g23
        float Bv = 0.f;
        if constexpr (NO > 2) {
            auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[t][2]), __float_as_uint(p[t][3]), false, false);
            Bv = __uint_as_float(b[0]) + __uint_as_float(b[1]);             // p2 g01, p3 g01, p2 g23, p3 g23
        }
        auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(Bv), false, false);
        y[t] = (__uint_as_float(c[0]) + __uint_as_float(c[1])) + bo;      // group g: output g
    }
}

// Lane group 0 gets (y_0 + y_1) + ... + y_{NO-1} of the per-group outputs (row order, RNVP.jl:180).
template <int NO>
__device__ __forceinline__ float group_row_sum(float y) {
    float s = y;
    if constexpr (NO > 1) {  // group 1 → group 0
        auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(y), __float_as_uint(y), false, false);
        s = s + __uint_as_float(a[1]);
    }
    if constexpr (NO > 2) {  // groups 2, 3 → groups 0, 1
        auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(y), __float_as_uint(y), false, false);
        const float y2 = __uint_as_float(b[1]);
        s = s + y2;
        if constexpr (NO > 3) {
            auto c = __builtin_amdgcn_permlane16_swap(__float_as_uint(y2), __float_as_uint(y2), false, false);
            s = s + __uint_as_float(c[1]);
        }
    }
    return s;
}

// Final Dense through MFMA (out <= 32): rows 16m + 4g + r in out[t][m].
template <int HT, int TT, bool RELU>
__device__ __forceinline__ void out_mfma(const uint8_t* buf, const UNet& N, const f32x4 (&h)[TT][HT],
                                         f32x4 (&out)[TT][2]) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const uint8_t* wb = buf + N.off_out + lane * 16;
    const int mt = (N.n_out + 15) >> 4;
#pragma unroll
    for (int t = 0; t < TT; ++t) out[t][0] = out[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kq = 0; kq < HT; ++kq) {
        const f32x4 w0 = lds4(wb + (kq * mt + 0) * 1024);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < TT; ++t) out[t][0] = mfma4(w0[r], h[t][kq][r], out[t][0]);
        if (mt > 1) {
            const f32x4 w1 = lds4(wb + (kq * mt + 1) * 1024);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < TT; ++t) out[t][1] = mfma4(w1[r], h[t][kq][r], out[t][1]);
        }
    }
    const uint8_t* bb = buf + N.off_out + HT * mt * 1024;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m < mt) {
            const f32x4 b = lds4(bb + ((16 * m + 4 * g) << 2));
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                f32x4 v = out[t][m] + b;
                if (!RELU && N.act_out != DF_ACT_IDENTITY)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = impl::act_fn(N.act_out, v[r]);
                out[t][m] = v;
            }
        }
    }
}

template <int PH>
__device__ __forceinline__ float couple1(float v, float y) {
    if (PH == impl::PH_S_FWD) return v * expf(y);
    if (PH == impl::PH_T_FWD) return v + y;
    if (PH == impl::PH_T_BWD) return v - y;
    return v * expf(-y);  // PH_S_BWD
}

// Output Dense + coupling phase of net N on the last hidden activations H.
// NO > 0: n_out = n_af = NO at compile time (FAST variant, OUTV only).
template <int HT, int TT, bool OUTV, bool RELU, int PH, int NO = 0>
__device__ __forceinline__ void tail(const uint8_t* buf, const UNet& N, const ULayer& L, const int32_t* tab,
                                     float* state, const int (&ro)[TT], float (&sum)[TT], const f32x4 (&H)[TT][HT]) {
    const int g = (threadIdx.x & 63) >> 4;
    constexpr bool SPH = (PH == impl::PH_S_FWD || PH == impl::PH_S_BWD);
    const int32_t* af = tab + L.af_tab;
    const int n_af = (OUTV && NO > 0) ? NO : L.n_af;
#pragma unroll
    for (int t = 0; t < TT; ++t) sum[t] = 0.f;
#ifdef DF_EXP_NOTAIL  // diagnostic build only: no output Dense / coupling (results are wrong)
    if (true) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < HT; ++m) acc += H[t][m][0];
            asm volatile("" ::"v"(acc));
        }
        return;
    }
#endif
    if constexpr (OUTV && NO > 0) {
        float y[TT];
        out_valu_t<HT, TT, NO>(buf, N, H, y);
        const int slot = af[g < NO ? g : 0];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (g < NO) state[ro[t] + slot] = couple1<PH>(state[ro[t] + slot], y[t]);
            if (SPH) sum[t] = group_row_sum<NO>(y[t]);  // valid in lane group 0 (ldj_update)
        }
    } else if constexpr (OUTV) {
        f32x4 o[TT];
        out_valu<HT, TT, RELU, NO>(buf, N, H, o);
        const int slot = (g < n_af) ? af[g] : 0;
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const float y = impl::sel4(o[t], g);
            if (g < n_af) state[ro[t] + slot] = couple1<PH>(state[ro[t] + slot], y);
            if (SPH) {
                // ldj = Σ_k s[k] in row order (RNVP.jl:180 / :86)
                float s_ = o[t][0];
#pragma unroll
                for (int oo = 1; oo < 4; ++oo)
                    if (oo < n_af) s_ = s_ + o[t][oo];
                sum[t] = s_;
            }
        }
    } else {
        f32x4 o[TT][2];
        out_mfma<HT, TT, RELU>(buf, N, H, o);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            float p = 0.f;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int oo = 16 * m + 4 * g + r;
                    if (oo < L.n_af) {
                        const int slot = af[oo];
                        const float y = o[t][m][r];
                        state[ro[t] + slot] = couple1<PH>(state[ro[t] + slot], y);
                        if (SPH) p = p + y;
                    }
                }
            if (SPH) sum[t] = xgroup_sum(p);
        }
    }
}

// ---- SPLIT variant: f32 GEMMs on bf16 MFMA (v_mfma_f32_16x16x32_bf16) ----
// Both operands are split in three bf16 planes, a = a0 + a1 + a2 exactly (RNE
// remainders, 8+8+8 significand bits; weights by the planner, activations here
// by v_cvt_pk_bf16_f32), and W·x is accumulated in f32 from the six products
// w0x0 + w0x1 + w1x0 + w0x2 + w1x1 + w2x0.  The dropped terms are below 2^-26
// of |w·x| and every product is exact, so the sums carry f32-level error
// (≈ Σ|w·x|·2^-24, like the exact-f32 MFMA chain) at 16/6 of its MFMA rate.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma_bf(const bf16x8& a, const bf16x8& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Remainder x - (float)h[S] of an RNE bf16 pair h, as one v_dot2c_f32_bf16
// (x + h·(-1, 0) or x + h·(0, -1)): the difference is exactly representable, and the
// dot2 returns it bitwise (tools/probe/dot2_split.hip), so the two bf16 → f32 unpacks
// and the f32 subtract of the plain form become one instruction per value.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#ifndef DF_SPLIT_DOT2
#define DF_SPLIT_DOT2 1
#endif
template <int S>
__device__ __forceinline__ float split_rem(bf16x2 h, float x) {
#if DF_SPLIT_DOT2 == 2
    // plain VALU: hi unpacked by a shift (low half) or a mask (high half), then one
    // v_sub_f32 (asm: -O3 would pair two of them into v_pk_add_f32).  Beside MFMAs a
    // v_dot2c_f32_bf16 or a packed f32 op waits for the matrix pipe (≈ 16 cycles each,
    // tools/probe/mfma_valu.hip); shifts, masks and subtracts co-issue.
    const uint32_t u = __builtin_bit_cast(uint32_t, h);
    const float hi = __uint_as_float(S == 0 ? (u << 16) : (u & 0xffff0000u));
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(hi));
    return r;
#elif DF_SPLIT_DOT2
    // (-1, 0) is materialised by a v_mov: the compiler would otherwise encode it as the
    // inline constant -1.0, which the hardware reads as the f32 0xbf800000, i.e. (0, -1)
    // (probe: tools/probe/dot2_split.hip).  The asm is pure, so it is hoisted and shared.
    uint32_t c;
    if (S == 0) asm("v_mov_b32 %0, 0xbf80" : "=v"(c));
    else c = 0xbf800000u;
    return __builtin_amdgcn_fdot2_f32_bf16(h, __builtin_bit_cast(bf16x2, c), x, false);
#else
    return x - (float)h[S];
#endif
}

// 2 f32 values → their three bf16 planes (pairs).
__device__ __forceinline__ void split2(float a, float b, bf16x2& p0, bf16x2& p1, bf16x2& p2) {
    p0 = bf16x2{(__bf16)a, (__bf16)b};
    const float ra = split_rem<0>(p0, a), rb = split_rem<1>(p0, b);
    p1 = bf16x2{(__bf16)ra, (__bf16)rb};
    p2 = bf16x2{(__bf16)split_rem<0>(p1, ra), (__bf16)split_rem<1>(p1, rb)};
}

// 8 f32 values → their three bf16 planes.
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        bf16x2 h, m, l;
        split2(v[e], v[e + 1], h, m, l);
        p0[e] = h[0]; p0[e + 1] = h[1];
        p1[e] = m[0]; p1[e + 1] = m[1];
        p2[e] = l[0]; p2[e + 1] = l[1];
    }
}

// Remainders on the matrix pipe (DF_SPLIT_MREM): for one accumulator tile c (lane
// (g, j): rows 4g + r of sample j) and its RNE bf16 plane h (the same four values),
// v_mfma_f32_4x4x4_16b_bf16 with A = −I in each of its 16 independent 4×4 blocks and
// C = c gives c − h: the only non-zero product is −h, exact, and C + one product
// rounds once — to the exact difference (representable: h is c rounded to 8
// significant bits).  Bitwise the dot2 remainder, one matrix instruction per 256
// values instead of 256 lanes' v_dot2c_f32_bf16 (which cost ≈ 8–10 issue cycles each
// beside the MFMAs), and 2 matrix-pipe passes where the 16-wide contraction
// (v_mfma_f32_16x16x16_bf16, A = −I) took 4: 8.6 against 16.1 cycles alone, 15.5
// against 22.7 beside a product MFMA (tools/probe/mfma_rem.hip).  The subtraction
// is lane-local: lane l holds row l%4 of its block's A, column l%4 of B (its four
// bf16) and column l%4 of C/D (its four f32), so with A's row l%4 = −1 at element
// l%4 and 0 elsewhere D[e] = C[e] − B[e] in the lane's own registers, whichever
// accumulator layout the tile is in.  (A non-finite value turns 0·inf into NaN for
// its own lane's four values only — four rows of the same sample, whose outputs are
// non-finite anyway.)
#ifndef DF_SPLIT_MREM
#define DF_SPLIT_MREM 1
#endif
typedef short short4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ short4v neg_eye() {
    const int i = threadIdx.x & 3;
    short4v p;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = (e == i) ? (short)0xbf80 : (short)0;
    return p;
}

__device__ __forceinline__ f32x4 mrem(short4v eye, bf16x4v h, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(eye, __builtin_bit_cast(short4v, h), c, 0, 0, 0);
}

// planes of two accumulator tiles (8 values: a then b), remainders on the matrix pipe
__device__ __forceinline__ void split8_mrem(short4v eye, const f32x4& a, const f32x4& b, bf16x8& p0, bf16x8& p1,
                                            bf16x8& p2) {
    bf16x4v h0, h1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h0[e] = (__bf16)a[e];
        h1[e] = (__bf16)b[e];
    }
    p0 = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    const f32x4 ra = mrem(eye, h0, a), rb = mrem(eye, h1, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h0[e] = (__bf16)ra[e];
        h1[e] = (__bf16)rb[e];
    }
    p1 = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    const f32x4 sa = mrem(eye, h0, ra), sb = mrem(eye, h1, rb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h0[e] = (__bf16)sa[e];
        h1[e] = (__bf16)sb[e];
    }
    p2 = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// First Dense of a FAST net (one k-step, bias folded in slot g = 3): lane group g
// carries feature g's planes in the product slots (x0, x1, x0, x2, x1, x0, 0, 0)
// against the planner's (w0, w0, w1, w0, w1, w2, 0, 0): one MFMA per m-tile.
template <int HT, int TT>
__device__ __forceinline__ void dense_first_split(const uint8_t* buf, const UNet& N, const float (&xin)[TT][4],
                                                  f32x4 (&acc)[TT][HT]) {
    const int lane = threadIdx.x & 63;
    bf16x8 b[TT];
    const __bf16 z = (__bf16)0.f;
#pragma unroll
    for (int t = 0; t < TT; t += 2) {  // tiles in pairs: one split of two values
        bf16x2 h, m, l;
        split2(xin[t][0], t + 1 < TT ? xin[t + 1][0] : 0.f, h, m, l);
        b[t] = bf16x8{h[0], m[0], h[0], l[0], m[0], h[0], z, z};
        if (t + 1 < TT) b[t + 1] = bf16x8{h[1], m[1], h[1], l[1], m[1], h[1], z, z};
    }
    const uint8_t* wb = buf + N.off_w0 + lane * 16;
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        const bf16x8 w = *reinterpret_cast<const bf16x8*>(wb + m * 1024);
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t][m] = mfma_bf(w, b[t], f32x4{0.f, 0.f, 0.f, 0.f});
    }
}

// Hidden H×H Dense: k-chunk c of 32 inputs = accumulator tiles 2c, 2c+1 (lane
// (g, j): rows 32c + 16(e>>2) + 4g + (e&3) of sample j), split on the fly.
// The accumulators start from the bias (b + W·x: the sum's rounding order differs
// from Flux's W*x .+ b by one f32 rounding, like any other summation order).
// BIAS false (the training kernel's W1ᵀδ): the chains start from zero.
template <int HT, int TT, bool BIAS = true, bool FENCE = false>
__device__ __forceinline__ void dense_hidden_split(const uint8_t* wb, const f32x4 (&in)[TT][HT],
                                                   f32x4 (&out)[TT][HT]) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const uint8_t* bb = wb + (HT / 2) * HT * 3072;
    wb += lane * 16;
    const short4v eye = DF_SPLIT_MREM ? neg_eye() : short4v{0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < HT; ++m) {
        const f32x4 b = BIAS ? lds4(bb + ((16 * m + 4 * g) << 2)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TT; ++t) out[t][m] = b;
    }
#pragma unroll
    for (int c = 0; c < HT / 2; ++c) {
        bf16x8 x[TT][3];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const float v[8] = {in[t][2 * c][0],     in[t][2 * c][1],     in[t][2 * c][2],     in[t][2 * c][3],
                                in[t][2 * c + 1][0], in[t][2 * c + 1][1], in[t][2 * c + 1][2], in[t][2 * c + 1][3]};
#ifdef DF_DIAG_NOSPLIT  // diagnostic build: hi plane only, repeated (results are wrong)
            for (int e = 0; e < 8; ++e) x[t][0][e] = (__bf16)v[e];
            x[t][1] = x[t][0];
            x[t][2] = x[t][0];
#else
            if constexpr (DF_SPLIT_MREM) split8_mrem(eye, in[t][2 * c], in[t][2 * c + 1], x[t][0], x[t][1], x[t][2]);
            else split8(v, x[t][0], x[t][1], x[t][2]);
#endif
        }
#pragma unroll
        for (int m = 0; m < HT; ++m) {
            const uint8_t* f = wb + (c * HT + m) * 3072;
            const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(f);
            const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(f + 1024);
            const bf16x8 w2 = *reinterpret_cast<const bf16x8*>(f + 2048);
#pragma unroll
            for (int t = 0; t < TT; ++t) {  // small terms first
                f32x4 a = out[t][m];
                a = mfma_bf(w2, x[t][0], a);
                a = mfma_bf(w1, x[t][1], a);
                a = mfma_bf(w0, x[t][2], a);
                a = mfma_bf(w1, x[t][0], a);
                a = mfma_bf(w0, x[t][1], a);
                out[t][m] = mfma_bf(w0, x[t][0], a);
            }
            if (FENCE) asm volatile("" ::: "memory");  // fragment reads not hoisted past this m-tile
        }
    }
}

// ---- SPLIT variant, LDS reads ahead of their use (DF_SPLIT_PREFETCH) ----
// The straight form above reads every fragment right before the MFMAs that take it, so
// a wave stands in s_waitcnt lgkmcnt(0) for one LDS round trip per m-tile, per first-
// Dense fragment and per output-weight vector: a third of its life
// (profiles/prefetch_isa_waits.txt).  Here every read is requested one step ahead: the
// step's own matrix (or fma) work runs between a request and its wait.  Arithmetic,
// operand order and roundings are those of the straight form: bitwise the same outputs.
//
// The waits cannot be counted ones (lgkmcnt(n) leaving the newest n requests in flight):
// while a stage DMA (global_load_lds) is outstanding, which is the whole net, the
// compiler retires every LDS read with lgkmcnt(0).  So a step waits for its own reads
// FIRST (lds_wait0, written out: the compiler adds no wait of its own after it) and only
// then requests the next step's.  The order is pinned with scheduling barriers; left
// alone the scheduler sinks the reads back to their uses, or spreads them until the
// instance spills.
#ifndef DF_SPLIT_PREFETCH
#define DF_SPLIT_PREFETCH 1
#endif

__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

// s_waitcnt lgkmcnt(0) alone (vmcnt 63, expcnt 7: the stage DMA is not waited for)
__device__ __forceinline__ void lds_wait0() { __builtin_amdgcn_s_waitcnt(0xc07f); }

// What one (chunk c, m-tile m) step of the hidden Dense reads: the three weight planes
// and, in chunk 0, the m-tile's bias (the start of its accumulator chains).
struct SplitStep {
    bf16x8 w0, w1, w2;
    f32x4 b;
};

// wl = the Dense's fragments + lane * 16, bl = its bias + 16 g; steps are contiguous
// (step s = c·HT + m at s·3072).  A step past the Dense requests nothing.
template <int HT, bool BIAS>
__device__ __forceinline__ void split_step_request(const uint8_t* wl, const uint8_t* bl, int s, SplitStep& f) {
    if (s >= (HT / 2) * HT) return;
    const uint8_t* p = wl + s * 3072;
    f.w0 = *reinterpret_cast<const bf16x8*>(p);
    f.w1 = *reinterpret_cast<const bf16x8*>(p + 1024);
    f.w2 = *reinterpret_cast<const bf16x8*>(p + 2048);
    if (BIAS && s < HT) f.b = lds4(bl + (s << 6));
}

// dense_hidden_split with the (c, m) nest as one sequence of HT/2 × HT steps on two
// fragment sets: a step retires its own fragments (requested before the previous step's
// MFMAs), requests the next step's and issues its 6·TT MFMAs.  The request of a chunk's
// first step so precedes that chunk's activation split.  f0 = step 0, requested by the
// caller.
template <int HT, int TT, bool BIAS = true>
__device__ __forceinline__ void dense_hidden_split_pf(const uint8_t* wb, int l16, int g16, const f32x4 (&in)[TT][HT],
                                                      f32x4 (&out)[TT][HT], const SplitStep& f0) {
    const uint8_t* bl = wb + (HT / 2) * HT * 3072 + g16;
    const uint8_t* wl = wb + l16;
    const short4v eye = neg_eye();
    SplitStep f[2];
    f[0] = f0;
    bf16x8 x[TT][3];
#pragma unroll
    for (int s = 0; s < (HT / 2) * HT; ++s) {
        const int c = s / HT, m = s % HT;
        if (m == 0) {
#pragma unroll
            for (int t = 0; t < TT; ++t) split8_mrem(eye, in[t][2 * c], in[t][2 * c + 1], x[t][0], x[t][1], x[t][2]);
        }
        // the last step of a chunk is the register peak (its planes, all accumulators and
        // the next chunk's f32 tiles): the next chunk's first request follows its MFMAs,
        // where the planes are dead, and the activation split covers it
        constexpr int NS = (HT / 2) * HT;
        const bool late = (m == HT - 1) && (s + 1 < NS);
        sched_fence();
        lds_wait0();
        if (!late) split_step_request<HT, BIAS>(wl, bl, s + 1, f[(s + 1) & 1]);
        sched_fence();
        const SplitStep& w = f[s & 1];
#pragma unroll
        for (int t = 0; t < TT; ++t) {  // small terms first
            f32x4 a = c == 0 ? (BIAS ? w.b : f32x4{0.f, 0.f, 0.f, 0.f}) : out[t][m];
            a = mfma_bf(w.w2, x[t][0], a);
            a = mfma_bf(w.w1, x[t][1], a);
            a = mfma_bf(w.w0, x[t][2], a);
            a = mfma_bf(w.w1, x[t][0], a);
            a = mfma_bf(w.w0, x[t][1], a);
            out[t][m] = mfma_bf(w.w0, x[t][0], a);
        }
        if (late) {
#pragma unroll
            for (int t = 0; t < TT; ++t) asm volatile("" : "+v"(out[t][m]));  // the MFMAs stay above the request
            sched_fence();
            split_step_request<HT, BIAS>(wl, bl, s + 1, f[(s + 1) & 1]);
        }
    }
}

// dense_first_split on fragments w[HT] the caller requested ahead of the feature reads:
// HT × TT MFMAs back to back.
template <int HT, int TT>
__device__ __forceinline__ void dense_first_split_pf(const bf16x8 (&w)[HT], const float (&xin)[TT][4],
                                                     f32x4 (&acc)[TT][HT]) {
    bf16x8 b[TT];
    const __bf16 z = (__bf16)0.f;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        // one value per tile, split on its own: each plane is the low half of its
        // conversion, so a remainder takes a shift and a subtract (a pair of two tiles'
        // values needs a mask for the high half as well); the planes are split2's
        // The second remainder takes m from the operand's own word (m, h), whose low half
        // it is: r1 is converted once, with that word.
        const bf16x2 h = bf16x2{(__bf16)xin[t][0], z};
        const float r1 = split_rem<0>(h, xin[t][0]);
        // (the word is made opaque: left alone the compiler converts r1 a second time, with a
        // zero, for the remainder)
        uint32_t w = __builtin_bit_cast(uint32_t, bf16x2{(__bf16)r1, (__bf16)xin[t][0]});
        asm("" : "+v"(w));
        const bf16x2 mh = __builtin_bit_cast(bf16x2, w);
        const __bf16 l = (__bf16)split_rem<0>(mh, r1);
        b[t] = bf16x8{(__bf16)xin[t][0], (__bf16)r1, (__bf16)xin[t][0], l, mh[0], mh[1], z, z};
    }
#pragma unroll
    for (int m = 0; m < HT; ++m)
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t][m] = mfma_bf(w[m], b[t], f32x4{0.f, 0.f, 0.f, 0.f});
}

// The HT weight vectors of output oo (w3g = the output Dense + 16 g); nothing past NO.
template <int HT, int NO>
__device__ __forceinline__ void out_row_request(const uint8_t* w3g, int oo, f32x4 (&w)[HT]) {
    if (oo >= NO) return;
#pragma unroll
    for (int kq = 0; kq < HT; ++kq) w[kq] = lds4(w3g + ((oo * 16 * HT + 16 * kq) << 2));
}

// What a lane group owns after the tail's transposed reduction.  A reduction tree has four
// slots, one per lane group.  The pair form (split_tail_pair) fills every tree with BOTH
// tiles' outputs of a group of two tiles; every lane takes part in the couplings (copies
// compute and store the same bits to the same words), and ONE ldj update serves both rows:
//   NO = 1: one tree, lane group g owns the output of tile g & 1 (groups 2, 3: copies);
//   NO = 2: one tree, lane group g owns output g & 1 of tile g >> 1;
//   NO = 3: two trees: in the first lane group g owns output g & 1 of tile g >> 1, in the
//           second output 2 of tile g & 1 (groups 2, 3: copies), so a lane group's two
//           values may lie in two tiles; Σ s of tile 0 ends in lane group 0, of tile 1 in
//           lane group 3, which update the ldj words of their first tree's tile;
//   NO = 4: two trees, lane group g owns outputs g & 1 and 2 + (g & 1) of tile g >> 1.
// Otherwise every tile has its own tree and lane group g owns output g of each of the TT
// tiles (TT rows, one value per row; groups g >= NO are masked, lane group 0 updates ldj).
// Three and four outputs take the pair form where the lane group's offsets are values held
// across the bodies (WIDE = LANES of net_tiles): derived in every body, the second tree's
// words and columns cost more than the form saves.
constexpr bool split_tail_pair(int TT, int NO, bool WIDE) { return TT == 2 && (NO <= 2 || WIDE); }
// The values a lane group owns and its row offsets: in the pair form the one of the group's
// first tile, and the tile a value lies in is part of the value's column (SplitTail).
constexpr int split_tail_vals(int TT, int NO, bool WIDE) { return split_tail_pair(TT, NO, WIDE) ? (NO + 1) / 2 : TT; }
constexpr int split_tail_rows(int TT, int NO, bool WIDE) { return split_tail_pair(TT, NO, WIDE) ? 1 : TT; }

// One tree on the slots (a0, a1, b0, b1): lane groups 0..3 get the sums of a0, a1, b0, b1
// over the four lane groups, each associated ((p_g0 + p_g1) + (p_g2 + p_g3)).
__device__ __forceinline__ float pair_tree(float a0, float a1, float b0, float b1) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(a0), __float_as_uint(a1), false, false);
    const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // a0 g01, a1 g01, a0 g23, a1 g23
    auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(b0), __float_as_uint(b1), false, false);
    const float Bv = __uint_as_float(b[0]) + __uint_as_float(b[1]);  // b0 g01, b1 g01, b0 g23, b1 g23
    auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(Bv), false, false);
    return __uint_as_float(c[0]) + __uint_as_float(c[1]);
}

// What a read-ahead SPLIT body and the ldj update behind it (uniform_kernel's tiles_loop)
// share: ce, the state column of ldj_elem (ldj_chain is the column before it), goes in;
// per owned row u the row's offset and its two ldj words as they stood before the body
// (requested with the coupling's old values, so no round trip of their own) come out.
// l16, g16: the lane's two offsets into fragments and vectors, lane · 16 and (lane >> 4) · 16,
// from the kernel where the instance has the registers to hold them across bodies (LANES
// of net_tiles); otherwise the body derives them from an opaque copy of the thread id.
// ts, the offset from a tile's rows to the next tile's, goes in as well; lcol comes out: ce,
// in the pair form plus ts where the lane group's ldj words are the second tile's.
template <int TT>
struct SplitTail {
    int ce, ts, l16, g16;
    int lcol;
    int row[TT];
    float e_old[TT], a_old[TT];
};

// out_valu_t on two sets of weight vectors: output 0's (w0, with the bias bo and the
// coupling's slot word) were requested by the caller before the second relu; output
// oo + 1's are requested ahead of output oo's 4·HT·TT fma, the coupling's old state
// values (state[row + aslot[u]] -> v[u]) and, LDJ, the rows' ldj words (tl) with output 1's.
// fma order (oo, kq, r) as in out_valu_t; the swap reduction as in out_valu_t per tile, or
// trees that hold both tiles (split_tail_vals): every sum still associates
// ((p_g0 + p_g1) + (p_g2 + p_g3)), as outputs 2, 3 of a four-output net do in their slots.
// bo[u], aslot[u]: the bias and the state column of the u-th output the lane group owns.
template <int HT, int TT, int NO, bool LDJ, bool WIDE, int NU>
__device__ __forceinline__ void out_valu_t_pf(const uint8_t* w3g, const f32x4 (&w0)[HT], const float (&bo)[NU],
                                              const f32x4 (&h)[TT][HT], const float* state, const int (&aslot)[NU],
                                              SplitTail<TT>& tl, float (&v)[NU], float (&y)[NU]) {
    static_assert(NO >= 1 && NO <= 4, "FAST tails: 1..4 outputs");
    static_assert(NU == split_tail_vals(TT, NO, WIDE), "outputs a lane group owns");
    constexpr bool PAIR = split_tail_pair(TT, NO, WIDE);
    constexpr int NR = split_tail_rows(TT, NO, WIDE);
    float p[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int oo = 0; oo < 4; ++oo) p[t][oo] = 0.f;
    f32x4 w[2][HT];
#pragma unroll
    for (int kq = 0; kq < HT; ++kq) w[0][kq] = w0[kq];
#pragma unroll
    for (int oo = 0; oo < NO; ++oo) {
        sched_fence();
        lds_wait0();
        if (oo == 0) {
#pragma unroll
            for (int u = 0; u < NU; ++u) v[u] = state[tl.row[NR == 1 ? 0 : u] + aslot[u]];
            if constexpr (LDJ) {  // a word whose value the update does not use is read for nothing
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    tl.e_old[r] = state[tl.row[r] + tl.lcol];
                    tl.a_old[r] = state[tl.row[r] + tl.lcol - 1];
                }
            }
        }
        out_row_request<HT, NO>(w3g, oo + 1, w[(oo + 1) & 1]);
        sched_fence();
#pragma unroll
        for (int kq = 0; kq < HT; ++kq)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < TT; ++t) p[t][oo] = __builtin_fmaf(w[oo & 1][kq][r], h[t][kq][r], p[t][oo]);
        // the fma are pure: without a use tied to the fences they sink below the next request
#pragma unroll
        for (int t = 0; t < TT; ++t) asm volatile("" : "+v"(p[t][oo]));
    }
    if constexpr (PAIR && NO >= 3) {  // two trees, both tiles in each (split_tail_pair)
        y[0] = pair_tree(p[0][0], p[0][1], p[1][0], p[1][1]) + bo[0];  // output g & 1 of tile g >> 1
        if constexpr (NO == 4) {
            y[1] = pair_tree(p[0][2], p[0][3], p[1][2], p[1][3]) + bo[1];  // output 2 + (g & 1) of tile g >> 1
        } else {  // output 2 of both tiles through one swap, as the one-output tree
            auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[0][2]), __float_as_uint(p[1][2]), false, false);
            const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // t0 g01, t1 g01, t0 g23, t1 g23
            auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(A), false, false);
            y[1] = (__uint_as_float(c[0]) + __uint_as_float(c[1])) + bo[1];  // output 2 of tile g & 1
        }
    } else if constexpr (PAIR) {  // one tree: the slots hold both tiles
        const float q = NO == 2 ? p[0][1] : p[1][0];
        auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[0][0]), __float_as_uint(q), false, false);
        const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // NO = 2, tile 0: p0 g01, p1 g01, p0 g23, p1 g23
        float Bv = A;                                                     // NO = 1: t0 g01, t1 g01, t0 g23, t1 g23
        if constexpr (NO == 2) {
            auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[1][0]), __float_as_uint(p[1][1]), false, false);
            Bv = __uint_as_float(b[0]) + __uint_as_float(b[1]);           // tile 1: p0 g01, p1 g01, p0 g23, p1 g23
        }
        auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(Bv), false, false);
        y[0] = (__uint_as_float(c[0]) + __uint_as_float(c[1])) + bo[0];   // split_tail_vals: the group's (tile, output)
    } else {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[t][0]), __float_as_uint(p[t][1]), false, false);
            const float A = __uint_as_float(a[0]) + __uint_as_float(a[1]);  // rows: p0 g01, p1 g01, p0 g23, p1 g23
            float Bv = 0.f;
            if constexpr (NO > 2) {
                auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(p[t][2]), __float_as_uint(p[t][3]), false, false);
                Bv = __uint_as_float(b[0]) + __uint_as_float(b[1]);             // p2 g01, p3 g01, p2 g23, p3 g23
            }
            auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(Bv), false, false);
            y[t] = (__uint_as_float(c[0]) + __uint_as_float(c[1])) + bo[t];   // group g: output g
        }
    }
}

// What a net body of the read-ahead SPLIT path takes from the descriptors, as values the
// kernel loads once per net into scalar registers (run_net), outside the tile-group loop:
// the net's start in its stage and the layer's two slot words (df_plan.h).
struct SplitHead {
    int off_w0, feat_word, af_word;
};
// the read-ahead SPLIT path of net_tiles (diagnostic builds keep the straight form)
#if DF_SPLIT_PREFETCH && !defined(DF_EXP_NOTAIL) && !defined(DF_DIAG_NOSPLIT)
#define DF_SPLIT_HEAD_REGS 1
#else
#define DF_SPLIT_HEAD_REGS 0
#endif

// Wave priority by phase of a read-ahead SPLIT body (DF_SPLIT_PRIO): 1, the default,
// raises a wave (s_setprio 2) from the first product MFMA of its first Dense to the last
// MFMA of its hidden Dense and drops it to 0 for the rest — the VALU tail (second relu,
// output GEMV, coupling), the ldj update, the next head's request and any stage switch —
// so that a wave with matrix work issues first and a wave in its tail takes the gaps
// between another wave's MFMAs: 1.329 -> 1.246 M cycles per config-2 launch.  2 is the
// opposite assignment, the control (1.380); 0 sets no priority.  Levels 1 and 3 measure as
// 2 does.  (profiles/head_ab.txt.)
#ifndef DF_SPLIT_PRIO
#define DF_SPLIT_PRIO 1
#endif
template <bool MATRIX_PHASE>
__device__ __forceinline__ void split_prio() {
    if constexpr (DF_SPLIT_PRIO == 1) __builtin_amdgcn_s_setprio(MATRIX_PHASE ? 2 : 0);
    if constexpr (DF_SPLIT_PRIO == 2) __builtin_amdgcn_s_setprio(MATRIX_PHASE ? 0 : 2);
}

// Evaluate net N for TT 16-sample tiles (state rows ro[t]) and apply its
// coupling phase; sum[t] = Σ_k s_k for s phases (row order).
// hd: the read-ahead SPLIT path's scalar words (SplitHead); unused by every other path.
// tl, LDJ: that path's tail (SplitTail); there sum[u] belongs to row tl.row[u],
// u < split_tail_rows(TT, NO, LANES), at column tl.lcol, and LDJ asks an s phase for the
// rows' ldj words.
template <int HT, int TT, bool OUTV, bool RELU, int PH, bool FAST = false, int NO = 0, bool SPLIT = false,
          bool LDJ = false, bool LANES = false>
__device__ __forceinline__ void net_tiles(const uint8_t* buf, const UNet& N, const ULayer& L, const int32_t* tab,
                                          float* state, const int (&ro)[TT], float (&sum)[TT], const SplitHead& hd,
                                          SplitTail<TT>& tl) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    constexpr bool SPH = (PH == impl::PH_S_FWD || PH == impl::PH_S_BWD);
#if DF_SPLIT_HEAD_REGS
    if constexpr (SPLIT && FAST && HT >= 2 && OUTV && NO > 0) {
        // The head is ONE request: the first-Dense fragments, the features and step 0 of
        // the hidden Dense, then one wait, then the first-Dense split and its MFMAs.
        // Nothing of it depends on a load: the net's start in the stage and the layer's
        // two slot words (df_plan.h) are scalar registers the caller loaded once per net,
        // the hidden and the output Dense follow from the start (kSplitOffH /
        // kSplitOffOut), and a lane group takes its slots from the words by a bit-field
        // extract.  (With the table word in LDS and every offset a scalar load at its use,
        // a body made five dependent round trips before its first MFMA:
        // profiles/head_isa_waits.txt.)
        // l16 and g16 from an opaque copy of the thread id: derived here they die with the
        // body; derived once per kernel (LANES) they are two VGPRs held across all bodies,
        // which the logpdf instances (past 120 of 128 VGPRs) do not have
        int l16 = tl.l16, g16 = tl.g16;
        if constexpr (!LANES) {
            int tx = threadIdx.x;
            asm volatile("" : "+v"(tx));
            l16 = (tx & 63) << 4, g16 = tx & 48;
        }
        const int g = g16 >> 4;
        const uint8_t* net = buf + hd.off_w0;
        const int slot = ((uint32_t)hd.feat_word >> (g16 >> 1)) & ((1 << kSplitSlotBits) - 1);
        static_assert(kSplitSlotBits == 8, "slot of lane group g at bit 8 g = g16 / 2");
        bf16x8 w0[HT];
#pragma unroll
        for (int m = 0; m < HT; ++m) w0[m] = *reinterpret_cast<const bf16x8*>(net + l16 + m * 1024);
        float xin[TT][4];
#pragma unroll
        for (int t = 0; t < TT; ++t) xin[t][0] = state[ro[t] + slot];
        const uint8_t* wh = net + kSplitOffH(HT);
        SplitStep f0;
        split_step_request<HT, true>(wh + l16, wh + (HT / 2) * HT * 3072 + g16, 0, f0);
        sched_fence();
        lds_wait0();
        split_prio<true>();
        sched_fence();
        f32x4 A[TT][HT], B[TT][HT];
        dense_first_split_pf<HT, TT>(w0, xin, A);
        bias_act<HT, TT, true>(buf, DF_ACT_RELU, A, false);
        dense_hidden_split_pf<HT, TT>(wh, l16, g16, A, B, f0);
        // tail: the first output's weights and the bias before the second relu
        const uint8_t* w3 = net + kSplitOffOut(HT);
        const uint8_t* w3g = w3 + g16;
        sched_fence();
        split_prio<false>();
        f32x4 wo[HT];
        out_row_request<HT, NO>(w3g, 0, wo);
        // the row and the outputs this lane group owns after the reduction (split_tail_vals)
        constexpr int NU = split_tail_vals(TT, NO, LANES);
        constexpr int NR = split_tail_rows(TT, NO, LANES);
        constexpr bool PAIR = split_tail_pair(TT, NO, LANES);
        const float* bias = reinterpret_cast<const float*>(w3) + NO * 16 * HT;
        float bo[NU];
        int aslot[NU];
        tl.lcol = tl.ce;
        if constexpr (PAIR) {
            // The lane group's tile as an offset (the tile step or 0) that goes into its
            // columns, not into the row: column and offset are values of the lane group and
            // the net alone, so their sum leaves the tile-group loop where the lane group's
            // offsets are held across the bodies.  (Not a choice between ro[0] and ro[1]
            // either: that is an indexed read of ro, which then lives in scratch.)
            const int go = NO == 1 ? 0 : (g & 1);
            const int t0 = (NO == 1 ? (g & 1) : (g >> 1)) ? tl.ts : 0;
            bo[0] = bias[go];
            aslot[0] = (((uint32_t)hd.af_word >> (kSplitSlotBits * go)) & ((1 << kSplitSlotBits) - 1)) + t0;
            tl.lcol = tl.ce + t0;
            if constexpr (NO == 3) {  // output 2, of tile g & 1: a uniform word and column
                bo[1] = bias[2];
                aslot[1] = (((uint32_t)hd.af_word >> (kSplitSlotBits * 2)) & ((1 << kSplitSlotBits) - 1)) +
                           (go ? tl.ts : 0);
            } else if constexpr (NO == 4) {
                bo[1] = bias[go + 2];
                aslot[1] = (((uint32_t)hd.af_word >> (kSplitSlotBits * (go + 2))) & ((1 << kSplitSlotBits) - 1)) + t0;
            }
            tl.row[0] = ro[0];
        } else {
            const int go = g < NO ? g : 0;
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                bo[t] = bias[go];
                aslot[t] = ((uint32_t)hd.af_word >> (kSplitSlotBits * go)) & ((1 << kSplitSlotBits) - 1);
                tl.row[t] = ro[t];
            }
        }
        sched_fence();
        bias_act<HT, TT, true>(buf, DF_ACT_RELU, B, false);
        float v[NU], y[NU];
        out_valu_t_pf<HT, TT, NO, SPH && LDJ, LANES>(w3g, wo, bo, B, state, aslot, tl, v, y);
        // one region for the lane groups that own an output (all of them when the trees hold
        // both tiles), so that the couplings interleave
        if (PAIR || g < NO) {
#pragma unroll
            for (int u = 0; u < NU; ++u) state[tl.row[NR == 1 ? 0 : u] + aslot[u]] = couple1<PH>(v[u], y[u]);
        }
        if constexpr (!SPH) {
#pragma unroll
            for (int t = 0; t < TT; ++t) sum[t] = 0.f;
        } else if constexpr (PAIR && NO == 1) {
            sum[0] = y[0];
        } else if constexpr (PAIR) {
            // Σ s of the group's tile in group_row_sum's order, ((y_0 + y_1) + y_2) + y_3: the
            // swap of a tree with itself gives every lane group both outputs of its tile, so
            // with two and four outputs all four lane groups hold their row's sum and the ldj
            // update needs no mask; with three, y_2 is the tile's own in lane groups 0 and 3
            auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(y[0]), __float_as_uint(y[0]), false, false);
            float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
            if constexpr (NO == 3) s = s + y[1];
            if constexpr (NO == 4) {
                auto c = __builtin_amdgcn_permlane16_swap(__float_as_uint(y[1]), __float_as_uint(y[1]), false, false);
                s = (s + __uint_as_float(c[0])) + __uint_as_float(c[1]);
            }
            sum[0] = s;
        } else {
#pragma unroll
            for (int t = 0; t < TT; ++t) sum[t] = group_row_sum<NO>(y[t]);  // valid in lane group 0
        }
        return;
    }
#endif
    if constexpr (SPLIT && FAST && HT >= 2) {
        float xin[TT][4];
        const int slot = tab[L.feat_tab + g];
#pragma unroll
        for (int t = 0; t < TT; ++t) xin[t][0] = state[ro[t] + slot];
        f32x4 A[TT][HT], B[TT][HT];
        dense_first_split<HT, TT>(buf, N, xin, A);
        bias_act<HT, TT, true>(buf, DF_ACT_RELU, A, false);
        dense_hidden_split<HT, TT>(buf + N.off_h, A, B);
        bias_act<HT, TT, true>(buf, DF_ACT_RELU, B, false);
        tail<HT, TT, OUTV, RELU, PH, NO>(buf, N, L, tab, state, ro, sum, B);
        return;
    }
    // conditioner input: features k = 4r + g of vcat(θ,z)[axis_nn] (zero slot pads)
    float xin[TT][4];
    const int32_t* feat = tab + L.feat_tab;
    constexpr int KS = FAST ? 1 : 0;
    const int ks = FAST ? 1 : N.ks;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int slot = (r < ks) ? feat[4 * r + g] : 0;
#pragma unroll
        for (int t = 0; t < TT; ++t) xin[t][r] = (r < ks) ? state[ro[t] + slot] : 0.f;
    }

    f32x4 A[TT][HT], B[TT][HT];
    dense_first<HT, TT, KS>(buf, N, xin, A);
    bias_act<HT, TT, RELU>(buf + N.off_b0, N.act0, A, FAST ? false : !N.fold0);
    if (FAST || N.nh == 1) {  // the default _dflt_net (n_sublayers = 2): one H×H Dense
        dense_hidden<HT, TT>(buf + N.off_h, A, B);
        bias_act<HT, TT, RELU>(buf + N.off_h + HT * HT * 1024, N.acth, B);
        tail<HT, TT, OUTV, RELU, PH, NO>(buf, N, L, tab, state, ro, sum, B);
        return;
    }
    // hidden Denses alternate A -> B -> A ... (no register copies)
    bool in_a = true;
    for (int k = 0; k < N.nh; k += 2) {
        dense_hidden<HT, TT>(buf + N.off_h + k * N.hstride, A, B);
        bias_act<HT, TT, RELU>(buf + N.off_h + k * N.hstride + HT * HT * 1024, N.acth, B);
        in_a = false;
        if (k + 1 < N.nh) {
            dense_hidden<HT, TT>(buf + N.off_h + (k + 1) * N.hstride, B, A);
            bias_act<HT, TT, RELU>(buf + N.off_h + (k + 1) * N.hstride + HT * HT * 1024, N.acth, A);
            in_a = true;
        }
    }
    if (in_a) tail<HT, TT, OUTV, RELU, PH, NO>(buf, N, L, tab, state, ro, sum, A);
    else tail<HT, TT, OUTV, RELU, PH, NO>(buf, N, L, tab, state, ro, sum, B);
}

// The s-net and t-net of one RNVP layer evaluated together (FAST variant, exact f32,
// both nets in the resident stage, NO = n_af outputs each): they read the same
// conditioner features (vcat(θ,z)[axis_nn], RNVP.jl:174-177), so their MFMA chains and
// GEMV tails are independent and interleave, which halves the dependent latency of a
// layer for a wave that has no other work (small batches: profiles/r04_phase_cfg1.txt).
// The coupling is then applied in the reference's order with the same roundings as the
// two phases of net_tiles: forward z·exp(s) then + t (RNVP.jl:182-184), inverse (x − t)
// then ·exp(−s) (RNVP.jl:86-90); ssum[t] = Σ_k s_k in row order (lane group 0).
template <int HT, int TT, bool RELU, bool FWDP, int NO>
__device__ __forceinline__ void net_pair_tiles(const uint8_t* buf, const ULayer& L, const int32_t* tab, float* state,
                                               const int (&ro)[TT], float (&ssum)[TT]) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    float xin[TT][4];
    const int slot_in = tab[L.feat_tab + g];
#pragma unroll
    for (int t = 0; t < TT; ++t) xin[t][0] = state[ro[t] + slot_in];
    f32x4 As[TT][HT], At[TT][HT], Bs[TT][HT], Bt[TT][HT];
    dense_first<HT, TT, 1>(buf, L.s, xin, As);
    dense_first<HT, TT, 1>(buf, L.t, xin, At);
    bias_act<HT, TT, RELU>(buf + L.s.off_b0, L.s.act0, As, false);
    bias_act<HT, TT, RELU>(buf + L.t.off_b0, L.t.act0, At, false);
    dense_hidden<HT, TT>(buf + L.s.off_h, As, Bs);
    dense_hidden<HT, TT>(buf + L.t.off_h, At, Bt);
    bias_act<HT, TT, RELU>(buf + L.s.off_h + HT * HT * 1024, L.s.acth, Bs);
    bias_act<HT, TT, RELU>(buf + L.t.off_h + HT * HT * 1024, L.t.acth, Bt);
    float ys[TT], yt[TT];
    out_valu_t<HT, TT, NO>(buf, L.s, Bs, ys);
    out_valu_t<HT, TT, NO>(buf, L.t, Bt, yt);
    const int slot = tab[L.af_tab + (g < NO ? g : 0)];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        if (g < NO) {
            float v = state[ro[t] + slot];
            if (FWDP) {
                v = v * expf(ys[t]);
                v = v + yt[t];
            } else {
                v = v - yt[t];
                v = v * expf(-ys[t]);
            }
            state[ro[t] + slot] = v;
        }
        ssum[t] = group_row_sum<NO>(ys[t]);
    }
}

}  // namespace uni

#ifndef DF_UNI_WAVES
#define DF_UNI_WAVES 4
#endif
#ifndef DF_FAST_WAVES
#define DF_FAST_WAVES 4
#endif

template <int HT, int MODE, bool OUTV, bool RELU, bool FAST = false, bool SPLIT = false>
__global__ void __launch_bounds__(kBlockThreads, FAST ? DF_FAST_WAVES : DF_UNI_WAVES)
uniform_kernel(ChainArgs a) {
    using namespace uni;
    constexpr bool FWD = (MODE == MODE_FWD || MODE == MODE_FWD_INPLACE);
    constexpr bool WANT_LDJ = (MODE != MODE_FWD_INPLACE);

    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int stage_area = a.stage_bytes * a.n_stage_bufs;
    int32_t* tab = reinterpret_cast<int32_t*>(smem + stage_area);
    float* state = reinterpret_cast<float*>(smem + stage_area + a.tab_bytes);

    ClockStamp clk;
    clk.begin(a);
#ifdef DF_PHASE_STAMPS  // diagnostic build (wrong outputs): wave 0 of workgroup 0 stamps its phases
    uint64_t ph[16] = {};
#define DF_PH(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) ph[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DF_PH(i) do {} while (0)
#endif
    DF_PH(0);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int d = a.d, n = a.n, stride = a.stride, nd = n + d;
    const int nt = a.tiles;
    const int S = kWavesPerBlock * 16 * nt;
    const int cA = nd + 1, cE = nd + 2;
    const int64_t s0 = (int64_t)blockIdx.x * S;
    const int nvalid = (int)((a.batch - s0) < S ? (a.batch - s0) : S);

    Stager sg;
    sg.base = smem;
    sg.bytes = a.stage_bytes;
    sg.sched = FWD ? a.sched_fwd : a.sched_bwd;
    sg.n = FWD ? a.n_sched_fwd : a.n_sched_bwd;
    constexpr bool kLaneLocalDma = SPLIT && DF_SPLIT_PREFETCH;  // df_chain_impl.h dma_stage
    constexpr bool kSplitHead = SPLIT && FAST && OUTV && HT >= 2 && DF_SPLIT_HEAD_REGS;  // net_tiles' read-ahead path
    impl::stager_start<kLaneLocalDma>(sg, a);

    // Copy-in of the tables, the NormalizationLayer bounds (a.params, kept in LDS right
    // after the tables) and the state tile.  Fast form: every thread issues ALL its loads
    // — up to four table words, one bound, one θ bound per lane, its sample row's z and
    // θ — before its first LDS store, so the copy costs one memory latency; three serial
    // load → store loops cost three (≈1.5 k cycles each, profiles/r04_phase_cfg1.txt),
    // which is a third of a config-1 launch at B = 4096.
    float* tabf = reinterpret_cast<float*>(tab);
    constexpr int kRowMax = 8;  // fast copy-in: d, n <= 8 (every default-shape chain of the configs)
    const bool fast_copy = d <= kRowMax && n <= kRowMax && a.n_par <= kBlockThreads && a.tab_ints <= 4 * kBlockThreads;
    auto row_init = [&](int smp) {  // [0 | ldj_chain | ldj_elem | 1 (folded-bias input)]
        for (int c = nd; c < stride; ++c) state[smp * stride + c] = (c == nd + 3) ? 1.f : 0.f;
    };
    auto theta_in = [&](float v, float lo, float hi) {  // normalize_input (Data.jl:213-218)
        const float diff = hi - lo;
        return (diff == 0.f) ? 0.f : (v - lo) / diff;
    };
    if (fast_copy) {
        const int n_tab = a.tab_ints, n_par = a.n_par;
        int tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tid + u * kBlockThreads;
            tv[u] = i < n_tab ? a.tables[i] : 0;
        }
        const float pv = tid < n_par ? a.params[tid] : 0.f;
        const bool norm_th = a.tmin != nullptr;
        const float blo = (norm_th && lane < n) ? a.tmin[lane] : 0.f;  // lane c: column c's bounds
        const float bhi = (norm_th && lane < n) ? a.tmax[lane] : 0.f;
        const int smp = tid;                                           // this thread's first row
        const bool valid = smp < nvalid;
        float zr[kRowMax], tr[kRowMax];
#pragma unroll
        for (int c = 0; c < kRowMax; ++c)
            if (c < d) zr[c] = valid ? a.zin[(s0 + smp) * d + c] : 0.f;
#pragma unroll
        for (int c = 0; c < kRowMax; ++c)
            if (c < n) tr[c] = valid ? a.theta[(s0 + smp) * n + c] : 0.f;
        // every load is in flight: the stores
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tid + u * kBlockThreads;
            if (i < n_tab) tab[i] = tv[u];
        }
        if (tid < n_par) tabf[n_tab + tid] = pv;
#pragma unroll
        for (int c = 0; c < kRowMax; ++c)
            if (c < n) {
                const float lo = __shfl(blo, c), hi = __shfl(bhi, c);
                if (smp < S) state[smp * stride + c] = (norm_th && valid) ? theta_in(tr[c], lo, hi) : tr[c];
            }
        if (smp < S) {
#pragma unroll
            for (int c = 0; c < kRowMax; ++c)
                if (c < d) state[smp * stride + n + c] = zr[c];
            row_init(smp);
        }
        // rows beyond the first kBlockThreads (tiles > 4): element by element
        for (int i = tid + kBlockThreads * d; i < S * d; i += kBlockThreads) {
            const int r = i / d, c = i - r * d;
            state[r * stride + n + c] = r < nvalid ? a.zin[(s0 + r) * d + c] : 0.f;
        }
        for (int i = tid + kBlockThreads * n; i < S * n; i += kBlockThreads) {
            const int r = i / n, c = i - r * n;
            float v = 0.f;
            if (r < nvalid) {
                v = a.theta[(s0 + r) * n + c];
                if (norm_th) v = theta_in(v, a.tmin[c], a.tmax[c]);
            }
            state[r * stride + c] = v;
        }
        for (int r = tid + kBlockThreads; r < S; r += kBlockThreads) row_init(r);
    } else {
        for (int i = tid; i < a.tab_ints; i += kBlockThreads) tab[i] = a.tables[i];
        for (int i = tid; i < S * d; i += kBlockThreads) {
            const int smp = i / d, c = i - smp * d;
            float v = 0.f;
            if (smp < nvalid) v = a.zin[(s0 + smp) * d + c];
            state[smp * stride + n + c] = v;
        }
        for (int i = tid; i < S * n; i += kBlockThreads) {
            const int smp = i / n, c = i - smp * n;
            float v = 0.f;
            if (smp < nvalid) {
                v = a.theta[(s0 + smp) * n + c];
                if (a.tmin) v = theta_in(v, a.tmin[c], a.tmax[c]);
            }
            state[smp * stride + c] = v;
        }
        for (int i = tid; i < S; i += kBlockThreads) row_init(i);
    }
    DF_PH(1);
    DF_PH(2);
    DF_PH(3);
    __syncthreads();
    DF_PH(4);

    const int row0 = ((wave * nt) * 16 + j) * stride;  // tile tt: row0 + tt*16*stride
#ifdef DF_NO_PAIR  // A/B build: the s and t nets of a layer one after the other
    constexpr bool no_pair = true;
#else
    constexpr bool no_pair = false;
#endif
    const int tstep = 16 * stride;
    bool have_acc = false;
    // read-ahead SPLIT bodies: the lane's two fragment offsets as values held across all
    // bodies (SplitTail).  What the compiler then hoists out of the bodies costs some ten
    // VGPRs: the hidden-64 forward instances have them (117 -> 125, 114 -> 123 of 128); the
    // inverse and logpdf instances (123, 125) would spill, and the hidden-32 instances would
    // lose their fifth wave (90 -> 100 VGPRs)
    constexpr bool kHoldLanes = kSplitHead && HT == 4 && FWD;
    int lane16 = lane << 4, group16 = g << 4;
    if constexpr (kHoldLanes) asm volatile("" : "+v"(lane16), "+v"(group16));

    auto ldj_update = [&](int ro, float l, bool first_in_elem, bool last_in_elem) {
        if (!WANT_LDJ || g != 0) return;
        const float e = first_in_elem ? l : state[ro + cE] + l;
        state[ro + cE] = e;
        if (last_in_elem) state[ro + cA] = have_acc ? state[ro + cA] + e : e;
    };

    for (int it = 0; it < a.n_layers; ++it) {
        const int li = FWD ? it : a.n_layers - 1 - it;
        // descriptors through the constant address space: scalar loads (the host
        // writes them before the launch; nothing in the kernel stores to them)
        using CULayer = const __attribute__((address_space(4))) ULayer;
#ifdef DF_PHASE_STAMPS  // diagnostic: the whole descriptor loaded (and waited for) up front
        const ULayer L = *(const ULayer*)(&((CULayer*)(uintptr_t)a.ulayers)[li]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (it == 1) DF_PH(13);
#else
        const ULayer& L = *(const ULayer*)(&((CULayer*)(uintptr_t)a.ulayers)[li]);
#endif
        const int kind = L.kind;
        const bool first_in_elem = FWD ? L.elem_start : L.elem_end;
        const bool last_in_elem = FWD ? L.elem_end : L.elem_start;
        // SPLIT: the rarely run loops below (normalisation, snapshots) take their lane
        // indices from an opaque copy of the thread id.  From the kernel's own they are
        // loop-invariant, and their hoisted address arithmetic held some fifteen VGPRs
        // across every net body of an instance that has 128.
        int gl = g, jl = j, wavel = wave, row0l = row0;
        if constexpr (kLaneLocalDma) {
            if (kind == DF_LAYER_NORM || (!FWD && a.snap)) {
                int tx = tid;
                asm volatile("" : "+v"(tx));
                gl = (tx & 63) >> 4, jl = tx & 15, wavel = tx >> 6;
                row0l = ((wavel * nt) * 16 + jl) * stride;
            }
        }
        if (kind == DF_LAYER_NORM) {
            const float al = L.alpha, be = L.beta, delta = be - al;
            auto norm = [&](const auto* xmn) {
                const auto* xmx = xmn + d;
                for (int tt = 0; tt < nt; ++tt) {
                    const int ro = row0l + tt * tstep;
                    for (int i = gl; i < d; i += 4) {
                        const float lo = xmn[i], hi = xmx[i], xd = hi - lo;
                        float v = state[ro + n + i];
                        if (FWD) v = ((xd * v - al * hi) + be * lo) / delta;
                        else v = (be * (v - lo) + al * (hi - v)) / xd;
                        state[ro + n + i] = v;
                    }
                    ldj_update(ro, FWD ? L.ldj_const : -L.ldj_const, first_in_elem, last_in_elem);
                }
            };
            if (fast_copy) norm(tabf + a.tab_ints + L.norm_off);  // the bounds were copied to LDS
            else norm(a.params + L.norm_off);
        } else {
            const bool rnvp = (kind == DF_LAYER_RNVP);
            // this wave's tiles in groups of kTT (nt is a multiple of kTT)
            constexpr int kTT = FAST ? kFastTileGroup : kUniformTileGroup;
            auto tiles_loop = [&](const UNet& N, const SplitHead& hd, auto ph_tag, auto no_tag, bool sphase,
                                  float sign) {
                constexpr int PH = decltype(ph_tag)::value;
                constexpr int NO = decltype(no_tag)::value;
                const uint8_t* buf = sg.buf();
                for (int tt = 0; tt < nt; tt += kTT) {
                    int ro[kTT];
                    float ssum[kTT];
                    // SPLIT: the row offsets from one opaque copy of row0 per tile group:
                    // left to itself the compiler strength-reduces every state address of
                    // the loop into its own VGPR induction variable (six), which the SPLIT
                    // kernel at 128 VGPRs spills — and a reload's vmcnt(0) also waits for the
                    // stage DMA issued just before (headline 1583 -> 1623 Msamples/s,
                    // gpurun_out/ab4e; the exact-f32 kernels keep the induction variables:
                    // config 1 at 2^20 lost 0.9% with the opaque copy)
                    int r0 = row0;
                    if constexpr (SPLIT) asm volatile("" : "+v"(r0));
#pragma unroll
                    for (int t = 0; t < kTT; ++t) ro[t] = r0 + (tt + t) * tstep;
                    SplitTail<kTT> tl;
                    tl.ce = cE, tl.ts = tstep, tl.l16 = lane16, tl.g16 = group16;
                    net_tiles<HT, kTT, OUTV, RELU, PH, FAST, NO, SPLIT, WANT_LDJ, kHoldLanes>(buf, N, L, tab, state, ro,
                                                                                              ssum, hd, tl);
                    constexpr bool SPH = (PH == impl::PH_S_FWD || PH == impl::PH_S_BWD);
                    if constexpr (kSplitHead && NO > 0 && SPH) {
                        // ldj_update on the words the body read with the coupling's old values:
                        // the same additions in the same order, the three uniform flags select
                        // between values, and no LDS round trip stands between read and write.
                        // Pair form (split_tail_pair): every lane group holds its row's Σ s, so all
                        // lanes store (copies write the same bits), but with three outputs, where
                        // lane groups 0 and 3 hold the two rows' sums; else lane group 0 stores.
                        constexpr bool PAIR = split_tail_pair(kTT, NO, kHoldLanes);
                        constexpr int NU = split_tail_rows(kTT, NO, kHoldLanes);
                        if constexpr (WANT_LDJ) {
                            if (PAIR ? (NO != 3 || g == 0 || g == 3) : g == 0) {
#pragma unroll
                                for (int u = 0; u < NU; ++u) {
                                    const float l = sign * ssum[u];
                                    const float e = first_in_elem ? l : tl.e_old[u] + l;
                                    state[tl.row[u] + tl.lcol] = e;
                                    if (last_in_elem) state[tl.row[u] + tl.lcol - 1] = have_acc ? tl.a_old[u] + e : e;
                                }
                            }
                        }
                    } else {
#pragma unroll
                        for (int t = 0; t < kTT; ++t) {
                            if (sphase) ldj_update(ro[t], sign * ssum[t], first_in_elem, last_in_elem);
                            else if (!rnvp) ldj_update(ro[t], 0.f, first_in_elem, last_in_elem);
                        }
                    }
                }
            };
            auto run_net = [&](const UNet& N, auto ph_tag, bool sphase, float sign) {
                // read-ahead SPLIT path: every descriptor word of the net as a value, loaded
                // here in one round trip before the stage switch and pinned: left at their
                // uses the scalar loads sink into the tile-group loop, each one a wait of its
                // own in front of the body's LDS reads
                SplitHead hd{0, 0, 0};
                int stage = N.stage, n_out = N.n_out;
                if constexpr (kSplitHead) {
                    hd = SplitHead{N.off_w0, L.feat_word, L.af_word};
                    asm volatile("" : "+s"(stage), "+s"(n_out), "+s"(hd.off_w0), "+s"(hd.feat_word), "+s"(hd.af_word));
                }
                impl::ensure_stage<kLaneLocalDma>(stage, sg, a);
                if constexpr (FAST && OUTV) {  // output count fixed per net: branch-free tails
                    switch (n_out) {
                        case 1: tiles_loop(N, hd, ph_tag, std::integral_constant<int, 1>{}, sphase, sign); break;
                        case 2: tiles_loop(N, hd, ph_tag, std::integral_constant<int, 2>{}, sphase, sign); break;
                        case 3: tiles_loop(N, hd, ph_tag, std::integral_constant<int, 3>{}, sphase, sign); break;
                        default: tiles_loop(N, hd, ph_tag, std::integral_constant<int, 4>{}, sphase, sign); break;
                    }
                } else {
                    tiles_loop(N, hd, ph_tag, std::integral_constant<int, 0>{}, sphase, sign);
                }
            };
            using PSF = std::integral_constant<int, impl::PH_S_FWD>;
            using PTF = std::integral_constant<int, impl::PH_T_FWD>;
            using PTB = std::integral_constant<int, impl::PH_T_BWD>;
            using PSB = std::integral_constant<int, impl::PH_S_BWD>;
            bool paired = false;
            if constexpr (FAST && OUTV && !SPLIT && HT <= 2) {
                // s and t together when both sit in one stage with the same output count
                if (rnvp && L.s.stage == L.t.stage && L.s.n_out == L.t.n_out && !no_pair) {
                    impl::ensure_stage(L.s.stage, sg, a);
                    auto pair_loop = [&](auto no_tag) {
                        constexpr int NO = decltype(no_tag)::value;
                        const uint8_t* buf = sg.buf();
                        for (int tt = 0; tt < nt; tt += kTT) {
                            int ro[kTT];
                            float ssum[kTT];
#pragma unroll
                            for (int t = 0; t < kTT; ++t) ro[t] = row0 + (tt + t) * tstep;
                            net_pair_tiles<HT, kTT, RELU, FWD, NO>(buf, L, tab, state, ro, ssum);
#pragma unroll
                            for (int t = 0; t < kTT; ++t)
                                ldj_update(ro[t], FWD ? ssum[t] : -ssum[t], first_in_elem, last_in_elem);
                        }
                    };
                    switch (L.s.n_out) {
                        case 1: pair_loop(std::integral_constant<int, 1>{}); break;
                        case 2: pair_loop(std::integral_constant<int, 2>{}); break;
                        case 3: pair_loop(std::integral_constant<int, 3>{}); break;
                        default: pair_loop(std::integral_constant<int, 4>{}); break;
                    }
                    paired = true;
                }
            }
            if (paired) {
            } else if (FWD) {
#ifdef DF_PHASE_STAMPS
                if (it == 1) DF_PH(11);
#endif
                if (rnvp) run_net(L.s, PSF{}, true, 1.f);
#ifdef DF_PHASE_STAMPS
                if (it == 1) DF_PH(12);
#endif
                run_net(L.t, PTF{}, false, 1.f);
            } else {
                run_net(L.t, PTB{}, false, 1.f);
                if (rnvp) run_net(L.s, PSB{}, true, -1.f);  // ln_det_jac = -Σ s
            }
        }
        have_acc = have_acc || last_in_elem;
#ifdef DF_PHASE_STAMPS
        if (it == 0) DF_PH(5);
        if (it == 1) DF_PH(6);
        if (it == 2) DF_PH(7);
        if (it == 3) DF_PH(8);
#endif
        if (!FWD && a.snap) {  // training: keep every layer's output for the reverse sweep
            float* dst = a.snap + (int64_t)li * a.batch * d;
            for (int tt = 0; tt < nt; ++tt) {
                const int smp = (wavel * nt + tt) * 16 + jl;
                if (smp < nvalid)
                    for (int i = gl; i < d; i += 4) dst[(s0 + smp) * d + i] = state[row0l + tt * tstep + n + i];
            }
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (MODE == MODE_LOGPDF) {
        double part = 0.0;
        if (g == 0) {
            for (int tt = 0; tt < nt; ++tt) {
                const int ro = row0 + tt * tstep;
                const int smp = (wave * nt + tt) * 16 + j;
                float q = 0.f;
                for (int i = 0; i < d; ++i) {
                    const float zz = state[ro + n + i];
                    q = q + zz * zz;
                }
                const float lp = (a.c0 - q / 2.f) + state[ro + cA];
                if (smp < nvalid) {
                    if (a.lp_out) a.lp_out[s0 + smp] = lp;
                    part += (double)lp;
                }
            }
        }
        if (a.partial) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
            __syncthreads();
            double* red = reinterpret_cast<double*>(smem);
            if (lane == 0) red[wave] = part;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int w = 0; w < kWavesPerBlock; ++w) s += red[w];
                a.partial[blockIdx.x] = s;
            }
        }
        if (!a.xout) {
            clk.end(a);
            return;
        }
    }
    __syncthreads();
    for (int i = tid; i < S * d; i += kBlockThreads) {
        const int smp = i / d, c = i - smp * d;
        if (smp < nvalid) a.xout[(s0 + smp) * d + c] = state[smp * stride + n + c];
    }
    if (WANT_LDJ && MODE != MODE_LOGPDF && a.ldj_out) {
        for (int i = tid; i < nvalid; i += kBlockThreads) a.ldj_out[s0 + i] = state[i * stride + cA];
    }
    DF_PH(9);
#ifdef DF_PHASE_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DF_PH(10);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < 14; ++i) a.xout[i] = (float)(ph[i] - ph[0]);
    }
#endif
#undef DF_PH
    clk.end(a);
}

template <int HT, bool RELU, bool FAST = false, bool SPLIT = false>
void* uniform_kernel_ptr_r(int mode, bool outv) {
#define DF_U(M) (outv ? reinterpret_cast<void*>(&uniform_kernel<HT, M, true, RELU, FAST, SPLIT>) \
                      : reinterpret_cast<void*>(&uniform_kernel<HT, M, false, RELU, FAST, SPLIT>))
    switch (mode) {
        case MODE_FWD: return DF_U(MODE_FWD);
        case MODE_FWD_INPLACE: return DF_U(MODE_FWD_INPLACE);
        case MODE_BWD: return DF_U(MODE_BWD);
        default: return DF_U(MODE_LOGPDF);
    }
#undef DF_U
}

// variant index: bit 0 = OUTV, bit 1 = RELU, bit 2 = FAST (RELU only: one first-Dense
// k-step with the bias folded in, chain-wide), bit 3 = SPLIT (FAST with OUTV on the
// bf16x3 split stages; hidden widths 32 and 64)
template <int HT>
void* uniform_kernel_ptr(int mode, int variant) {
    const bool outv = variant & 1;
    if constexpr (HT >= 2) {
        if ((variant & 8) && (variant & 4) && outv) return uniform_kernel_ptr_r<HT, true, true, true>(mode, true);
    }
    if (variant & 8) return nullptr;
    if (variant & 4) return uniform_kernel_ptr_r<HT, true, true>(mode, outv);
    return (variant & 2) ? uniform_kernel_ptr_r<HT, true>(mode, outv) : uniform_kernel_ptr_r<HT, false>(mode, outv);
}

template <int HT>
hipError_t launch_uniform_ht(int mode, int variant, const ChainArgs& a, unsigned grid, size_t lds, hipStream_t st) {
    void* args[] = {const_cast<ChainArgs*>(&a)};
    return hipLaunchKernel(uniform_kernel_ptr<HT>(mode, variant), dim3(grid), dim3(kBlockThreads), args, lds, st);
}

template <int HT>
hipError_t set_uniform_lds_limit_ht(size_t lds) {
    for (int mode = 0; mode < 4; ++mode)
        for (int v = 0; v < 16; ++v) {
            void* k = uniform_kernel_ptr<HT>(mode, v);
            if (!k) continue;
            hipError_t e = hipFuncSetAttribute(k,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

template <int HT>
hipError_t uniform_occupancy_ht(int mode, int variant, size_t lds, int* blocks) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, uniform_kernel_ptr<HT>(mode, variant), kBlockThreads,
                                                        lds);
}

}  // namespace df
