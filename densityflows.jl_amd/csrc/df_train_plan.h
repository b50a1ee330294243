// df_train_plan.h — the trainer's host plan (TrainPlan) and the plain structs and constants
// it shares with the training kernels.  Host-only, like df_plan.h: no HIP type, so
// df_train_plan.cpp builds with g++ and tests/train_plan_fingerprint.cpp checks every byte
// of it off the device.  df_train.h and df_ltrain.h include this header.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "df_plan.h"

namespace df {

namespace trn {
// Activation modes of the training kernels: σ' from the output alone, relu-only,
// or σ' of softplus / logcosh / swish, which needs the pre-activation.
enum { AM_Y = 0, AM_RELU = 1, AM_PRE = 2 };
}  // namespace trn

// One conditioner net of the specialised shape, as the training kernel sees it.
struct GNet {
    UNet u;                  // forward fragments (offsets rebased to the net's own LDS copy)
    int32_t n_in;            // conditioner inputs (|axis_nn|)
    int32_t h_true;          // hidden width
    int32_t off_w0t;         // transposed region: W0ᵀ fragments [kq < HT][lane][4]
    int32_t off_ht;          // transposed region: W_hᵀ fragments [kq][m][lane][4]
    int32_t fwd_bytes;       // forward region bytes (16-B multiple)
    int32_t t_bytes;         // transposed region bytes
    int64_t fwd_src;         // byte offset of the forward region in the chain blob
    int64_t t_src;           // byte offset of the transposed region in the training blob
    int32_t p_begin, p_count;          // the net's contiguous slice of the trainables
    int32_t w_off[3], b_off[3];        // first Dense, hidden Dense, output Dense (b_off -1: no bias)
    // SPLIT (chain plan.split, hidden 32/64, relu): the recompute runs on the net's
    // region of the chain's SPLIT blob (bitwise the inverse pass), W1ᵀδ and dW1 on
    // bf16x3 products; W1ᵀ planes [c][m][p][lane][8] in the trainer's split blob
    int32_t split;
    UNet su;                 // SPLIT forward region offsets (rebased to the net's LDS copy)
    int32_t sfwd_bytes;
    int64_t sfwd_src;        // byte offset of the net's region in the chain's SPLIT blob
    int32_t st_bytes;
    int64_t st_src;          // byte offset of its W1ᵀ planes in the trainer's split blob
};

enum : int { TR_PHASE_S = 0, TR_PHASE_T = 1 };

// ---- optimiser chains (df_train_create_opt; Optimisers.OptimiserChain) ----
// The rules of a chain, passed to the kernels by value: kind[r] is a df_opt_kind, p[r] its
// parameters (df_opt_rule::p).
constexpr int kOptMaxRules = 8;
struct OptChain {
    int32_t n;
    int32_t kind[kOptMaxRules];
    float p[kOptMaxRules][4];
};
// One 256-thread workgroup of the update kernel: elements [begin, begin + count) of the
// flat vectors, all of parameter tensor `tensor` (no workgroup spans two tensors).
struct OptBlock {
    int32_t begin, count, tensor;
};
constexpr int kOptThreads = 256;

constexpr int kLChunkBytes = 32 * 1024;  // layer-wise weight chunk (LDS, double-buffered)

struct SweepOp {
    int layer;   // index in plan.layers
    int net;     // index in TrainPlan::nets / lnets, -1 for a NormalizationLayer
    int phase;   // TR_PHASE_S / TR_PHASE_T
};

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

// What df_train_create_opt reads off the chain handle and its caller.
struct TrainPlanOpts {
    bool exact = false, no_wide = false;  // df_chain::exact, df_chain::no_wide
    bool split = false, wsplit = false;   // use_split(c), use_wsplit(c)
    int sweep = DF_SWEEP_AUTO;            // the requested df_sweep_form, with DF_SWEEP_SEPARATE
};

// One packed blob repack() regathers (TrainPlan::MP ... MLS, its launch order): the chain's blob, the trainer's
// transposed fragments, the wide blob and biases, the SPLIT and wide SPLIT blobs, the layer-wise blob, two plane blobs.
struct MapSrc {
    const std::vector<int32_t>*dst, *src;
    bool on, split;          // on: the blob exists; split: bf16x3 planes (launch_repack_split)
};

// Everything a trainer decides on the host before its first device call.
struct TrainPlan {
    enum { MP, MT, MW, MWB, MS, MWS, ML, MTS, MLS, kMaps };
    int64_t n_params = 0;
    int amode = 0;                    // fused kernel activation mode (trn::AM_*)
    bool layerwise = false;           // hidden width > 64, deep or wide-output conditioners
    int sweep_req = DF_SWEEP_AUTO;    // the requested form (df_sweep_form)
    bool separate = false;            // DF_SWEEP_SEPARATE: unmerged dW / front launches
    // The parameter tensors (one Dense weight or bias each) as slices of the flat vectors:
    // tensor k is [toff[k], toff[k+1]).
    std::vector<int32_t> toff;
    // fused path
    std::vector<GNet> nets;
    std::vector<int> net_nh;
    std::vector<SweepOp> ops;         // the reverse sweep of either path
    std::vector<uint8_t> tblob;       // transposed fragments
    std::vector<int32_t> tdst, tsrc;  // repack map (float index ← trainables index)
    std::vector<uint8_t> tsblob;      // SPLIT W1ᵀ planes of the fused path (GNet::st_src)
    std::vector<int32_t> tsdst, tssrc;  // repack map (byte offset ← trainables index·4 + plane)
    // layer-wise path
    std::vector<LNet> lnets;
    std::vector<uint8_t> lblob;       // fragments (W and Wᵀ) then padded biases
    std::vector<int32_t> ldst, lsrc;  // repack map (float index ← trainables index)
    std::vector<uint8_t> lsblob;      // SPLIT planes of the layer-wise Wᵀ operands (LOp::sfrag)
    std::vector<int32_t> lsdst, lssrc;  // repack map (byte offset ← trainables index·4 + plane)
    int lwidth = 16;                  // widest activation row (floats)
    int lmax_h = 1;                   // activation buffers needed (hidden Denses + 1)
    bool any_pre = false;
    // H0-free sweep (DF_SWEEP_H0FREE) as planned: the chain is eligible.  df_train::fmode is the live flag
    bool fmode = false;
    // Optimiser chain.  A chain that is exactly [Adam] is not one: chain_mode stays false and df_train_apply
    // launches adam_kernel.  The trainer copies och and adam (df_train_adjust changes η there, not here).
    bool chain_mode = false;
    OptChain och{};
    int och_clip = -1;                // index of the chain's ClipNorm (-1: none): the rules before it
                                      //   run inside the Σ dx² kernel too
    int och_eta = -1;                 // the rule df_train_adjust sets η of: the Adam, else the first Descent
    df_adam adam{1e-3f, 0.9f, 0.999f, 1e-8f};
    std::vector<OptBlock> oblocks;    // chain_mode: the update kernel's workgroup → tensor table

    // The repack table's sources.  The pointers hold while P and this plan stay where they are.
    std::array<MapSrc, kMaps> map_sources(const Plan& P) const {
        return {{{&P.pack_dst, &P.pack_src, true, false},
                 {&tdst, &tsrc, !tdst.empty(), false},
                 {&P.wpack_dst, &P.wpack_src, P.wide != 0, false},
                 {&P.wbias_dst, &P.wbias_src, P.wide != 0, false},
                 {&P.spack_dst, &P.spack_src, P.split != 0, true},
                 {&P.wspack_dst, &P.wspack_src, P.wsplit != 0, true},
                 {&ldst, &lsrc, !ldst.empty(), false},
                 {&tsdst, &tssrc, !tsdst.empty(), true},
                 {&lsdst, &lssrc, !lsdst.empty(), true}}};
    }
};

// Plans a trainer of the chain P under the rules.  Checks, in this order: the rules, the sweep
// form, the fused sweep, the layer-wise sweep.  Returns a df_status, with *err set on failure.
int build_train_plan(const Plan& P, const TrainPlanOpts& o, const df_opt_rule* rules, int n_rules, TrainPlan* out,
                     std::string* err);

}  // namespace df
