// df_plan.cpp — validate a df_chain_desc and pack it for the fused kernels.
//
// Reference semantics restated here (DensityFlows.jl v1.0.0):
//   * conditioner input = vcat(θ, z)[axis_nn]        src/affine/RNVP.jl:157,174,196
//     → the kernel keeps each sample's state row as [θ (n) | z (d) | 0] in LDS,
//       so a 1-based axis_nn entry k is the state slot k-1; padding slot n+d is 0.
//   * x_af = z_af .* exp.(s) .+ t, row k of s/t ↔ dim axis_af[k]   RNVP.jl:182-184
//     → af table: slot n + axis_af[k] - 1.
//   * s/t nets: Chain(Dense(in,h,σ), (n-1)×Dense(h,h,σ), Dense(h,out))  Layers.jl:33-50
//   * Flux.Dense weight is (out, in) column-major: W[i + out*k].
//
// build_plan (at the end of the file) is the sequence of the passes below; the four blobs
// (f32, SPLIT, wide, wide SPLIT) share the stage writer, the parameter sink and the
// fragment walkers of df_pack.h.
#include "df_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <set>
#include <sstream>
#include <utility>

#include "df_pack.h"

namespace df {
namespace {

using namespace pack;

struct Fail {
    int code;
    std::string msg;
};

[[noreturn]] void fail(int code, const std::string& m) { throw Fail{code, m}; }

int pow2_tiles(int t) {
    int p = 1;
    while (p < t) p *= 2;
    return p;
}

// The DF_* environment knobs, read once per plan.
struct Knobs {
    bool f32_exact, no_wide, force_generic, no_fold, no_fast;
    int stage_bytes = 0;      // DF_STAGE_KB: the f32 stage capacity (0: unset)
    int split_lds_bytes = 0;  // DF_SPLIT_LDS_KB: the SPLIT kernel's LDS target (0: unset)

    Knobs() {
        auto on = [](const char* name) {
            const char* e = std::getenv(name);
            return e && e[0] == '1';
        };
        f32_exact = on("DF_F32_EXACT");
        no_wide = on("DF_NO_WIDE");
        force_generic = on("DF_FORCE_GENERIC");
        no_fold = on("DF_NO_FOLD");
        no_fast = on("DF_NO_FAST");
        if (const char* e = std::getenv("DF_STAGE_KB")) stage_bytes = std::max(4, std::atoi(e)) * 1024;
        if (const char* e = std::getenv("DF_SPLIT_LDS_KB")) split_lds_bytes = std::max(32, std::atoi(e)) * 1024;
    }
};

// What the planner derives from the descriptor's shapes before it packs anything.
struct Shape {
    bool all_valu = true;       // every net ends in a VALU GEMV (kernel variant OUTV)
    int ht = 1;                 // kernel variant: max row tiles
    bool uniform_shape = true;  // every net has the default _dflt_net shape
    bool relu_only = true;      // ... with hidden σ = relu and output σ = identity
    bool fast_shape = true;     // FAST: every first Dense one k-step with its bias folded, n_sublayers = 2
    bool any_fold = false;
    std::vector<char> fold;     // per layer: first-Dense bias folded into k-slot 4·ks − 1
};

// A Dense of the descriptor beside its DevDense: W[row, k] and b[row] as parameters
// (a zero of the padding outside the Dense, and for the bias of a Dense without one).
struct DenseSrc {
    const df_dense_desc& D;
    const DevDense& DD;
    Param W(int row, int k) const {
        if (row >= D.out_dim || k >= D.in_dim) return {-1, 0.f};
        return {DD.w_off + row + D.out_dim * k, D.W[(size_t)row + (size_t)D.out_dim * k]};
    }
    Param b(int row) const {
        if (!D.b || row >= D.out_dim) return {-1, 0.f};
        return {DD.b_off + row, D.b[row]};
    }
};

template <class T>
void copy_layer_header(const DevLayer& L, T& out) {
    out.kind = L.kind;
    out.elem_start = L.elem_start;
    out.elem_end = L.elem_end;
    out.n_af = L.n_af;
    out.feat_tab = L.feat_tab;
    out.af_tab = L.af_tab;
    out.norm_off = L.norm_off;
    out.alpha = L.alpha;
    out.beta = L.beta;
    out.ldj_const = L.ldj_const;
}

// Stage schedule: the order in which a kernel's ensure_stage() calls ask for stages
// (forward: s-net then t-net per layer; inverse: layers reversed, t-net then s-net),
// consecutive duplicates removed.  net_stages(layer, is_s_net, push) lists a net's stages.
template <class L, class F>
std::vector<int32_t> stage_schedule(const std::vector<L>& layers, bool fwd, F net_stages) {
    std::vector<int32_t> out;
    auto push = [&](int s) {
        if (out.empty() || out.back() != s) out.push_back(s);
    };
    for (size_t it = 0; it < layers.size(); ++it) {
        const L& l = layers[fwd ? it : layers.size() - 1 - it];
        if (l.kind == DF_LAYER_NORM) continue;
        if (fwd && l.kind == DF_LAYER_RNVP) net_stages(l, true, push);
        net_stages(l, false, push);
        if (!fwd && l.kind == DF_LAYER_RNVP) net_stages(l, true, push);
    }
    return out;
}

// 16-sample tiles per wave whose state rows fit `target` bytes of LDS next to `fixed`
int tiles_that_fit(int fixed, int per_tile, int target) {
    int t = 0;
    while (t < kMaxTilesPerWave && fixed + (t + 1) * per_tile <= target) ++t;
    return t;
}

int tile_bytes(const Plan& P) { return kWavesPerBlock * 16 * P.stride * 4; }

// ---------- validation ----------

void check_net(const df_dense_desc* net, int nd, int in_dim, int out_dim, const char* which) {
    if (nd < 1) fail(DF_ERR_INVALID, std::string(which) + ": a conditioner needs at least one Dense");
    if (!net) fail(DF_ERR_INVALID, std::string(which) + ": null Dense array");
    int prev = in_dim;
    for (int k = 0; k < nd; ++k) {
        const df_dense_desc& D = net[k];
        if (D.in_dim != prev) {
            std::ostringstream os;
            os << which << ": Dense " << k + 1 << " expects " << D.in_dim << " inputs but receives " << prev;
            fail(DF_ERR_SHAPE, os.str());
        }
        if (D.out_dim < 1 || !D.W) fail(DF_ERR_INVALID, std::string(which) + ": empty Dense");
        if (D.act < DF_ACT_IDENTITY || D.act > DF_ACT_SWISH)
            fail(DF_ERR_INVALID, std::string(which) + ": unknown activation");
        if (k + 1 < nd && D.out_dim > kMaxHidden) fail(DF_ERR_UNSUPPORTED, "hidden width > 256");
        prev = D.out_dim;
    }
    if (prev != out_dim) {
        std::ostringstream os;
        os << which << ": output dimension " << prev << " does not match the " << out_dim
           << " transformed dimensions";
        fail(DF_ERR_SHAPE, os.str());
    }
}

void validate(const df_chain_desc* desc) {
    // the descriptor structs are unchanged since ABI 2 (ABI 3 added entry points only)
    if (desc->abi_version < 2 || desc->abi_version > DF_ABI_VERSION) fail(DF_ERR_INVALID, "ABI version mismatch");
    const int d = desc->d, n = desc->n;
    if (d < 1 || n < 0) fail(DF_ERR_INVALID, "d must be >= 1 and n >= 0");
    if (n + d > kMaxState) fail(DF_ERR_UNSUPPORTED, "n + d > 64 is outside the fused kernel's limits");
    if (desc->n_layers < 1 || !desc->layers) fail(DF_ERR_INVALID, "a FlowChain needs at least one element");
    if (desc->n_layers > kMaxLayers) fail(DF_ERR_UNSUPPORTED, "too many layers");
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (li > 0 && L.element < desc->layers[li - 1].element)
            fail(DF_ERR_INVALID, "layer element indices must be non-decreasing");
        if (L.kind == DF_LAYER_NORM) {
            if (!L.x_min || !L.x_max) fail(DF_ERR_INVALID, "NormalizationLayer without x_min/x_max");
            if (!(L.beta > L.alpha))
                fail(DF_ERR_INVALID, "Bounds of the normalisation need to be in the correct order, β > α.");
            continue;
        }
        if (L.kind != DF_LAYER_RNVP && L.kind != DF_LAYER_NICE) fail(DF_ERR_INVALID, "unknown layer kind");
        if (L.n_af < 1 || L.n_af > d || !L.axis_af) fail(DF_ERR_INVALID, "invalid axis_af");
        if (L.n_af > kMaxAf) fail(DF_ERR_UNSUPPORTED, "more than 32 transformed dims in one layer");
        std::set<int> seen;
        for (int k = 0; k < L.n_af; ++k) {
            int a = L.axis_af[k];
            if (a < 1 || a > d) fail(DF_ERR_INVALID, "The mask cannot contain values higher than the dimension");
            if (!seen.insert(a).second) fail(DF_ERR_INVALID, "axis_af contains a repeated dimension");
        }
        if (L.n_nn < 1 || L.n_nn > n + d || !L.axis_nn) fail(DF_ERR_INVALID, "invalid axis_nn");
        for (int k = 0; k < L.n_nn; ++k) {
            if (L.axis_nn[k] < 1 || L.axis_nn[k] > n + d) fail(DF_ERR_INVALID, "axis_nn out of range");
            // the conditioner must not read transformed dims (else the layer is not a coupling)
            if (L.axis_nn[k] > n && seen.count(L.axis_nn[k] - n))
                fail(DF_ERR_UNSUPPORTED, "axis_nn contains a transformed dimension");
        }
        if (L.kind == DF_LAYER_RNVP) {
            check_net(L.s_net, L.n_dense_s, L.n_nn, L.n_af, "s_net");
        } else if (L.n_dense_s != 0) {
            fail(DF_ERR_INVALID, "NICECouplingLayer has no s_net");
        }
        check_net(L.t_net, L.n_dense_t, L.n_nn, L.n_af, "t_net");
    }
}

// ---------- shape analysis ----------

// fn(net, n_dense) for the s-net (RNVP only) and then the t-net of a coupling layer
template <class F>
void for_each_net(const df_layer_desc& L, F fn) {
    if (L.kind == DF_LAYER_RNVP) fn(L.s_net, L.n_dense_s);
    fn(L.t_net, L.n_dense_t);
}

Shape analyse_shape(const df_chain_desc* desc, const Knobs& K) {
    Shape S;
    // A final Dense with <= 4 outputs after >= 1 hidden Dense is evaluated as a
    // VALU GEMV (kernel variant OUTV); the choice is chain-wide.
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        S.all_valu = S.all_valu && (L.kind == DF_LAYER_NICE || L.n_dense_s >= 2) && L.n_dense_t >= 2 && L.n_af <= 4;
    }
    // kernel variant: the row tiles of the widest MFMA operand
    int max_tiles = 1;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        for_each_net(L, [&](const df_dense_desc* net, int nd) {
            for (int k = 0; k < nd; ++k) {
                const bool valu_last = k + 1 == nd && S.all_valu;
                if (!valu_last) max_tiles = std::max(max_tiles, (net[k].out_dim + 15) / 16);
                if (k > 0) max_tiles = std::max(max_tiles, (net[k].in_dim + 15) / 16);
            }
        });
    }
    S.ht = pow2_tiles(max_tiles);
    if (S.ht > kMaxHidden / 16) fail(DF_ERR_UNSUPPORTED, "hidden width > 256");

    // Does every net have the default _dflt_net shape?
    // Dense(in<=16, H) -> nh × Dense(H, H) -> Dense(H, out) with ceil(H/16) = HT <= 4,
    // one hidden σ per net.  Such chains run on the specialised kernel, whose
    // first Dense uses a compact fragment layout (no k-quad padding).
    S.uniform_shape = S.ht <= 4 && !K.force_generic;
    for (int li = 0; li < desc->n_layers && S.uniform_shape; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        auto default_net = [&](const df_dense_desc* net, int nd) {
            if (nd < 2 || (L.n_nn + 3) / 4 > 4) return false;
            for (int k = 0; k + 1 < nd; ++k) {
                if ((net[k].out_dim + 15) / 16 != S.ht) return false;
                if (k >= 1 && net[k].act != net[1].act) return false;
                if (net[k].act != DF_ACT_RELU) S.relu_only = false;
            }
            if (net[nd - 1].act != DF_ACT_IDENTITY) S.relu_only = false;
            if (!S.all_valu && (net[nd - 1].out_dim + 15) / 16 > 2) return false;
            return true;
        };
        for_each_net(L, [&](const df_dense_desc* net, int nd) {
            S.uniform_shape = S.uniform_shape && default_net(net, nd);
        });
    }

    // First-Dense bias folding (specialised kernel; "pass 1c" in the kernels' comments).
    // With in < 4·ks the compact first Dense has a free k-slot; the LAST one
    // (k = 4·ks − 1) carries the bias against a state column that holds 1, so the
    // MFMA chain ends with fma(b, 1, Σ_k W x) = round(W*x + b): bit-identical to
    // the separate `W*x .+ b` (Flux) add it replaces.  Both nets of a layer share
    // the feature table, so a layer folds only when all of its nets have a bias.
    S.fold.assign(desc->n_layers, 0);
    const bool allow_fold = S.uniform_shape && !K.no_fold;
    S.fast_shape = allow_fold;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        const int ks = (L.n_nn + 3) / 4;
        const bool f = allow_fold && L.n_nn < 4 * ks && L.t_net[0].b != nullptr &&
                       (L.kind != DF_LAYER_RNVP || L.s_net[0].b != nullptr);
        S.fold[li] = f ? 1 : 0;
        S.any_fold = S.any_fold || f;
        // FAST: every layer folds into its one k-step, every conditioner has exactly one
        // hidden H×H Dense (n_sublayers = 2)
        S.fast_shape = S.fast_shape && f && ks == 1 && L.n_dense_t == 3 &&
                       (L.kind != DF_LAYER_RNVP || L.n_dense_s == 3);
    }
    return S;
}

// ---------- descriptors: tables, bounds, DevLayer, DevDense, trainables ----------

void add_norm_layer(const df_layer_desc& L, DevLayer& DL, Plan& P) {
    DL.norm_off = (int)P.params.size();
    for (int i = 0; i < P.d; ++i) P.params.push_back(L.x_min[i]);
    for (int i = 0; i < P.d; ++i) P.params.push_back(L.x_max[i]);
    DL.alpha = L.alpha;
    DL.beta = L.beta;
    // ldj = sum(log.(x_diff ./ δ)) in Float32, sequential (Base.sum, n < 16)
    // src/norm/Normalization.jl:88
    const float delta = L.beta - L.alpha;
    float acc = 0.f;
    for (int i = 0; i < P.d; ++i) {
        float xd = L.x_max[i] - L.x_min[i];
        float v = logf(xd / delta);
        acc = (i == 0) ? v : acc + v;
    }
    DL.ldj_const = acc;
}

void add_net(const df_dense_desc* net, int nd, int ks_state, const Shape& S, Plan& P) {
    int prev_tiles = 0;
    for (int k = 0; k < nd; ++k) {
        const df_dense_desc& D = net[k];
        DevDense DD{};
        DD.in_kind = (k == 0) ? IN_STATE : IN_HIDDEN;
        DD.n_out = D.out_dim;
        DD.in_dim = D.in_dim;
        DD.act = D.act;
        DD.has_bias = D.b ? 1 : 0;
        DD.out_valu = (k + 1 == nd) && S.all_valu ? 1 : 0;
        DD.kt_in = (k == 0) ? 0 : prev_tiles;
        DD.ks = (k == 0) ? ks_state : 4 * prev_tiles;
        DD.mt = DD.out_valu ? 0 : (D.out_dim + 15) / 16;
        DD.compact = (k == 0 && !DD.out_valu && S.uniform_shape) ? 1 : 0;
        prev_tiles = DD.mt;
        DD.w_off = (int32_t)P.trainables.size();
        P.trainables.insert(P.trainables.end(), D.W, D.W + (size_t)D.in_dim * D.out_dim);
        DD.b_off = -1;
        if (D.b) {
            DD.b_off = (int32_t)P.trainables.size();
            P.trainables.insert(P.trainables.end(), D.b, D.b + D.out_dim);
        }
        P.denses.push_back(DD);
        // bookkeeping: parameters and algorithmic FLOPs (2 × MACs)
        P.n_params += (int64_t)D.in_dim * D.out_dim + (D.b ? D.out_dim : 0);
        P.flops_per_sample += 2.0 * D.in_dim * D.out_dim;
    }
}

void describe_layers(const df_chain_desc* desc, const Shape& S, Plan& P) {
    const int zero_slot = P.n + P.d, one_slot = P.n + P.d + 3;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        DevLayer DL{};
        DL.kind = L.kind;
        DL.elem_start = (li == 0 || desc->layers[li - 1].element != L.element) ? 1 : 0;
        DL.elem_end = (li + 1 == desc->n_layers || desc->layers[li + 1].element != L.element) ? 1 : 0;
        if (L.kind == DF_LAYER_NORM) {
            add_norm_layer(L, DL, P);
            P.layers.push_back(DL);
            continue;
        }
        DL.n_af = L.n_af;
        const int ks_state = (L.n_nn + 3) / 4;
        // feature table [ks*4]: k = 4s + g → state slot of vcat(θ,z)[axis_nn[k]]
        DL.feat_tab = (int)P.tables.size();
        for (int k = 0; k < ks_state * 4; ++k)
            P.tables.push_back(k < L.n_nn ? L.axis_nn[k] - 1
                                          : (S.fold[li] && k == 4 * ks_state - 1) ? one_slot : zero_slot);
        DL.af_tab = (int)P.tables.size();
        for (int k = 0; k < L.n_af; ++k) P.tables.push_back(P.n + L.axis_af[k] - 1);
        DL.out_valu = S.all_valu ? 1 : 0;
        if (L.kind == DF_LAYER_RNVP) {
            DL.s_dense0 = (int)P.denses.size();
            DL.s_ndense = L.n_dense_s;
            add_net(L.s_net, L.n_dense_s, ks_state, S, P);
        }
        DL.t_dense0 = (int)P.denses.size();
        DL.t_ndense = L.n_dense_t;
        add_net(L.t_net, L.n_dense_t, ks_state, S, P);
        P.layers.push_back(DL);
    }
}

// ---------- the f32 blob ----------

// One packable item of a coupling layer, in kernel consumption order.
struct Item {
    enum Kind { CHUNK_KQ, BIAS, W3 } kind;
    int dense;   // index into plan.denses
    int kq;      // CHUNK_KQ: k-quad index
    int bytes;
};

// The items of the Denses [d0, d0 + nd): their bytes, and the items themselves when asked for.
int64_t dense_items(const Plan& P, int d0, int nd, std::vector<Item>* items = nullptr) {
    int64_t total = 0;
    auto add = [&](Item::Kind kind, int idx, int kq, int bytes) {
        total += bytes;
        if (items) items->push_back({kind, idx, kq, bytes});
    };
    for (int idx = d0; idx < d0 + nd; ++idx) {
        const DevDense& DD = P.denses[idx];
        if (DD.out_valu) {
            add(Item::W3, idx, 0, round_up((DD.n_out * 16 * DD.kt_in + 4) * 4, 16));
            continue;
        }
        if (DD.compact) add(Item::CHUNK_KQ, idx, 0, round_up(DD.mt * DD.ks * 256, 16));
        else
            for (int kq = 0; kq < (DD.ks + 3) / 4; ++kq) add(Item::CHUNK_KQ, idx, kq, DD.mt * 1024);
        add(Item::BIAS, idx, 0, DD.mt * 16 * 4);
    }
    return total;
}

// fn(stage) for every stage a net of the f32 blob reads, in the order the kernel asks for them
template <class F>
void f32_net_stages(const Plan& P, int d0, int nd, F fn) {
    for (int k = 0; k < nd; ++k) {
        const DevDense& D = P.denses[d0 + k];
        if (D.out_valu) {
            fn(D.w3_stage);
        } else {
            for (int c = 0; c < D.n_chunks; ++c) fn(P.chunks[D.chunk0 + c].stage);
            fn(D.bias_stage);
        }
    }
}

// Whole chain in one stage when it is small (loaded once per workgroup);
// otherwise 24 KiB stages, double-buffered in LDS, one net per stage
// whenever a net fits.
int f32_stage_cap(const df_chain_desc* desc, const Shape& S, const Knobs& K, const Plan& P) {
    int64_t total_bytes = 0, biggest_net = 0;
    for (const DevLayer& L : P.layers) {
        if (L.kind == DF_LAYER_NORM) continue;
        const int64_t sb = dense_items(P, L.s_dense0, L.s_ndense), tb = dense_items(P, L.t_dense0, L.t_ndense);
        total_bytes += sb + tb;
        biggest_net = std::max(biggest_net, std::max(sb, tb));
    }
    if (total_bytes <= kSingleStageCap) return kSingleStageCap;
    if (K.stage_bytes) return K.stage_bytes;
    // Wide conditioners (>= 128 hidden) run one 16-sample tile per wave, so the
    // stage-switch barrier is amortised over the MFMAs of one stage: give them
    // the largest stages that still fit twice next to the state tile.
    int cap = kStageCap;
    if (P.ht >= 8 && !S.uniform_shape) {
        int tab_ints = 0;
        for (int li = 0; li < desc->n_layers; ++li)
            if (desc->layers[li].kind != DF_LAYER_NORM)
                tab_ints += 4 * ((desc->layers[li].n_nn + 3) / 4) + desc->layers[li].n_af;
        const int room = (160 * 1024 - tile_bytes(P) - round_up(tab_ints * 4, 16) - 1024) / 2;
        cap = std::max(kStageCap, std::min(kBigStageCap, room / kStageAlign * kStageAlign));
    }
    // The specialised kernel needs every net whole in one stage.  A hidden-64 net with an
    // MFMA output Dense and 13-16 inputs is 24.5 KiB (at most 28.6 KiB with 32 outputs):
    // the stage grows to hold it, as the SPLIT packing's does (build_split).
    if (S.uniform_shape) cap = std::max(cap, round_up((int)biggest_net, kStageAlign));
    return cap;
}

// Record that k-quad `kq` of a Dense lies at (stage, off): a new chunk, or one more k-quad
// of the Dense's last chunk when contiguous with it in the same stage.
void add_chunk(Plan& P, DevDense& DD, int stage, int off, int kq) {
    if (DD.n_chunks > 0) {
        DevChunk& C = P.chunks[DD.chunk0 + DD.n_chunks - 1];
        if (C.stage == stage && C.lds_off + (C.kq_end - C.kq_begin) * DD.mt * 1024 == off && C.kq_end == kq) {
            C.kq_end++;
            return;
        }
    } else {
        DD.chunk0 = (int)P.chunks.size();
    }
    P.chunks.push_back({stage, off, kq, kq + 1});
    DD.n_chunks++;
}

void pack_f32(const df_chain_desc* desc, const Shape& S, const Knobs& K, Plan& P) {
    StageWriter stages(P.blob, P.stages, &P.stage_max, f32_stage_cap(desc, S, K, P));
    ParamSink<uint8_t> sink(P.blob, P.pack_dst, P.pack_src, ParamSink<uint8_t>::WORDS);
    std::vector<Item> items;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        const DevLayer& DL = P.layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        items.clear();
        const int64_t s_bytes = dense_items(P, DL.s_dense0, DL.s_ndense, &items);
        const size_t t_first = items.size();  // the t-net's first item
        const int64_t t_bytes = dense_items(P, DL.t_dense0, DL.t_ndense, &items);
        // Keep a layer — else each net — inside one stage whenever it fits.
        auto keep_whole = [&](int64_t bytes) {
            if (bytes > stages.remaining() && bytes <= stages.cap()) stages.begin_stage();
        };
        keep_whole(s_bytes + t_bytes);
        for (size_t ii = 0; ii < items.size(); ++ii) {
            const Item& it = items[ii];
            if (ii == 0 && t_first > 0) keep_whole(s_bytes);
            if (ii == t_first) keep_whole(t_bytes);
            DevDense& DD = P.denses[it.dense];
            const bool s_net = ii < t_first;
            const DenseSrc D{s_net ? L.s_net[it.dense - DL.s_dense0] : L.t_net[it.dense - DL.t_dense0], DD};
            if (it.bytes > stages.cap()) fail(DF_ERR_UNSUPPORTED, "packed item exceeds the LDS stage buffer");
            const StageWriter::Slot at = stages.alloc(it.bytes);
            auto W = [&](int64_t q, int row, int k) { sink.f32(at.at + 4 * q, D.W(row, k)); };
            auto B = [&](int64_t q, int row) { sink.f32(at.at + 4 * q, D.b(row)); };
            if (it.kind == Item::BIAS) {
                DD.bias_stage = at.stage;
                DD.bias_lds = at.off;
                for (int row = 0; row < DD.mt * 16; ++row) B(row, row);
            } else if (it.kind == Item::W3) {  // VALU GEMV output  [o][16*kt_in] then b[4]
                DD.w3_stage = at.stage;
                DD.w3_lds = at.off;
                const int inp = 16 * DD.kt_in;
                for (int o = 0; o < DD.n_out; ++o)
                    for (int k = 0; k < inp; ++k) W(o * inp + k, o, k);
                for (int o = 0; o < 4; ++o) B(DD.n_out * inp + o, o);
            } else if (DD.compact) {  // [m][r < ks][lane]
                add_chunk(P, DD, at.stage, at.off, it.kq);
                for (int m = 0; m < DD.mt; ++m)
                    for (int r = 0; r < DD.ks; ++r)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int k = k_state(r, lane >> 4), row = 16 * m + (lane & 15);
                            const int64_t q = (m * DD.ks + r) * 64 + lane;
                            if (S.fold[li] && k == 4 * DD.ks - 1) B(q, row);  // bias · state[one_slot]
                            else W(q, row, k);
                        }
            } else {  // the fragments of k-quad kq (a first Dense's k-steps beyond ks read past `in`: zeros)
                add_chunk(P, DD, at.stage, at.off, it.kq);
                if (DD.in_kind == IN_STATE) for_each_f32_frag(it.kq, it.kq + 1, DD.mt, k_state_quad, W);
                else for_each_f32_frag(it.kq, it.kq + 1, DD.mt, k_hidden_quad, W);
            }
        }
    }
    stages.close();
    auto net_stages = [&](const DevLayer& L, bool s_net, auto& push) {
        if (s_net) f32_net_stages(P, L.s_dense0, L.s_ndense, push);
        else f32_net_stages(P, L.t_dense0, L.t_ndense, push);
    };
    P.sched_fwd = stage_schedule(P.layers, true, net_stages);
    P.sched_bwd = stage_schedule(P.layers, false, net_stages);
}

// Every net reads one stage only: a stage switch then serves all of a wave's tiles.
bool nets_resident(const Plan& P) {
    bool resident = true;
    for (const DevLayer& L : P.layers) {
        if (L.kind == DF_LAYER_NORM) continue;
        for (const auto& [d0, nd] : {std::pair{L.s_dense0, L.s_ndense}, std::pair{L.t_dense0, L.t_ndense}}) {
            int st = -1;
            f32_net_stages(P, d0, nd, [&](int x) {
                if (st < 0) st = x;
                resident = resident && x == st;
            });
        }
    }
    return resident;
}

// ---------- the specialised kernel's descriptors ----------

// The compact descriptor of one net of the f32 blob; false when its layout is not the regular one.
bool make_unet(const Plan& P, int d0, int nd, UNet* u) {
    if (nd < 2) return false;
    const DevDense& D0 = P.denses[d0];
    if (D0.in_kind != IN_STATE || D0.ks > 4 || D0.mt != P.ht || D0.n_chunks != 1 || !D0.compact) return false;
    const DevChunk& C0 = P.chunks[D0.chunk0];
    u->stage = C0.stage;
    u->ks = D0.ks;
    u->nh = nd - 2;
    u->off_w0 = C0.lds_off;
    u->off_b0 = D0.bias_lds;
    u->act0 = D0.act;
    u->acth = DF_ACT_IDENTITY;
    u->hstride = P.ht * P.ht * 1024 + 64 * P.ht;
    for (int k = 1; k + 1 < nd; ++k) {
        const DevDense& D = P.denses[d0 + k];
        if (D.mt != P.ht || D.kt_in != P.ht || D.n_chunks != 1) return false;
        const DevChunk& C = P.chunks[D.chunk0];
        if (C.kq_begin != 0 || C.kq_end != P.ht) return false;
        if (k == 1) {
            u->off_h = C.lds_off;
            u->acth = D.act;
        }
        if (D.act != u->acth) return false;
        if (C.lds_off != u->off_h + (k - 1) * u->hstride) return false;
        if (D.bias_lds != C.lds_off + P.ht * P.ht * 1024) return false;
    }
    if (nd == 2) u->off_h = 0;
    const DevDense& DL = P.denses[d0 + nd - 1];
    if (DL.kt_in != P.ht) return false;
    u->n_out = DL.n_out;
    u->act_out = DL.act;
    if (DL.out_valu) {
        u->off_out = DL.w3_lds;
    } else {
        if (DL.n_chunks != 1) return false;
        const DevChunk& C = P.chunks[DL.chunk0];
        if (C.kq_begin != 0 || C.kq_end != P.ht) return false;
        u->off_out = C.lds_off;
        if (DL.bias_lds != C.lds_off + P.ht * DL.mt * 1024) return false;
    }
    return true;
}

void make_ulayers(const Shape& S, Plan& P) {
    for (const DevLayer& L : P.layers) {
        ULayer U{};
        copy_layer_header(L, U);
        if (L.kind != DF_LAYER_NORM) {
            bool ok = make_unet(P, L.t_dense0, L.t_ndense, &U.t);
            if (L.kind == DF_LAYER_RNVP) ok = ok && make_unet(P, L.s_dense0, L.s_ndense, &U.s);
            if (!ok) fail(DF_ERR_UNSUPPORTED, "internal: default-shape net with an irregular layout");
            U.s.fold0 = U.t.fold0 = S.fold[P.ulayers.size()];
        }
        P.ulayers.push_back(U);
    }
}

// Tiles of 16 samples per wave kept resident in LDS.  When every net lives
// in one stage, a stage switch serves all of a wave's tiles, so take as
// many as fit two workgroups per CU (<= 80 KiB each); otherwise one tile.
void choose_tiles(bool resident, Plan& P) {
    const int nbuf = P.stages.size() > 1 ? 2 : 1;
    const int fixed = nbuf * P.stage_max + table_lds_bytes(P);
    P.tiles = resident ? std::max(1, tiles_that_fit(fixed, tile_bytes(P), kLdsPerBlockTarget)) : 1;
    if (P.uniform) {  // the specialised kernel evaluates tiles in groups
        P.tile_group = P.fast ? kFastTileGroup : kUniformTileGroup;
        if (P.fast && P.tiles < P.tile_group) {  // not enough LDS for a FAST tile group
            P.fast = 0;
            P.tile_group = kUniformTileGroup;
        }
        if (P.tiles < P.tile_group) fail(DF_ERR_UNSUPPORTED, "LDS too small for the specialised kernel");
        P.tiles -= P.tiles % P.tile_group;
    }
    P.samples_per_block = kWavesPerBlock * 16 * P.tiles;
    if (table_lds_ints(P) > kMaxTableInts)
        fail(DF_ERR_UNSUPPORTED, params_in_lds(P) ? "chain index tables and NormalizationLayer bounds exceed 16 KiB"
                                                  : "chain index tables exceed 16 KiB");
}

// ---------- the SPLIT blob of a FAST plan ----------

// SPLIT packing of a FAST plan (layout: df_plan.h, kSplit*): every net gets the
// bf16 planes of its first and hidden Dense; nets are packed whole into stages of
// at most max(one net, 24 KiB) (a chain of <= 64 KiB is one stage).  The split
// descriptors are the FAST ones with stage ids and offsets into the split blob.
void build_split(const df_chain_desc* desc, const Shape& S, const Knobs& K, Plan& P) {
    P.split = 0;
    if (!P.fast || (P.ht != 2 && P.ht != 4)) return;
    const int ht = P.ht, H = 16 * ht;
    auto net_bytes = [&](int n_out) {
        return kSplitFirstBytes(ht) + kSplitHiddenBytes(ht) + 4 * H + round_up((n_out * H + 4) * 4, 16);
    };
    int total = 0, biggest = 0;
    for (const ULayer& U : P.ulayers) {
        if (U.kind == DF_LAYER_NORM) continue;
        const int tb = net_bytes(U.t.n_out), sb = U.kind == DF_LAYER_RNVP ? net_bytes(U.s.n_out) : 0;
        total += sb + tb;
        biggest = std::max(biggest, std::max(sb, tb));
    }
    const int cap = total <= kSingleStageCap ? kSingleStageCap : std::max(kStageCap, round_up(biggest, kStageAlign));
    StageWriter stages(P.sblob, P.sstages, &P.sstage_max, cap);
    ParamSink<uint8_t> sink(P.sblob, P.spack_dst, P.spack_src, ParamSink<uint8_t>::PLANES);
    P.sulayers = P.ulayers;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        const DevLayer& DL = P.layers[li];
        auto pack = [&](const df_dense_desc* net, int d0, UNet* u) {
            const DenseSrc W0{net[0], P.denses[d0]}, W1{net[1], P.denses[d0 + 1]}, W2{net[2], P.denses[d0 + 2]};
            const StageWriter::Slot at = stages.alloc(net_bytes(u->n_out));
            u->stage = at.stage;
            u->off_w0 = at.off;
            u->off_h = at.off + kSplitFirstBytes(ht);
            u->off_out = u->off_h + kSplitHiddenBytes(ht) + 4 * H;
            u->off_b0 = -1;
            u->hstride = 0;
            // the kernel derives both from off_w0
            if (u->off_h != u->off_w0 + kSplitOffH(ht) || u->off_out != u->off_w0 + kSplitOffOut(ht))
                fail(DF_ERR_INVALID, "internal: SPLIT net layout differs from kSplitOffH / kSplitOffOut");
            // first Dense: slots (w0, w0, w1, w0, w1, w2, 0, 0) of W[16m+i, g] (g = 3 folded: the bias)
            static const int kPlaneOfSlot[6] = {0, 0, 1, 0, 1, 2};
            for (int m = 0; m < ht; ++m)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, row = 16 * m + (lane & 15);
                    const Param w = (S.fold[li] && g == 3) ? W0.b(row) : W0.W(row, g);
                    for (int e = 0; e < 6; ++e)
                        sink.plane(at.at + ((int64_t)m * 64 + lane) * 16 + 2 * e, kPlaneOfSlot[e], w);
                }
            // hidden Dense: planes, then the f32 bias
            const int64_t stage0 = at.at - at.off;  // the stage in the blob
            const int64_t hidden = stage0 + u->off_h;
            for_each_plane_frag(0, ht / 2, 0, ht, k_plane_hidden, [&](int64_t pos, int row, int k, int p) {
                sink.plane(hidden + pos, p, W1.W(row, k));
            });
            for (int row = 0; row < H; ++row) sink.f32(hidden + kSplitHiddenBytes(ht) + 4 * row, W1.b(row));
            // output Dense (VALU GEMV): [o][H] then b[4]
            const int64_t out = stage0 + u->off_out;
            const int n_out = net[2].out_dim;
            for (int o = 0; o < n_out; ++o)
                for (int k = 0; k < H; ++k) sink.f32(out + 4 * ((int64_t)o * H + k), W2.W(o, k));
            for (int o = 0; o < 4; ++o) sink.f32(out + 4 * ((int64_t)n_out * H + o), W2.b(o));
            P.split_flops_per_sample += 2.0 * (net[0].in_dim * net[0].out_dim + net[1].in_dim * net[1].out_dim);
        };
        ULayer& U = P.sulayers[li];
        if (L.kind == DF_LAYER_RNVP) pack(L.s_net, DL.s_dense0, &U.s);
        pack(L.t_net, DL.t_dense0, &U.t);
        // what the kernel no longer loads: the slot words (df_plan.h) stand for the
        // layer's table entries, and a net's hidden and output Dense follow from off_w0
        for (int g = 0; g < 4; ++g) {
            const int32_t f = P.tables[U.feat_tab + g], a = P.tables[U.af_tab + (g < U.n_af ? g : 0)];
            if (f < 0 || f >= (1 << kSplitSlotBits) || a < 0 || a >= (1 << kSplitSlotBits))
                fail(DF_ERR_UNSUPPORTED, "SPLIT plan: a state slot does not fit the 8 bits of a slot word");
        }
        U.feat_word = split_feat_word(P.tables.data(), U);
        U.af_word = split_af_word(P.tables.data(), U);
    }
    stages.close();
    auto net_stages = [](const ULayer& U, bool s_net, auto& push) { push(s_net ? U.s.stage : U.t.stage); };
    P.ssched_fwd = stage_schedule(P.sulayers, true, net_stages);
    P.ssched_bwd = stage_schedule(P.sulayers, false, net_stages);
    const int nbuf = P.sstages.size() > 1 ? 2 : 1;
    const int target = K.split_lds_bytes ? K.split_lds_bytes : kLdsPerBlockTarget;
    int t = tiles_that_fit(nbuf * P.sstage_max + table_lds_bytes(P), tile_bytes(P), target);
    t -= t % P.tile_group;
    if (t < P.tile_group) {  // no room for one tile group next to the split stages: stay on f32
        P.sulayers.clear();
        P.sstages.clear();
        P.sblob.clear();
        P.spack_dst.clear();
        P.spack_src.clear();
        P.split_flops_per_sample = 0.0;
        return;
    }
    P.stiles = t;
    P.sblob.resize(round_up((int)P.sblob.size(), 16) + 16, 0);
    P.split = 1;
}

// ---------- the wide blobs ----------

bool wide_shape(const df_chain_desc* desc) {
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        bool ok = true;
        for_each_net(L, [&](const df_dense_desc* net, int nd) {
            ok = ok && nd == 3 && net[0].in_dim <= kMaxState && net[0].out_dim == 256 && net[1].out_dim == 256 &&
                 net[2].out_dim <= 32 && net[0].act == DF_ACT_RELU && net[1].act == DF_ACT_RELU &&
                 net[2].act == DF_ACT_IDENTITY;
        });
        if (!ok) return false;
    }
    return true;
}

// Wide-net packing (see WNet).  Leaves P.wide = 0 unless every coupling layer's
// conditioners are Dense(in <= 64, 256) → Dense(256, 256) → Dense(256, out <= 32).
void build_wide(const df_chain_desc* desc, const Knobs& K, Plan& P) {
    if (K.no_wide || P.uniform || P.ht != 16 || !wide_shape(desc)) return;
    StageWriter stages(P.wblob, P.wstages);
    ParamSink<uint8_t> sink(P.wblob, P.wpack_dst, P.wpack_src, ParamSink<uint8_t>::WORDS);
    ParamSink<float> bias_sink(P.wbias, P.wbias_dst, P.wbias_src, ParamSink<float>::WORDS);
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        const DevLayer& DL = P.layers[li];
        WLayer W{};
        copy_layer_header(DL, W);
        auto pack = [&](const df_dense_desc* net, int d0, WNet& N) {
            const DenseSrc D[3] = {{net[0], P.denses[d0]}, {net[1], P.denses[d0 + 1]}, {net[2], P.denses[d0 + 2]}};
            const int ks = (net[0].in_dim + 3) / 4;  // state k-steps: feature k = 4s + g
            const int nkq0 = (ks + 3) / 4;
            N.stage0 = (int)P.wstages.size();
            N.nst0 = (nkq0 + 1) / 2;
            N.ks = ks;
            N.n_out = net[2].out_dim;
            N.mto = (N.n_out + 15) / 16;
            N.act0 = net[0].act;
            N.act1 = net[1].act;
            N.act_out = net[2].act;
            // k-quads [kq0, kq1) of a Dense as one stage of `bytes`
            auto stage = [&](int bytes, const DenseSrc& src, int kq0, int kq1, int mt, auto k_of) {
                const int64_t base = stages.fixed_stage(bytes);
                for_each_f32_frag(kq0, kq1, mt, k_of,
                                  [&](int64_t q, int row, int k) { sink.f32(base + 4 * q, src.W(row, k)); });
            };
            // first Dense: [kk < 2][m < 16], k-steps beyond ks read past `in` (zeros)
            for (int st = 0; st < N.nst0; ++st) stage(kWideStageBytes, D[0], 2 * st, 2 * st + 2, 16, k_state_quad);
            // hidden Dense: 8 stages of [kk < 2][m < 16]
            for (int st = 0; st < 8; ++st) stage(kWideStageBytes, D[1], 2 * st, 2 * st + 2, 16, k_hidden_quad);
            // output Dense: [kq < 16][m < mto]
            stage(16 * N.mto * 1024, D[2], 0, 16, N.mto, k_hidden_quad);
            // every wide Dense gets a bias row (zeros without a bias: the kernel adds it
            // unconditionally, no per-element select; x + 0 = x up to the sign of a zero)
            auto bias = [&](const DenseSrc& src, int rows) -> int32_t {
                const int32_t off = (int32_t)P.wbias.size();
                P.wbias.resize(P.wbias.size() + rows, 0.f);
                for (int r = 0; r < rows; ++r) bias_sink.f32(4 * (int64_t)(off + r), src.b(r));
                return off;
            };
            N.b0 = bias(D[0], 256);
            N.b1 = bias(D[1], 256);
            N.bo = bias(D[2], 16 * N.mto);
        };
        if (L.kind == DF_LAYER_RNVP) pack(L.s_net, DL.s_dense0, W.s);
        if (L.kind != DF_LAYER_NORM) pack(L.t_net, DL.t_dense0, W.t);
        P.wlayers.push_back(W);
    }
    auto net_stages = [](const WLayer& L, bool s_net, auto& push) {
        const WNet& N = s_net ? L.s : L.t;
        for (int s = 0; s < N.nst0 + 9; ++s) push(N.stage0 + s);
    };
    P.wsched_fwd = stage_schedule(P.wlayers, true, net_stages);
    P.wsched_bwd = stage_schedule(P.wlayers, false, net_stages);
    P.wblob.resize(P.wblob.size() + 16, 0);
    P.wbias.resize(P.wbias.size() + 4, 0.f);
    P.wide = 1;
}

// SPLIT packing of a wide plan (see Plan::wsplit): per net, ceil(in/32) first-Dense
// stages, 8 hidden stages, one output stage, each chunk [m][plane][lane][8 bf16]
// with lane (g, i) holding W[16m + i, k(e)], e < 8:
//   first Dense  k_plane_first (features through the layer's split table)
//   hidden/out   k_plane_hidden (accumulator tiles 2c, 2c+1)
void build_wide_split(const df_chain_desc* desc, Plan& P) {
    P.wsplit = 0;
    if (!P.wide) return;
    P.wstables = P.tables;
    P.wslayers = P.wlayers;
    StageWriter stages(P.wsblob, P.wsstages);
    ParamSink<uint8_t> sink(P.wsblob, P.wspack_dst, P.wspack_src, ParamSink<uint8_t>::PLANES);
    const int zero_slot = P.n + P.d;
    for (int li = 0; li < desc->n_layers; ++li) {
        const df_layer_desc& L = desc->layers[li];
        if (L.kind == DF_LAYER_NORM) continue;
        const DevLayer& DL = P.layers[li];
        WLayer& W = P.wslayers[li];
        const int nc0 = (L.n_nn + 31) / 32;
        W.pad0 = (int32_t)P.wstables.size();
        for (int k = 0; k < 32 * nc0; ++k) P.wstables.push_back(k < L.n_nn ? L.axis_nn[k] - 1 : zero_slot);
        auto pack = [&](const df_dense_desc* net, int d0, WNet& N) {
            const DenseSrc D[3] = {{net[0], P.denses[d0]}, {net[1], P.denses[d0 + 1]}, {net[2], P.denses[d0 + 2]}};
            N.stage0 = (int)P.wsstages.size();
            N.nst0 = nc0 * kWideSplitHalves;
            N.nso = (kWideSplitHalves == 2 && N.mto == 2) ? 2 : 1;
            // chunks [c0, c1) of m-tiles m0 .. m0 + mt of a Dense as one stage of `bytes`
            auto stage = [&](int bytes, const DenseSrc& src, int c0, int c1, int m0, int mt, auto k_of) {
                const int64_t base = stages.fixed_stage(bytes);
                for_each_plane_frag(c0, c1, m0, mt, k_of, [&](int64_t pos, int row, int k, int p) {
                    sink.plane(base + pos, p, src.W(row, k));
                });
            };
            constexpr int MH = 16 / kWideSplitHalves;  // m-tiles per stage
            for (int c = 0; c < nc0; ++c)
                for (int hv = 0; hv < kWideSplitHalves; ++hv)
                    stage(kWideSplitStageBytes, D[0], c, c + 1, MH * hv, MH, k_plane_first);
            for (int c = 0; c < 8; ++c)
                for (int hv = 0; hv < kWideSplitHalves; ++hv)
                    stage(kWideSplitStageBytes, D[1], c, c + 1, MH * hv, MH, k_plane_hidden);
            const int cps = 8 / N.nso;  // output chunks per stage
            for (int so = 0; so < N.nso; ++so)
                stage(cps * N.mto * 3 * 1024, D[2], so * cps, (so + 1) * cps, 0, N.mto, k_plane_hidden);
            P.split_flops_per_sample += 2.0 * ((double)net[0].in_dim * net[0].out_dim +
                                               (double)net[1].in_dim * net[1].out_dim +
                                               (double)net[2].in_dim * net[2].out_dim);
        };
        if (L.kind == DF_LAYER_RNVP) pack(L.s_net, DL.s_dense0, W.s);
        pack(L.t_net, DL.t_dense0, W.t);
    }
    auto net_stages = [](const WLayer& L, bool s_net, auto& push) {
        const WNet& N = s_net ? L.s : L.t;
        for (int s = 0; s < N.nst0 + 8 * kWideSplitHalves + N.nso; ++s) push(N.stage0 + s);
    };
    P.wssched_fwd = stage_schedule(P.wslayers, true, net_stages);
    P.wssched_bwd = stage_schedule(P.wslayers, false, net_stages);
    P.wsblob.resize(P.wsblob.size() + 16, 0);
    P.wsplit = 1;
}

// floats per sample row of the LDS state tile: [θ | z | 0 | ldj_chain | ldj_elem], then a
// column that holds 1 when a first-Dense bias is folded; odd, to spread LDS banks
int state_stride(int n, int d, bool any_fold) {
    const int s = n + d + (any_fold ? 4 : 3);
    return s % 2 == 0 ? s + 1 : s;
}

}  // namespace

size_t plan_lds_bytes(const Plan& p) {
    size_t tab = (size_t)table_lds_bytes(p);
    const int nbuf = p.stages.size() > 1 ? 2 : 1;
    return (size_t)nbuf * p.stage_max + tab + (size_t)p.samples_per_block * p.stride * 4;
}

int build_plan(const df_chain_desc* desc, Plan* out, std::string* err, int exact) {
    try {
        if (!desc || !out) fail(DF_ERR_INVALID, "null descriptor");
        const Knobs K;
        validate(desc);
        const Shape S = analyse_shape(desc, K);

        Plan P;
        P.d = desc->d;
        P.n = desc->n;
        P.n_layers = desc->n_layers;
        P.outv = S.all_valu ? 1 : 0;
        P.ht = S.ht;
        P.stride = state_stride(P.n, P.d, S.any_fold);
        describe_layers(desc, S, P);
        pack_f32(desc, S, K, P);

        // Specialised-kernel descriptors when every net has the default shape.
        const bool resident = nets_resident(P);
        P.uniform = (S.uniform_shape && resident) ? 1 : 0;
        P.relu_only = (P.uniform && S.relu_only) ? 1 : 0;
        P.fast = (P.relu_only && S.fast_shape && !K.no_fast) ? 1 : 0;
        if (S.uniform_shape && !resident) fail(DF_ERR_UNSUPPORTED, "internal: default-shape net split across stages");
        if (P.uniform) make_ulayers(S, P);
        choose_tiles(resident, P);
        P.blob.resize(round_up((int)P.blob.size(), 16) + 16, 0);

        if (exact < 0) exact = K.f32_exact ? 1 : 0;
        if (!exact) build_split(desc, S, K, P);
        build_wide(desc, K, P);
        if (!exact) build_wide_split(desc, P);
        *out = std::move(P);
        return DF_OK;
    } catch (const Fail& f) {
        if (err) *err = f.msg;
        return f.code;
    } catch (const std::exception& e) {
        if (err) *err = e.what();
        return DF_ERR_INVALID;
    }
}

}  // namespace df
