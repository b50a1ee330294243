// Host check of what the specialised SPLIT kernel no longer loads in a net body
// (tests/test_split_head_words.py compiles this file with df_plan.cpp under
// -fsanitize=address,undefined and runs it; no GPU, nothing loaded into Python).
//
//   split_head_words_check "name;d;n;hidden;rnvp:1,2,3;+rnvp:4,5;norm;nice:2,1" ...
//
// Every argument is a model: its dimensions and its layers (kind:mask, the mask being the
// transformed dims, 1-based, in the given order; "+" keeps the layer in the FlowElement
// of the one before, as a CouplingBlock does; weights are arbitrary, the plan's structure
// does not depend on them).  For every model the planner must produce a SPLIT plan, and
// for every coupling layer of it
//   * ULayer::feat_word decodes, for lane group g = 0..3, to tables[feat_tab + g];
//   * ULayer::af_word decodes to tables[af_tab + (g < n_out ? g : 0)], the index the
//     kernel formed from the net's output count (n_out == n_af for both nets);
//   * UNet::off_h / off_out equal off_w0 + kSplitOffH / kSplitOffOut.
// Prints, per model, the resident tiles and the stage and offset of every net in forward
// order, then both schedules; exit status 1 on any mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "df_plan.h"

namespace {

struct Net {
    std::vector<std::vector<float>> W, b;
    std::vector<df_dense_desc> dense;
};

struct Model {
    std::string name;
    int d = 0, n = 0, hidden = 0;
    std::vector<df_layer_desc> layers;
    std::vector<std::unique_ptr<std::vector<int32_t>>> ints;
    std::vector<std::unique_ptr<std::vector<float>>> floats;
    std::vector<std::unique_ptr<Net>> nets;
};

float value(unsigned& seed) {  // small deterministic weights
    seed = seed * 1664525u + 1013904223u;
    return ((float)((seed >> 8) & 0xffff) / 65536.f - 0.5f) * 0.2f;
}

const df_dense_desc* make_net(Model& M, int in, int hidden, int out, unsigned& seed) {
    M.nets.push_back(std::make_unique<Net>());
    Net& N = *M.nets.back();
    const int dims[4] = {in, hidden, hidden, out};
    for (int k = 0; k < 3; ++k) {
        N.W.emplace_back((size_t)dims[k] * dims[k + 1]);
        N.b.emplace_back((size_t)dims[k + 1]);
        for (float& v : N.W.back()) v = value(seed);
        for (float& v : N.b.back()) v = value(seed);
    }
    for (int k = 0; k < 3; ++k)
        N.dense.push_back(df_dense_desc{dims[k], dims[k + 1], k < 2 ? DF_ACT_RELU : DF_ACT_IDENTITY, N.W[k].data(),
                                        N.b[k].data()});
    return N.dense.data();
}

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, sep)) out.push_back(item);
    return out;
}

bool parse(const std::string& arg, Model& M) {
    const std::vector<std::string> f = split(arg, ';');
    if (f.size() < 5) return false;
    M.name = f[0];
    M.d = std::atoi(f[1].c_str());
    M.n = std::atoi(f[2].c_str());
    M.hidden = std::atoi(f[3].c_str());
    unsigned seed = 12345u;
    int element = -1;
    for (size_t i = 4; i < f.size(); ++i) {
        std::string tok = f[i];
        const bool same = !tok.empty() && tok[0] == '+';
        if (same) tok = tok.substr(1);
        if (!same) ++element;
        df_layer_desc L{};
        L.element = element;
        if (tok == "norm") {
            L.kind = DF_LAYER_NORM;
            M.floats.push_back(std::make_unique<std::vector<float>>((size_t)M.d, -2.f));
            L.x_min = M.floats.back()->data();
            M.floats.push_back(std::make_unique<std::vector<float>>((size_t)M.d, 3.f));
            L.x_max = M.floats.back()->data();
            L.alpha = -1.f;
            L.beta = 1.f;
            M.layers.push_back(L);
            continue;
        }
        const std::vector<std::string> km = split(tok, ':');
        if (km.size() != 2 || (km[0] != "rnvp" && km[0] != "nice")) return false;
        L.kind = km[0] == "rnvp" ? DF_LAYER_RNVP : DF_LAYER_NICE;
        auto af = std::make_unique<std::vector<int32_t>>();
        for (const std::string& v : split(km[1], ',')) af->push_back(std::atoi(v.c_str()));
        auto nn = std::make_unique<std::vector<int32_t>>();
        for (int c = 1; c <= M.n; ++c) nn->push_back(c);  // vcat(θ, z): θ first, then the untouched dims, sorted
        for (int c = 1; c <= M.d; ++c) {
            bool masked = false;
            for (int32_t m : *af) masked = masked || m == c;
            if (!masked) nn->push_back(c + M.n);
        }
        L.n_af = (int32_t)af->size();
        L.axis_af = af->data();
        L.n_nn = (int32_t)nn->size();
        L.axis_nn = nn->data();
        if (L.kind == DF_LAYER_RNVP) {
            L.n_dense_s = 3;
            L.s_net = make_net(M, L.n_nn, M.hidden, L.n_af, seed);
        }
        L.n_dense_t = 3;
        L.t_net = make_net(M, L.n_nn, M.hidden, L.n_af, seed);
        M.ints.push_back(std::move(af));
        M.ints.push_back(std::move(nn));
        M.layers.push_back(L);
    }
    return !M.layers.empty();
}

int check(const Model& M) {
    df_chain_desc desc{};
    desc.abi_version = DF_ABI_VERSION;
    desc.d = M.d;
    desc.n = M.n;
    desc.n_layers = (int32_t)M.layers.size();
    desc.layers = M.layers.data();
    df::Plan P;
    std::string err;
    const int rc = df::build_plan(&desc, &P, &err, 0);
    if (rc != DF_OK) {
        std::printf("model %s: build_plan failed (%d): %s\n", M.name.c_str(), rc, err.c_str());
        return 1;
    }
    if (!P.split || !P.fast || P.sulayers.size() != M.layers.size()) {
        std::printf("model %s: no SPLIT plan (split %d fast %d)\n", M.name.c_str(), P.split, P.fast);
        return 1;
    }
    int bad = 0;
    std::printf("model %s ht %d stiles %d stages %d stride %d\n", M.name.c_str(), P.ht, P.stiles, (int)P.sstages.size(),
                P.stride);
    for (size_t li = 0; li < P.sulayers.size(); ++li) {
        const df::ULayer& U = P.sulayers[li];
        if (U.kind == DF_LAYER_NORM) continue;
        const uint32_t fw = (uint32_t)U.feat_word, aw = (uint32_t)U.af_word;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 0 && U.kind != DF_LAYER_RNVP) continue;
            const df::UNet& N = pass == 0 ? U.s : U.t;
            const char* which = pass == 0 ? "s" : "t";
            std::printf("net %s layer %d %s stage %d off %d n_out %d\n", M.name.c_str(), (int)li, which, N.stage,
                        N.off_w0, N.n_out);
            if (N.n_out != U.n_af || N.n_out < 1 || N.n_out > 4) {
                std::printf("  MISMATCH n_out %d n_af %d\n", N.n_out, U.n_af);
                ++bad;
            }
            for (int g = 0; g < 4; ++g) {  // as net_tiles indexed the tables: feat[g], af[g < NO ? g : 0]
                const int32_t slot = P.tables[U.feat_tab + g];
                const int32_t aslot = P.tables[U.af_tab + (g < N.n_out ? g : 0)];
                const int32_t got_f = (int32_t)((fw >> (df::kSplitSlotBits * g)) & 0xffu);
                const int32_t got_a = (int32_t)((aw >> (df::kSplitSlotBits * g)) & 0xffu);
                if (got_f != slot || got_a != aslot || slot < 0 || slot >= P.stride || aslot < 0 || aslot >= P.stride) {
                    std::printf("  MISMATCH layer %d %s g %d: feat %d (table %d) af %d (table %d) stride %d\n", (int)li,
                                which, g, got_f, slot, got_a, aslot, P.stride);
                    ++bad;
                }
            }
            if (N.off_h != N.off_w0 + df::kSplitOffH(P.ht) || N.off_out != N.off_w0 + df::kSplitOffOut(P.ht)) {
                std::printf("  MISMATCH layer %d %s: off_w0 %d off_h %d off_out %d\n", (int)li, which, N.off_w0, N.off_h,
                            N.off_out);
                ++bad;
            }
            const int end = N.off_out + (N.n_out * 16 * P.ht + 4) * 4;
            if (N.stage < 0 || N.stage >= (int)P.sstages.size() || end > P.sstages[N.stage].bytes) {
                std::printf("  MISMATCH layer %d %s: net ends at %d past its stage\n", (int)li, which, end);
                ++bad;
            }
        }
    }
    for (int fwd = 1; fwd >= 0; --fwd) {
        std::printf("sched %s %s", M.name.c_str(), fwd ? "fwd" : "bwd");
        for (int32_t s : fwd ? P.ssched_fwd : P.ssched_bwd) std::printf(" %d", s);
        std::printf("\n");
    }
    // the exact-f32 descriptors carry no slot words: the other kernels read their tables
    for (const df::ULayer& U : P.ulayers)
        if (U.feat_word != 0 || U.af_word != 0) {
            std::printf("  MISMATCH: an exact-f32 ULayer carries slot words\n");
            ++bad;
        }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s \"name;d;n;hidden;kind:mask;...\" ...\n", argv[0]);
        return 2;
    }
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        Model M;
        if (!parse(argv[i], M)) {
            std::fprintf(stderr, "cannot parse %s\n", argv[i]);
            return 2;
        }
        bad += check(M);
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
