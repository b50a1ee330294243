// Fingerprint of the planner's output (tests/test_plan_fingerprint.py compiles this file
// with df_plan.cpp under -fsanitize=address,undefined and runs it as a child process; no
// GPU, nothing loaded into Python).
//
//   plan_fingerprint [--time N] <descriptor file> <exact: -1 | 0 | 1>
//
// The descriptor file is a stream of little-endian 32-bit words (floats as their bits):
//   abi d n n_layers, then per layer
//     kind element
//     NORM:     alpha beta x_min[d] x_max[d]
//     coupling: n_af axis_af[n_af] n_nn axis_nn[n_nn] n_dense_s dense... n_dense_t dense...
//     dense:    in out act has_bias W[in*out] (b[out] when has_bias)
// A failing plan prints its status and message.  A plan prints every scalar of df::Plan
// and, for every vector of it, the length and the 64-bit FNV-1a hash of its bytes (struct
// vectors as raw bytes: the planner zero-initialises them).  --time N: N calls of
// build_plan, the median wall time in microseconds, and no fingerprint.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "df_plan.h"

namespace {

struct Desc {
    std::vector<uint32_t> words;
    size_t at = 0;
    std::deque<std::vector<df_dense_desc>> nets;
    std::vector<df_layer_desc> layers;
    df_chain_desc chain{};

    uint32_t u() {
        if (at >= words.size()) {
            std::fprintf(stderr, "descriptor file ends early\n");
            std::exit(2);
        }
        return words[at++];
    }
    int32_t i() { return (int32_t)u(); }
    float f() {
        const uint32_t v = u();
        float r;
        std::memcpy(&r, &v, 4);
        return r;
    }
    // n words in place (the vector is not resized after load)
    const void* span(size_t n) {
        if (at + n > words.size()) {
            std::fprintf(stderr, "descriptor file ends early\n");
            std::exit(2);
        }
        const void* p = words.data() + at;
        at += n;
        return p;
    }
    const df_dense_desc* net(int nd) {
        nets.emplace_back();
        std::vector<df_dense_desc>& N = nets.back();
        for (int k = 0; k < nd; ++k) {
            df_dense_desc D{};
            D.in_dim = i();
            D.out_dim = i();
            D.act = i();
            const int has_bias = i();
            D.W = static_cast<const float*>(span((size_t)D.in_dim * D.out_dim));
            D.b = has_bias ? static_cast<const float*>(span((size_t)D.out_dim)) : nullptr;
            N.push_back(D);
        }
        return N.data();
    }
    void parse() {
        chain.abi_version = i();
        chain.d = i();
        chain.n = i();
        chain.n_layers = i();
        for (int li = 0; li < chain.n_layers; ++li) {
            df_layer_desc L{};
            L.kind = i();
            L.element = i();
            if (L.kind == DF_LAYER_NORM) {
                L.alpha = f();
                L.beta = f();
                L.x_min = static_cast<const float*>(span((size_t)chain.d));
                L.x_max = static_cast<const float*>(span((size_t)chain.d));
            } else {
                L.n_af = i();
                L.axis_af = static_cast<const int32_t*>(span((size_t)L.n_af));
                L.n_nn = i();
                L.axis_nn = static_cast<const int32_t*>(span((size_t)L.n_nn));
                L.n_dense_s = i();
                L.s_net = L.n_dense_s ? net(L.n_dense_s) : nullptr;
                L.n_dense_t = i();
                L.t_net = L.n_dense_t ? net(L.n_dense_t) : nullptr;
            }
            layers.push_back(L);
        }
        chain.layers = layers.data();
    }
};

bool load(const char* path, Desc& D) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    std::fseek(fp, 0, SEEK_END);
    const long n = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    D.words.resize((size_t)n / 4);
    const size_t got = std::fread(D.words.data(), 4, D.words.size(), fp);
    std::fclose(fp);
    if (got != D.words.size()) return false;
    D.parse();
    return true;
}

template <class T>
void vec(const char* name, const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t q = 0; q < v.size() * sizeof(T); ++q) h = (h ^ p[q]) * 0x100000001b3ull;
    std::printf("%s %zu %016llx\n", name, v.size(), (unsigned long long)h);
}

void print(const df::Plan& P) {
#define S(x) std::printf(#x " %lld\n", (long long)P.x)
#define V(x) vec(#x, P.x)
    S(d); S(n); S(n_layers); S(stride); S(ht); S(tiles); S(outv); S(uniform); S(relu_only); S(tile_group); S(fast);
    S(samples_per_block); S(stage_max); S(n_params); S(wide); S(split); S(stiles); S(sstage_max); S(wsplit);
    std::printf("flops_per_sample %.17g\n", P.flops_per_sample);
    std::printf("split_flops_per_sample %.17g\n", P.split_flops_per_sample);
    std::printf("plan_lds_bytes %zu\n", df::plan_lds_bytes(P));
    V(ulayers); V(sched_fwd); V(sched_bwd); V(layers); V(denses); V(chunks); V(stages); V(blob); V(tables); V(params);
    V(trainables); V(pack_dst); V(pack_src);
    V(wlayers); V(wstages); V(wblob); V(wbias); V(wsched_fwd); V(wsched_bwd); V(wpack_dst); V(wpack_src);
    V(wbias_dst); V(wbias_src);
    V(sulayers); V(sstages); V(sblob); V(ssched_fwd); V(ssched_bwd); V(spack_dst); V(spack_src);
    V(wslayers); V(wsstages); V(wsblob); V(wssched_fwd); V(wssched_bwd); V(wspack_dst); V(wspack_src); V(wstables);
#undef S
#undef V
}

}  // namespace

int main(int argc, char** argv) {
    int times = 0, a = 1;
    if (argc > 2 && std::strcmp(argv[1], "--time") == 0) {
        times = std::atoi(argv[2]);
        a = 3;
    }
    if (argc != a + 2) {
        std::fprintf(stderr, "usage: %s [--time N] <descriptor file> <exact: -1 | 0 | 1>\n", argv[0]);
        return 2;
    }
    Desc D;
    if (!load(argv[a], D)) {
        std::fprintf(stderr, "cannot read %s\n", argv[a]);
        return 2;
    }
    const int exact = std::atoi(argv[a + 1]);
    if (times > 0) {
        std::vector<double> us;
        for (int r = 0; r < times; ++r) {
            df::Plan P;
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = df::build_plan(&D.chain, &P, &err, exact);
            const auto t1 = std::chrono::steady_clock::now();
            if (rc != DF_OK) {
                std::printf("status %d %s\n", rc, err.c_str());
                return 1;
            }
            us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("median_us %.1f min_us %.1f max_us %.1f calls %d\n", us[us.size() / 2], us.front(), us.back(), times);
        return 0;
    }
    df::Plan P;
    std::string err;
    const int rc = df::build_plan(&D.chain, &P, &err, exact);
    std::printf("status %d %s\n", rc, err.c_str());
    if (rc == DF_OK) print(P);
    return 0;
}
