// The chain descriptor file of the planner fingerprints (tests/plan_fingerprint.cpp and
// tests/train_plan_fingerprint.cpp), and the hash both print a vector with.
//
// The descriptor file is a stream of little-endian 32-bit words (floats as their bits):
//   abi d n n_layers, then per layer
//     kind element
//     NORM:     alpha beta x_min[d] x_max[d]
//     coupling: n_af axis_af[n_af] n_nn axis_nn[n_nn] n_dense_s dense... n_dense_t dense...
//     dense:    in out act has_bias W[in*out] (b[out] when has_bias)
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
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

}  // namespace
