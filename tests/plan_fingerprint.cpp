// Fingerprint of the planner's output (tests/test_plan_fingerprint.py compiles this file
// with df_plan.cpp under -fsanitize=address,undefined and runs it as a child process; no
// GPU, nothing loaded into Python).
//
//   plan_fingerprint [--time N] <descriptor file> <exact: -1 | 0 | 1>
//
// The descriptor file: tests/plan_desc.h.
// A failing plan prints its status and message.  A plan prints every scalar of df::Plan
// and, for every vector of it, the length and the 64-bit FNV-1a hash of its bytes (struct
// vectors as raw bytes: the planner zero-initialises them).  --time N: N calls of
// build_plan, the median wall time in microseconds, and no fingerprint.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "df_plan.h"
#include "plan_desc.h"

namespace {

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
