// Fingerprint of the trainer's host plan (tests/test_train_plan_fingerprint.py compiles this
// file with df_plan.cpp and df_train_plan.cpp under -fsanitize=address,undefined and runs it
// as a child process; no GPU, nothing loaded into Python).
//
//   train_plan_fingerprint [--time N] <descriptor file> <exact: -1 | 0 | 1> <sweep> <rules>
//
// The descriptor file: tests/plan_desc.h.  exact -1: DF_F32_EXACT, as df_chain_create reads
// it (and DF_NO_WIDE).  sweep: the int df_train_create_opt takes.  rules: "-" for none, else
// kind:p0,p1,p2,p3 per rule, joined with '/'.
// Prints the status and message, and for a plan every scalar of df::TrainPlan, the length
// and FNV-1a hash of every vector of it, every GNet, every Dense of lnets with both LOps,
// and the repack table's sources.  --time N: N calls of build_train_plan, the median wall
// time in microseconds, and no fingerprint.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "df_plan.h"
#include "plan_desc.h"
#ifndef DF_TRAIN_PLAN_GIVEN  // (the recorder of the golden file gave TrainPlan from the code before it existed)
#include "df_train_plan.h"
#endif

namespace {

void unet(const char* name, const df::UNet& u) {
    std::printf(" %s %d %d %d %d %d %d %d %d %d %d %d %d %d", name, u.stage, u.ks, u.nh, u.n_out, u.off_w0, u.off_b0,
                u.off_h, u.hstride, u.off_out, u.act0, u.acth, u.act_out, u.fold0);
}

void lop(const char* name, const df::LOp& o) {
    std::printf(" %s %d %d %d %lld %lld %lld", name, o.mt, o.nkq, o.chunk_kq, (long long)o.frag, (long long)o.bias,
                (long long)o.sfrag);
}

void print(const df::Plan& P, const df::TrainPlan& T) {
#define S(x) std::printf(#x " %lld\n", (long long)T.x)
#define V(x) vec(#x, T.x)
    S(n_params); S(amode); S(layerwise); S(sweep_req); S(separate); S(lwidth); S(lmax_h); S(any_pre); S(fmode);
    S(chain_mode); S(och_clip); S(och_eta);
    std::printf("adam %.9g %.9g %.9g %.9g\n", T.adam.eta, T.adam.beta1, T.adam.beta2, T.adam.epsilon);
    std::printf("och %d\n", T.och.n);
    for (int r = 0; r < df::kOptMaxRules; ++r)
        std::printf("rule %d kind %d p %.9g %.9g %.9g %.9g\n", r, T.och.kind[r], T.och.p[r][0], T.och.p[r][1],
                    T.och.p[r][2], T.och.p[r][3]);
    V(toff); V(net_nh); V(ops); V(tblob); V(tdst); V(tsrc); V(tsblob); V(tsdst); V(tssrc);
    V(lblob); V(ldst); V(lsrc); V(lsblob); V(lsdst); V(lssrc); V(oblocks);
#undef S
#undef V
    std::printf("nets %zu\n", T.nets.size());
    for (const df::GNet& g : T.nets) {
        std::printf("net %d %d %d %d %d %d %lld %lld %d %d w %d %d %d b %d %d %d split %d %d %lld %d %lld", g.n_in,
                    g.h_true, g.off_w0t, g.off_ht, g.fwd_bytes, g.t_bytes, (long long)g.fwd_src, (long long)g.t_src,
                    g.p_begin, g.p_count, g.w_off[0], g.w_off[1], g.w_off[2], g.b_off[0], g.b_off[1], g.b_off[2],
                    g.split, g.sfwd_bytes, (long long)g.sfwd_src, g.st_bytes, (long long)g.st_src);
        unet("u", g.u);
        unet("su", g.su);
        std::printf("\n");
    }
    std::printf("lnets %zu\n", T.lnets.size());
    for (const df::LNet& N : T.lnets) {
        std::printf("lnet pre %d denses %zu\n", (int)N.pre, N.dn.size());
        for (const df::LDense& D : N.dn) {
            std::printf("dense %d %d %d %d %d", D.in_dim, D.out_dim, D.act, D.w_off, D.b_off);
            lop("fwd", D.fwd);
            lop("bwd", D.bwd);
            std::printf("\n");
        }
    }
    int i = 0;
    for (const df::MapSrc& m : T.map_sources(P)) {
        std::printf("map %d on %d split %d n %zu\n", i++, (int)m.on, (int)m.split, m.on ? m.dst->size() : (size_t)0);
        vec(" dst", *m.dst);
        vec(" src", *m.src);
    }
}

std::vector<df_opt_rule> parse_rules(const char* s) {
    std::vector<df_opt_rule> rules;
    if (std::strcmp(s, "-") == 0) return rules;
    while (*s) {
        df_opt_rule r{};
        char* end = nullptr;
        r.kind = (int)std::strtol(s, &end, 10);
        for (int k = 0; k < 4 && (*end == ':' || *end == ','); ++k) r.p[k] = std::strtof(end + 1, &end);
        rules.push_back(r);
        s = *end == '/' ? end + 1 : end;
        if (*end && *end != '/') {
            std::fprintf(stderr, "cannot read the rules at '%s'\n", end);
            std::exit(2);
        }
    }
    return rules;
}

bool env_is_1(const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
}

}  // namespace

int main(int argc, char** argv) {
    int times = 0, a = 1;
    if (argc > 2 && std::strcmp(argv[1], "--time") == 0) {
        times = std::atoi(argv[2]);
        a = 3;
    }
    if (argc != a + 4) {
        std::fprintf(stderr, "usage: %s [--time N] <descriptor file> <exact: -1 | 0 | 1> <sweep> <rules>\n", argv[0]);
        return 2;
    }
    Desc D;
    if (!load(argv[a], D)) {
        std::fprintf(stderr, "cannot read %s\n", argv[a]);
        return 2;
    }
    const int ex = std::atoi(argv[a + 1]);
    df::TrainPlanOpts o;
    o.exact = ex < 0 ? env_is_1("DF_F32_EXACT") : ex == 1;
    o.no_wide = env_is_1("DF_NO_WIDE");
    o.sweep = std::atoi(argv[a + 2]);
    const std::vector<df_opt_rule> rules = parse_rules(argv[a + 3]);
    df::Plan P;
    std::string err;
    int rc = df::build_plan(&D.chain, &P, &err, o.exact ? 1 : 0);
    if (rc != DF_OK) {
        std::printf("chain status %d %s\n", rc, err.c_str());
        return 1;
    }
    o.split = P.split && !o.exact;    // use_split / use_wsplit (df_capi.hip)
    o.wsplit = P.wsplit && !o.exact;
    std::vector<double> us;
    for (int r = 0; r < std::max(times, 1); ++r) {
        df::TrainPlan T;
        err.clear();
        const auto t0 = std::chrono::steady_clock::now();
        rc = df::build_train_plan(P, o, rules.data(), (int)rules.size(), &T, &err);
        const auto t1 = std::chrono::steady_clock::now();
        us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        if (times > 0) continue;
        std::printf("status %d %s\n", rc, rc == DF_OK ? "" : err.c_str());  // (err: defined for a failure)
        if (rc == DF_OK) print(P, T);
        return 0;
    }
    std::sort(us.begin(), us.end());
    std::printf("status %d median_us %.1f min_us %.1f max_us %.1f calls %d\n", rc, us[us.size() / 2], us.front(),
                us.back(), times);
    return rc == DF_OK ? 0 : 1;
}
