// The repack table is closed (tests/test_repack_closure.py compiles this file with df_plan.cpp
// and df_train_plan.cpp under -fsanitize=address,undefined and runs it as a child process; no
// GPU, nothing loaded into Python).
//
//   repack_closure <descriptor A> <descriptor B> <exact: -1 | 0 | 1> <sweep>
//
// The descriptor files: tests/plan_desc.h; A and B are one structure with two parameter sets.
// exact -1: DF_F32_EXACT, as df_chain_create reads it (and DF_NO_WIDE).  sweep: the int
// df_train_create_opt takes.  Both chains are planned, both get a trainer plan under the
// default Adam rule, and every entry of TrainPlan::map_sources is held to:
//
//   bounds     every dst lies inside its blob (4·dst + 4 <= bytes for a word map; dst + 2, or
//              dst + 4 for plane 3, for a plane map), plane 0-2 destinations are 2-byte
//              aligned and plane-3 ones 4-byte aligned, every src decodes to [0, n_params)
//   conflicts  no two entries write overlapping bytes from different sources
//   closure    A's blob after A's map has run on B's trainables (what repack_kernel and
//              repack_split_kernel do: a float copy, bf16_split_plane for planes 0-2, the four
//              bytes for plane 3) is B's blob, byte for byte
//   on-flags   a map that is off has an empty blob, or one that A and B agree on
//
// Prints one "map <i> <name> on <0|1> split <0|1> n <entries> bytes <blob bytes>" line per map
// and "closed" at the end (exit status 0); the first violation goes to stderr with the map
// and the offset (exit status 1).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "df_plan.h"
#include "plan_desc.h"
#include "df_train_plan.h"

namespace {

const char* const kNames[df::TrainPlan::kMaps] = {"MP", "MT", "MW", "MWB", "MS", "MWS", "ML", "MTS", "MLS"};

struct Side {
    Desc D;
    df::Plan P;
    df::TrainPlan T;
};

bool env_is_1(const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
}

bool plan(const char* path, int ex, int sweep, Side& s) {
    if (!load(path, s.D)) {
        std::fprintf(stderr, "cannot read %s\n", path);
        return false;
    }
    df::TrainPlanOpts o;
    o.exact = ex < 0 ? env_is_1("DF_F32_EXACT") : ex == 1;
    o.no_wide = env_is_1("DF_NO_WIDE");
    o.sweep = sweep;
    std::string err;
    int rc = df::build_plan(&s.D.chain, &s.P, &err, o.exact ? 1 : 0);
    if (rc != DF_OK) {
        std::fprintf(stderr, "%s: chain status %d %s\n", path, rc, err.c_str());
        return false;
    }
    o.split = s.P.split && !o.exact;  // use_split / use_wsplit (df_capi.hip)
    o.wsplit = s.P.wsplit && !o.exact;
    const df_opt_rule adam{DF_OPT_ADAM, {1e-3f, 0.9f, 0.999f, 1e-8f}};  // df_train_create's default
    rc = df::build_train_plan(s.P, o, &adam, 1, &s.T, &err);
    if (rc != DF_OK) {
        std::fprintf(stderr, "%s: trainer status %d %s\n", path, rc, err.c_str());
        return false;
    }
    return true;
}

template <class T>
std::vector<uint8_t> bytes_of(const std::vector<T>& v) {
    std::vector<uint8_t> out(v.size() * sizeof(T));
    if (!out.empty()) std::memcpy(out.data(), v.data(), out.size());
    return out;
}

// The nine blobs in TrainPlan::MP ... MLS order (df_train_create_opt's `blobs`).
std::vector<std::vector<uint8_t>> blobs_of(const Side& s) {
    return {bytes_of(s.P.blob),   bytes_of(s.T.tblob),  bytes_of(s.P.wblob),  bytes_of(s.P.wbias), bytes_of(s.P.sblob),
            bytes_of(s.P.wsblob), bytes_of(s.T.lblob),  bytes_of(s.T.tsblob), bytes_of(s.T.lsblob)};
}

int fail(int i, const char* what, long long entry, long long dst, long long src) {
    std::fprintf(stderr, "map %d (%s): %s at entry %lld (dst %lld, src %lld)\n", i, kNames[i], what, entry, dst, src);
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <descriptor A> <descriptor B> <exact: -1 | 0 | 1> <sweep>\n", argv[0]);
        return 2;
    }
    const int ex = std::atoi(argv[3]), sweep = std::atoi(argv[4]);
    Side A, B;
    if (!plan(argv[1], ex, sweep, A) || !plan(argv[2], ex, sweep, B)) return 2;
    const int64_t np = A.T.n_params;
    if (np != (int64_t)A.P.trainables.size() || np != B.T.n_params || np != (int64_t)B.P.trainables.size()) {
        std::fprintf(stderr, "parameter counts differ: A %lld / %zu, B %lld / %zu\n", (long long)np,
                     A.P.trainables.size(), (long long)B.T.n_params, B.P.trainables.size());
        return 1;
    }
    const auto ma = A.T.map_sources(A.P), mb = B.T.map_sources(B.P);
    std::vector<std::vector<uint8_t>> ba = blobs_of(A);
    const std::vector<std::vector<uint8_t>> bb = blobs_of(B);
    const float* params = B.P.trainables.data();
    for (int i = 0; i < df::TrainPlan::kMaps; ++i) {
        const df::MapSrc &a = ma[i], &b = mb[i];
        std::vector<uint8_t>& blob = ba[i];
        const size_t bytes = blob.size();
        std::printf("map %d %s on %d split %d n %zu bytes %zu\n", i, kNames[i], (int)a.on, (int)a.split,
                    a.on ? a.dst->size() : (size_t)0, bytes);
        // the structure is the parameters' to leave alone
        if (a.on != b.on || a.split != b.split || *a.dst != *b.dst || *a.src != *b.src || bytes != bb[i].size()) {
            std::fprintf(stderr, "map %d (%s): A and B plan different maps or blob sizes\n", i, kNames[i]);
            return 1;
        }
        if (!a.on) {  // on-flags: nothing regathers this blob, so nothing in it may follow the parameters
            if (bytes != 0 && std::memcmp(blob.data(), bb[i].data(), bytes) != 0) {
                std::fprintf(stderr, "map %d (%s): switched off, but its blob differs between A and B\n", i,
                             kNames[i]);
                return 1;
            }
            continue;
        }
        if (a.dst->size() != a.src->size()) {
            std::fprintf(stderr, "map %d (%s): %zu destinations, %zu sources\n", i, kNames[i], a.dst->size(),
                         a.src->size());
            return 1;
        }
        std::vector<int32_t> owner(bytes, -1);  // the source that wrote each byte
        for (size_t e = 0; e < a.dst->size(); ++e) {
            const int64_t dst = (*a.dst)[e], code = (*a.src)[e];
            const int plane = a.split ? (int)(code & 3) : 3;
            const int64_t src = a.split ? code >> 2 : code;
            const int64_t at = a.split ? dst : 4 * dst;
            const int64_t width = plane == 3 ? 4 : 2;
            if (dst < 0 || at + width > (int64_t)bytes) return fail(i, "destination outside the blob", e, dst, code);
            if (at % width != 0) return fail(i, "misaligned destination", e, dst, code);
            if (code < 0 || src >= np) return fail(i, "source outside the parameters", e, dst, code);
            for (int64_t q = at; q < at + width; ++q) {
                if (owner[q] >= 0 && owner[q] != (int32_t)code)
                    return fail(i, "bytes written from two sources", e, dst, code);
                owner[q] = (int32_t)code;
            }
            const float v = params[src];
            if (plane == 3) {
                std::memcpy(blob.data() + at, &v, 4);
            } else {
                const uint16_t h = df::bf16_split_plane(v, plane);
                std::memcpy(blob.data() + at, &h, 2);
            }
        }
        for (size_t q = 0; q < bytes; ++q) {
            if (blob[q] == bb[i][q]) continue;
            std::fprintf(stderr,
                         "map %d (%s): not closed: byte %zu is %02x after the regather, %02x in B's blob; "
                         "written by source %d%s\n",
                         i, kNames[i], q, blob[q], bb[i][q], owner[q],
                         owner[q] < 0 ? " (no entry writes it)" : a.split ? " (index·4 + plane)" : "");
            return 1;
        }
    }
    std::printf("closed\n");
    return 0;
}
