// df_handle.h — the df_chain handle and the host helpers shared by the C ABI
// translation units (df_capi.hip: inference entry points; df_train_capi.hip:
// training entry points, with df_lsweep.hip: the layer-wise reverse sweep; the
// df_train handle of those two is in df_trainer.h, its host plan in df_train_plan.h).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "densityflows_hip.h"
#include "df_kernels.h"
#include "df_plan.h"

// Move-only owner of one hipMalloc allocation.  The destructor frees on the current
// device: handles are deleted inside their DeviceGuard scope.
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    // frees what it held, then allocates (empty again on failure)
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    void* get() const { return p_; }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p_);
    }

  private:
    void* p_ = nullptr;
};

struct df_chain {
    df::Plan plan;
    int device = 0;
    bool exact = false;         // DF_F32_EXACT=1 at df_chain_create: exact-f32 kernels only (read once)
    // launch knobs, read from the environment once at df_chain_create (a launch does no
    // getenv): DF_NO_WIDE=1, DF_DEBUG_LAUNCH=1, DF_TILES, DF_SMALL_MAX (-1: unset), DF_GRID_CUS
    // (grid_cus below)
    bool no_wide = false;
    bool debug_launch = false;
    int force_tiles = 0;
    int64_t small_max = -1;
    int small_waves = 2;  // DF_SMALL_WAVES: waves per small-kernel workgroup (1 or 2)
    // the small-batch kernel's descriptor, by flow (θ normalised) 0 / 1; rebuilt after
    // df_chain_set_weights / df_chain_set_theta_bounds
    df::SmallDesc small_sd[2] = {};
    bool small_sd_ok[2] = {false, false};
    DevBuf d_layers;
    DevBuf d_denses;
    DevBuf d_chunks;
    DevBuf d_stages;
    DevBuf d_blob;
    DevBuf d_tables;
    DevBuf d_params;
    DevBuf d_bounds;  // float [θmin (n) | θmax (n)]
    bool has_bounds = false;
    std::vector<float> h_bounds;  // host copy of d_bounds (the small-batch kernel's descriptor)
    DevBuf d_partial;  // double [partial_cap]
    int64_t partial_cap = 0;
    int64_t partial_gen = 0;  // bumped when d_partial is reallocated (captured train graphs hold it)
    int stage_bytes = 0;
    int n_stage_bufs = 1;
    DevBuf d_sched;    // [fwd schedule | bwd schedule]
    DevBuf d_ulayers;  // specialised-kernel descriptors
    int n_cu = 0;
    // DF_GRID_CUS (read once at df_chain_create; unset, 0 or invalid: n_cu; clamped to
    // [1, n_cu]): the CU count the persistent training and score grids are sized from
    // (df_train::grid, lgrid, score_grid and the Dense grid of the layer-wise sweep).  A test
    // aid: a small value brings several trips of every batch loop down to small batches.  The
    // chain-pass kernels (use_small, choose_tiles) keep n_cu.
    int grid_cus = 0;
    int occ[4][df::kMaxTilesPerWave + 1] = {};  // resident workgroups per CU, by mode and tiles
    int tab_bytes = 0;
    size_t lds = 0;
    int n_trainers = 0;         // live df_train handles bound to this chain
    // The live trainer whose repack() last wrote the packed blobs (nullptr: they hold
    // plan.trainables).  Its d_params are the parameters the chain evaluates: a trainer created
    // now starts from them, and df_train_destroy of the owner copies them into plan.trainables.
    df_train* params_owner = nullptr;
    // wide-net kernel (plan.wide): its own blob, stages, schedules, descriptors
    DevBuf d_wlayers;
    DevBuf d_wstages;
    DevBuf d_wblob;
    DevBuf d_wbias;
    DevBuf d_wsched;
    size_t wide_lds = 0;
    // SPLIT variant of the FAST kernel (plan.split): its own blob, stages, schedules, descriptors
    DevBuf d_sblob;
    DevBuf d_sstages;
    DevBuf d_ssched;
    DevBuf d_sulayers;
    int sstage_bytes = 0;
    int sn_stage_bufs = 1;
    size_t slds = 0;
    int socc[4][df::kMaxTilesPerWave + 1] = {};
    // SPLIT variant of the wide kernel (plan.wsplit)
    DevBuf d_wslayers;
    DevBuf d_wsstages;
    DevBuf d_wsblob;
    DevBuf d_wssched;
    DevBuf d_wstables;
    int wstab_bytes = 0;
    size_t wslds = 0;
    // effective-clock stamps (df_chain_clock_probe): 2 × uint64 per workgroup slot
    DevBuf d_clk;
    int64_t clk_cap = 0;  // workgroup slots
    bool clk_on = false;
    // θ broadcast workspace of df_flow_sample (NTuple θ), which allocates and grows it itself
    float* d_theta_ws = nullptr;
    int64_t theta_ws_cap = 0;
    // staging of df_flow_logpdf_grid: one chunk's [x (d, chunk) | θ (n, chunk)]; only grows
    DevBuf d_grid_ws;
    int64_t grid_ws_cap = 0;  // floats
    // workspaces of df_flow_sample_region (df_reject.hip), sized for one round of rej_cap
    // candidates; they only grow
    DevBuf d_rej_cand;    // float [d · rej_cap]: the round's candidates
    DevBuf d_rej_theta;   // float [n · rej_cap]: the θ broadcast
    DevBuf d_rej_mask;    // uint64 [rej_cap / 64]: one acceptance ballot per wave
    DevBuf d_rej_base;    // uint32 [rej_cap / 64]: accepted before each wave, within the round
    DevBuf d_rej_region;  // float [lo (d) | hi (d) | a (n_half · d) | b (n_half)]
    DevBuf d_rej_cnt;     // int64 [accepted | tried | round base | -]
    int64_t rej_cap = 0;  // candidates
    std::vector<float> h_rej_region;  // the host block d_rej_region was last uploaded from
    // workspace of df_flow_logpdf_wsum / df_chain_logpdf_wsum: the per-sample logpdf (float
    // [wlp_cap]) and the span sums of the fp64 reductions; they only grow
    DevBuf d_wlp, d_wlp_part;
    int64_t wlp_cap = 0;
    // df_moments.hip; capacities in bytes, they only grow.  df_flow_sample_logpdf: the forward
    // pass's ldj (float [batch]).  df_flow_sample_logpdf_moments: one chunk's x (d, chunk) and
    // lp (chunk), and the reduction's per-workgroup blocks (double [workgroups][3])
    DevBuf d_slp_ldj, d_mom_x, d_mom_lp, d_mom_part;
    int64_t slp_ldj_cap = 0, mom_x_cap = 0, mom_lp_cap = 0, mom_part_cap = 0;
    // df_calib.hip; capacities in bytes, they only grow.  df_flow_hpd_ranks draws one chunk's x
    // into d_mom_x, its base term into d_mom_lp and its ldj into d_slp_ldj; its own are the θ
    // rows repeated over a chunk's draws (float [n · chunk]) and the points' lp (float
    // [n_points], when the caller gives no logpdf_out)
    // df_pstats.hip: df_flow_point_stats draws one chunk's x into d_mom_x and repeats θ into
    // d_hpd_th in the same way; it has no workspace of its own
    DevBuf d_hpd_th, d_hpd_lp;
    int64_t hpd_th_cap = 0, hpd_lp_cap = 0;
    ~df_chain() {
        if (d_theta_ws) (void)hipFree(d_theta_ws);
    }
};

// SPLIT launches unless the chain was created under DF_F32_EXACT=1 (df_chain::exact)
bool use_split(const df_chain* c);
bool use_wsplit(const df_chain* c);

namespace df {
namespace api {

int set_err(int code, const std::string& msg);
int hip_err(hipError_t e, const char* where);
const char* last_error();

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess)) ok = true;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

template <typename T>
int upload(const std::vector<T>& v, DevBuf& dst) {
    size_t bytes = v.size() * sizeof(T);
    if (bytes == 0) bytes = 16;
    hipError_t e = dst.alloc(bytes);
    if (e != hipSuccess) return set_err(DF_ERR_NOMEM, "hipMalloc failed for the chain plan");
    if (!v.empty()) {
        e = hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_err(e, "hipMemcpy(plan)");
    }
    return DF_OK;
}

constexpr double kLog2Pi = 1.8378770664093453;  // log(2π)

// Device ordinal of a df_train handle (df_train_capi.hip; df_comm.hip checks it).
int train_device(const df_train* t);
// Device double the last df_train_gradient wrote Σ logpdf to (the caller's or the handle's own).
double* train_last_lpsum(df_train* t);

// df_flow_sample's θ checks (df_sample.hip): raw θ present and bounds set when n > 0.
int sample_check_theta(const df_chain* c, const float* theta_raw);
// df_flow_sample between those checks and its forward pass: the draw into x_out and, for
// theta_broadcast, the θ broadcast into the chain's workspace.  *theta_use is the (n, batch)
// θ the pass reads.  batch > 0; the caller holds the device.
int sample_draw(df_chain* c, float* x_out, const float* theta_raw, int theta_broadcast, int64_t batch, uint64_t seed,
                uint64_t offset, void* stream, const float** theta_use);

// df_moments.hip, shared with df_calib.hip.  capturing: the stream records a graph.  reserve: a
// handle's workspace holds `need` bytes afterwards; it only grows, and not inside a capture.
// launch_base_logpdf: the base term of df_flow_sample_logpdf (base_logpdf_kernel) of the (d, batch)
// draw z into lp.
bool capturing(hipStream_t st);
int reserve(DevBuf& buf, int64_t& cap, int64_t need, hipStream_t st, const char* what);
int launch_base_logpdf(const float* z, float* lp, int d, int64_t batch, hipStream_t st);

// df_calib.hip, shared with df_pstats.hip.  theta_repeat_kernel: column i·n_draws + k of dst
// (n, points · n_draws) is column i of th (n, points); total = n · points · n_draws > 0.
int launch_theta_repeat(float* dst, const float* th, int n, int64_t n_draws, int64_t total, hipStream_t st);

// df_pstats.hip, shared with df_quant.hip and df_hist.hip.  point_check_sizes: the rules of
// df_flow_point_stats on the chain pointer, n_points, n_draws and chunk, in its order and with
// its messages, before any use of the handle.  point_draw_chunks: that call from its first use of
// the handle on — per chunk of whole points the draw, the θ repeat, the forward pass, and what
// `out` asks for over the chunk, every member optional: the copy into draws, point_stats_kernel
// for rank (needs x) / sums, the selection of the n_orders `orders` (HOST, checked by the
// caller) into quant, and the tables of the planned histograms `hist` (edges: DEVICE) into
// counts.  n_points > 0.
struct HistTables;
struct PointOutputs {
    int32_t* rank = nullptr;
    double* sums = nullptr;
    float* draws = nullptr;
    const int32_t* orders = nullptr;
    int n_orders = 0;
    float* quant = nullptr;
    const HistTables* hist = nullptr;
    const float* edges = nullptr;
    int32_t* counts = nullptr;
};
int point_check_sizes(const df_chain* c, int64_t n_points, int64_t n_draws, int64_t chunk);
int point_draw_chunks(df_chain* c, const float* x, const float* theta_raw, int64_t n_points, int64_t n_draws,
                      int64_t chunk, uint64_t seed, uint64_t offset, const PointOutputs& out, void* stream);

// df_hist.hip.  check_histogram_tables: rules 4 (edges, bins, keep non-null) to 8 of
// df_draw_histograms; with a chain, d is the chain's, read after the n_tables rule.
// plan_histograms: the groups of checked tables for both team sizes (free_histograms).
// launch_draw_histograms: draw_hist_kernel over the (d, points · N) draws xs (16-byte aligned, N a
// multiple of 4, points > 0) into the points' blocks at counts, zeroed first on the split path.
int check_histogram_tables(const df_chain* c, int d, const float* edges, const int32_t* bins, const int32_t* keep,
                           int32_t n_tables, int64_t n_points, int64_t* block_words);
HistTables* plan_histograms(int d, const int32_t* bins, const int32_t* keep, int32_t n_tables);
void free_histograms(HistTables* h);
int64_t histogram_block_words(const HistTables* h);
int launch_draw_histograms(const float* xs, int d, int N, int64_t points, const float* edges, const HistTables* h,
                           int32_t* counts, hipStream_t st);

// df_quant.hip.  check_orders: orders non-null, 1 <= n_orders <= DF_QUANT_MAX_ORDERS, every order
// in [0, n_draws).  launch_order_statistics: order_select_kernel over the (d, points · N) draws xs
// (16-byte aligned, N a multiple of 4, points > 0, checked orders) into out[(i·d + k)·n_orders + q].
int check_orders(const int32_t* orders, int n_orders, int64_t n_draws);
int launch_order_statistics(const float* xs, int d, int N, int64_t points, const int32_t* orders, int n_orders,
                            float* out, hipStream_t st);

// Launch one fused chain pass.  flow: θ normalised with the handle's bounds;
// snap (inverse modes, specialised kernel): every layer's output kept.
int run(df_chain* c, int mode, bool flow, const float* zin, const float* theta, float* xout, float* ldj, float* lp,
        double* sum_out, int64_t batch, void* stream, float* snap = nullptr, float* hsave = nullptr,
        int hsave_w = 0, int hsave_h = 0, float* fsave = nullptr);

}  // namespace api
}  // namespace df
