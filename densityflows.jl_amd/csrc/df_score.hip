// df_score.hip — kernels of df_train_logpdf_grad: the per-net input-gradient sweep
// (df_score_impl.h, exact f32, hidden widths 16/32/64 and 0 or 1 hidden Dense) and the
// chain rule of the θ normalisation.
#include <mutex>

#include "df_score_impl.h"

namespace df {

namespace {

template <bool PAIR>
void* score_ptr_p(int ht, int nh, int am) {
#define DF_S(H)                                                                                           \
    (nh ? (am == trn::AM_RELU ? score_kernel_ptr<H, 1, trn::AM_RELU, PAIR>()                                   \
                              : (am == trn::AM_PRE ? score_kernel_ptr<H, 1, trn::AM_PRE, PAIR>()                \
                                                   : score_kernel_ptr<H, 1, trn::AM_Y, PAIR>()))                \
        : (am == trn::AM_RELU ? score_kernel_ptr<H, 0, trn::AM_RELU, PAIR>()                                   \
                              : (am == trn::AM_PRE ? score_kernel_ptr<H, 0, trn::AM_PRE, PAIR>()                \
                                                   : score_kernel_ptr<H, 0, trn::AM_Y, PAIR>())))
    if (nh < 0 || nh > 1 || am < 0 || am > 2) return nullptr;
    switch (ht) {
        case 1: return DF_S(1);
        case 2: return DF_S(2);
        case 4: return DF_S(4);
        default: return nullptr;
    }
#undef DF_S
}

void* score_ptr(int ht, int nh, int am, bool pair) {
    return pair ? score_ptr_p<true>(ht, nh, am) : score_ptr_p<false>(ht, nh, am);
}

// ∂θn/∂θ = 1 / (θmax - θmin), 0 for a constant row (normalize_input, src/Data.jl:213-218;
// grad_normalisation, src/Data.jl:236-241)
__global__ void score_theta_raw_kernel(float* gth, const float* tmin, const float* tmax, int n, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const int c = (int)(i % n);
        const float diff = tmax[c] - tmin[c];
        gth[i] = (diff == 0.f) ? 0.f : gth[i] / diff;
    }
}

// MaxDynamicSharedMemorySize of an instance = the largest request any launch of it has made
// in this process (the attribute belongs to the function, not to a trainer)
hipError_t raise_score_lds_limit(void* k, int ht, int nh, int am, bool pair, size_t lds) {
    static std::mutex mu;
    static size_t limit[5][2][3][2] = {};
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[ht][nh][am][pair ? 1 : 0];
    if (lds <= cur) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) cur = lds;
    return e;
}

}  // namespace

hipError_t launch_score_net(int ht, int nh, int am, bool pair, const ScoreArgs& a, unsigned grid, size_t lds,
                            hipStream_t st) {
    void* k = score_ptr(ht, nh, am, pair);
    if (!k) return hipErrorInvalidValue;
    if (lds > kScoreLdsMax) return hipErrorInvalidValue;
    hipError_t e = raise_score_lds_limit(k, ht, nh, am, pair, lds);
    if (e != hipSuccess) return e;
    void* args[] = {const_cast<ScoreArgs*>(&a)};
    return hipLaunchKernel(k, dim3(grid), dim3(kScoreThreads), args, lds, st);
}

hipError_t score_net_occupancy(int ht, int nh, int am, bool pair, size_t lds, int* blocks) {
    void* k = score_ptr(ht, nh, am, pair);
    if (!k) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k, kScoreThreads, lds);
}

hipError_t launch_score_theta_raw(float* gth, const float* tmin, const float* tmax, int n, int64_t batch,
                                  hipStream_t st) {
    const int64_t count = batch * n;
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(score_theta_raw_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, gth, tmin,
                       tmax, n, count);
    return hipGetLastError();
}

}  // namespace df
