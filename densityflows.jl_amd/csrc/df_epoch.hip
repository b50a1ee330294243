// df_epoch.hip — the kernels that feed a device-resident epoch (df_batch_gather,
// df_train_epoch): the mini-batch gather out of a resident data set, the check of an
// order array, and the device cursor that makes every full-batch step of an epoch the
// same captured graph.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "df_train.h"

namespace df {

namespace {

constexpr int kGatherThreads = 256;

unsigned gather_blocks(int64_t count) { return (unsigned)((count + kGatherThreads - 1) / kGatherThreads); }

}  // namespace

// One mini-batch of x (d floats per sample) and θ (n floats per sample) out of the resident
// set into the step's staging buffers, both (rows, B) column-major: sample j of the batch is
// row order[pos + j] of the set (order == nullptr: pos + j), pos = first + *cursor · batchsize
// (cursor == nullptr: first).  One thread per output float: the stores of a wave are 256
// contiguous bytes; the loads are dword loads (a row of d = 5 floats is not 16-byte aligned),
// contiguous within a row.  Lanes past count · (d + n) neither load nor store.  Both the
// position in `order` and the index read from it are compared unsigned against n_samples;
// one that fails reads row 0, so a bad order or cursor never becomes a bad address (the
// entry points refuse such input before any launch).
__global__ void __launch_bounds__(kGatherThreads)
batch_gather_kernel(float* __restrict__ x_out, float* __restrict__ th_out, const float* __restrict__ x_set,
                    const float* __restrict__ th_set, int d, int n, int64_t n_samples,
                    const int32_t* __restrict__ order, int64_t first, const int64_t* __restrict__ cursor,
                    int64_t batchsize, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    const int64_t nx = count * d;
    if (e >= nx + count * n) return;
    const bool is_x = e < nx;
    const int64_t q = is_x ? e : e - nx;
    const int w = is_x ? d : n;
    const int64_t j = q / w;
    const int r = (int)(q - j * w);
    const int64_t pos = first + (cursor ? *cursor * batchsize : 0) + j;
    int64_t row = 0;
    if ((uint64_t)pos < (uint64_t)n_samples) {
        row = order ? (int64_t)order[pos] : pos;
        if ((uint64_t)row >= (uint64_t)n_samples) row = 0;
    }
    if (is_x)
        x_out[q] = x_set[row * d + r];
    else
        th_out[q] = th_set[row * n + r];
}

// The same gather with a third array, the sample weights: w_out[j] = w_set[row j], by the
// threads past the x and θ elements.  The same rule for a bad position or index (row 0).
__global__ void __launch_bounds__(kGatherThreads)
batch_gather_w_kernel(float* __restrict__ x_out, float* __restrict__ th_out, float* __restrict__ w_out,
                      const float* __restrict__ x_set, const float* __restrict__ th_set,
                      const float* __restrict__ w_set, int d, int n, int64_t n_samples,
                      const int32_t* __restrict__ order, int64_t first, const int64_t* __restrict__ cursor,
                      int64_t batchsize, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    const int64_t nx = count * d, nt = count * n;
    if (e >= nx + nt + count) return;
    const int which = e < nx ? 0 : (e < nx + nt ? 1 : 2);
    const int64_t q = which == 0 ? e : (which == 1 ? e - nx : e - nx - nt);
    const int w = which == 0 ? d : (which == 1 ? n : 1);
    const int64_t j = q / w;
    const int r = (int)(q - j * w);
    const int64_t pos = first + (cursor ? *cursor * batchsize : 0) + j;
    int64_t row = 0;
    if ((uint64_t)pos < (uint64_t)n_samples) {
        row = order ? (int64_t)order[pos] : pos;
        if ((uint64_t)row >= (uint64_t)n_samples) row = 0;
    }
    if (which == 0)
        x_out[q] = x_set[row * d + r];
    else if (which == 1)
        th_out[q] = th_set[row * n + r];
    else
        w_out[q] = w_set[row];
}

// *bad = the number of entries of order[0, n_samples) outside [0, n_samples); *bad is zeroed
// by the launcher.  A valid order adds nothing.
__global__ void __launch_bounds__(kGatherThreads)
order_range_kernel(const int32_t* __restrict__ order, int64_t n_samples, int* __restrict__ bad) {
    int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kGatherThreads + threadIdx.x; i < n_samples;
         i += (int64_t)gridDim.x * kGatherThreads)
        mine += (uint64_t)(int64_t)order[i] >= (uint64_t)n_samples ? 1 : 0;
    if (mine) atomicAdd(bad, mine);
}

// The end of one step of an epoch (adam_advance_kernel's pattern): the step's Σ logpdf goes
// to step_lp[*cursor] when the caller asked for the curve, then the cursor moves on.
__global__ void cursor_advance_kernel(int64_t* cursor, const double* lp, double* step_lp) {
    if (threadIdx.x == 0) {
        const int64_t c = *cursor;
        if (step_lp) step_lp[c] = *lp;
        *cursor = c + 1;
    }
}

// The weighted step's end: both of its sums to step_ws[2·*cursor], then the cursor moves on.
__global__ void cursor_advance_w_kernel(int64_t* cursor, const double* ws, double* step_ws) {
    if (threadIdx.x == 0) {
        const int64_t c = *cursor;
        if (step_ws) {
            step_ws[2 * c] = ws[0];
            step_ws[2 * c + 1] = ws[1];
        }
        *cursor = c + 1;
    }
}

hipError_t launch_batch_gather_w(float* x_out, float* th_out, float* w_out, const float* x_set, const float* th_set,
                                 const float* w_set, int d, int n, int64_t n_samples, const int32_t* order,
                                 int64_t first, const int64_t* cursor, int64_t batchsize, int64_t count,
                                 hipStream_t st) {
    if (!th_out || !th_set) n = 0;
    const int64_t total = count * ((int64_t)d + n + 1);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_gather_w_kernel, dim3(gather_blocks(total)), dim3(kGatherThreads), 0, st, x_out, th_out,
                       w_out, x_set, th_set, w_set, d, n, n_samples, order, first, cursor, batchsize, count);
    return hipGetLastError();
}

hipError_t launch_cursor_advance_w(int64_t* cursor, const double* ws, double* step_ws, hipStream_t st) {
    hipLaunchKernelGGL(cursor_advance_w_kernel, dim3(1), dim3(64), 0, st, cursor, ws, step_ws);
    return hipGetLastError();
}

hipError_t launch_batch_gather(float* x_out, float* th_out, const float* x_set, const float* th_set, int d, int n,
                               int64_t n_samples, const int32_t* order, int64_t first, const int64_t* cursor,
                               int64_t batchsize, int64_t count, hipStream_t st) {
    if (!th_out || !th_set) n = 0;
    const int64_t total = count * ((int64_t)d + n);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_gather_kernel, dim3(gather_blocks(total)), dim3(kGatherThreads), 0, st, x_out, th_out,
                       x_set, th_set, d, n, n_samples, order, first, cursor, batchsize, count);
    return hipGetLastError();
}

hipError_t launch_order_range(const int32_t* order, int64_t n_samples, int* bad, hipStream_t st) {
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e != hipSuccess || n_samples <= 0) return e;
    const unsigned grid = (unsigned)std::min<int64_t>(gather_blocks(n_samples), 1024);
    hipLaunchKernelGGL(order_range_kernel, dim3(grid), dim3(kGatherThreads), 0, st, order, n_samples, bad);
    return hipGetLastError();
}

hipError_t launch_cursor_advance(int64_t* cursor, const double* lp, double* step_lp, hipStream_t st) {
    hipLaunchKernelGGL(cursor_advance_kernel, dim3(1), dim3(64), 0, st, cursor, lp, step_lp);
    return hipGetLastError();
}

}  // namespace df
