// Probe: matrix-pipe cost of the two instructions that can form the bf16x3 split's remainders
// c - hi (df_uniform_impl.h mrem): v_mfma_f32_4x4x4_16b_bf16 (16 blocks of 4x4, lane-local with
// A = -I per block) against v_mfma_f32_16x16x16_bf16 (A = -I), each alone and interleaved
// one-for-one with the product instruction v_mfma_f32_16x16x32_bf16 on separate accumulators.
// One workgroup of 4 waves per CU (one wave per SIMD), 12 instructions per loop trip on
// independent accumulator chains; time from hipEvents over the whole grid, clock calibrated
// against v_mfma_f32_16x16x4_f32 (32 cycles, as in mfma_issue.hip).
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short short4v __attribute__((ext_vector_type(4)));
constexpr int kIters = 32768, kChains = 6;  // 12 per trip: 2 x 6 alone, 6 + 6 interleaved

#define REM4(c) asm volatile("v_mfma_f32_4x4x4_16b_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(e), "v"(h))
#define REM16(c) asm volatile("v_mfma_f32_16x16x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(e), "v"(h))
#define PROD(c) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b))

#define PROLOGUE                                                        \
    bf16x8 a, b;                                                        \
    for (int k = 0; k < 8; ++k) {                                       \
        a[k] = (__bf16)in[(threadIdx.x + k) & 63];                      \
        b[k] = (__bf16)in[(threadIdx.x + 3 * k) & 63];                  \
    }                                                                   \
    short4v e, h;                                                       \
    for (int k = 0; k < 4; ++k) {                                       \
        e[k] = (k == (int)(threadIdx.x & 3)) ? (short)0xbf80 : (short)0; \
        h[k] = (short)(0x3c00 + ((threadIdx.x + k) & 63));              \
    }                                                                   \
    f32x4 c[kChains], p[kChains];                                       \
    for (int j = 0; j < kChains; ++j) c[j] = p[j] = f32x4{0.f, 0.f, 0.f, 0.f};

#define EPILOGUE                                                                                        \
    float s = 0.f;                                                                                      \
    for (int j = 0; j < kChains; ++j) s += c[j][0] + c[j][1] + c[j][2] + c[j][3] + p[j][0] + p[j][3]; \
    out[blockIdx.x * 256 + threadIdx.x] = s;

__global__ void __launch_bounds__(256) rem4_alone(const float* in, float* out) {
    PROLOGUE
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kChains; ++j) REM4(c[j]);
    EPILOGUE
}

__global__ void __launch_bounds__(256) rem16_alone(const float* in, float* out) {
    PROLOGUE
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kChains; ++j) REM16(c[j]);
    EPILOGUE
}

__global__ void __launch_bounds__(256) prod_alone(const float* in, float* out) {
    PROLOGUE
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kChains; ++j) PROD(p[j]);
    EPILOGUE
}

__global__ void __launch_bounds__(256) rem4_prod(const float* in, float* out) {
    PROLOGUE
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int j = 0; j < kChains; ++j) {
            REM4(c[j]);
            PROD(p[j]);
        }
    EPILOGUE
}

__global__ void __launch_bounds__(256) rem16_prod(const float* in, float* out) {
    PROLOGUE
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int j = 0; j < kChains; ++j) {
            REM16(c[j]);
            PROD(p[j]);
        }
    EPILOGUE
}

__global__ void __launch_bounds__(256) calib_16x16x4(const float* in, float* out) {
    const float a = in[threadIdx.x & 63], b = in[(threadIdx.x + 7) & 63];
    f32x4 c[kChains];
    for (int j = 0; j < kChains; ++j) c[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < kIters; ++i)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < kChains; ++j) c[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c[j], 0, 0, 0);
    float s = 0.f;
    for (int j = 0; j < kChains; ++j) s += c[j][0] + c[j][1] + c[j][2] + c[j][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <typename K>
static float time_ms(K kern, int grid, const float* in, float* out) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, in, out);
    hipEventRecord(e0, 0);
    for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, 0, in, out);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ms / 5.f;
}

int main() {
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    float *in, *out;
    hipMalloc(&in, 64 * 4);
    hipMalloc(&out, (size_t)cus * 256 * 4);
    float hbuf[64];
    for (int i = 0; i < 64; ++i) hbuf[i] = 1e-3f * (i + 1);
    hipMemcpy(in, hbuf, sizeof hbuf, hipMemcpyHostToDevice);
    const double trips = (double)kIters;  // per SIMD: one wave, kIters trips of 12 instructions
    const double cyc = 32.0 * 12.0 / (time_ms(calib_16x16x4, cus, in, out) / trips);  // cycles per ms
    const double prod = time_ms(prod_alone, cus, in, out) / trips * cyc / 12.0;
    const double r4 = time_ms(rem4_alone, cus, in, out) / trips * cyc / 12.0;
    const double r16 = time_ms(rem16_alone, cus, in, out) / trips * cyc / 12.0;
    const double r4p = time_ms(rem4_prod, cus, in, out) / trips * cyc / 6.0;    // per (rem, product) pair
    const double r16p = time_ms(rem16_prod, cus, in, out) / trips * cyc / 6.0;
    printf("CUs %d, one wave per SIMD, clock (from the 16x16x4 f32 calibration) %.0f MHz\n", cus, cyc / 1e3);
    printf("  v_mfma_f32_16x16x32_bf16 alone              %6.2f cycles per instruction\n", prod);
    printf("  v_mfma_f32_4x4x4_16b_bf16 alone             %6.2f cycles per instruction\n", r4);
    printf("  v_mfma_f32_16x16x16_bf16 alone              %6.2f cycles per instruction\n", r16);
    printf("  4x4x4 interleaved with 16x16x32             %6.2f cycles per pair, %6.2f beyond the product\n", r4p,
           r4p - prod);
    printf("  16x16x16 interleaved with 16x16x32          %6.2f cycles per pair, %6.2f beyond the product\n", r16p,
           r16p - prod);
    return 0;
}
