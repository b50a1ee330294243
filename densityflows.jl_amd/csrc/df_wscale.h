// df_wscale.h — the fixed-point scale of a point's importance weights, device code shared by
// df_resample.hip (the scan and the picks), df_wquant.hip (the scale call and the weighted
// selection) and df_whist.hip (the weighted tables): one quantiser for all three.
//   quantise  a weight takes part when its bits lie in [1, 0x7f7fffff] (finite, > 0).  With the
//             largest such weight wmax = f·2^e, f in [0.5, 1), q_j = rint(w_j·2^(32 − e)) half
//             to even, formed from the weight's bits by shifts: no conversion, no rounding mode
// api::launch_weight_scale (df_wquant.hip): weight_scale_kernel over the (points · N) weights w
// (16-byte aligned, N a multiple of 4) into scale (2 int64 per point: e and T = Σ q, {0, 0} for a
// point without a weight that takes part); checked arguments, nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace df {

// the bits of a weight that takes part, 0 otherwise (NaN, ±inf, negative, ±0); among weights
// that take part the bits order as the values do
__device__ __forceinline__ uint32_t rs_key(float w) {
    const uint32_t b = __float_as_uint(w);
    return b - 1u < 0x7f7fffffu ? b : 0u;
}

__device__ __forceinline__ uint32_t rs_max4(uint32_t m, const uint32_t k[4]) {
    const uint32_t a = k[0] > k[1] ? k[0] : k[1], b = k[2] > k[3] ? k[2] : k[3];
    const uint32_t c = a > b ? a : b;
    return m > c ? m : c;
}

__device__ __forceinline__ uint32_t rs_wave_max(uint32_t m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, off, 64);
        m = m > o ? m : o;
    }
    return m;
}

// e with wmax = f·2^e, f in [0.5, 1), from wmax's bits (not 0)
__device__ __forceinline__ int rs_exponent(uint32_t maxkey) {
    const int ef = (int)(maxkey >> 23);
    return ef ? ef - 126 : (32 - __clz((int)maxkey)) - 149;
}

// rint(w·2^(32 − e)), half to even, of the weight with bits `key` (0: no part)
__device__ __forceinline__ uint64_t rs_quant(uint32_t key, int e) {
    if (key == 0u) return 0;
    const int ef = (int)(key >> 23);
    const uint32_t m = ef ? (key & 0x7fffffu) | 0x800000u : key;  // w = m·2^ex, m < 2^24
    const int ex = ef ? ef - 150 : -149;
    const int s = ex + 32 - e;  // at most 8 for a normal wmax, at most 31 and m·2^s < 2^32 otherwise
    if (s >= 0) return (uint64_t)m << s;
    const int r = -s;
    if (r > 24) return 0;  // m·2^−r < 1/2
    uint32_t q = m >> r;
    const uint32_t rem = m & ((1u << r) - 1u), half = 1u << (r - 1);
    q += (rem > half || (rem == half && (q & 1u))) ? 1u : 0u;
    return q;
}

namespace api {
int launch_weight_scale(const float* w, int64_t points, int N, int64_t* scale, hipStream_t st);
}  // namespace api

}  // namespace df
