// df_philox.h — the library's counter-based generator: Philox4x32-10 (Salmon et al., "Parallel
// random numbers: as easy as 1, 2, 3", SC'11), one 128-bit counter and a 64-bit key into four
// 32-bit words.  df_sample.hip draws the base normals from counters (ctr, 0, 0, 0);
// df_resample.hip takes its uniform words from counters (ctr, 1, 0): disjoint at any seed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace df {

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

}  // namespace df
