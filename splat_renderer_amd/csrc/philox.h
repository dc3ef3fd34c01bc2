// philox.h — the counter-based random numbers of the seeded kernels (density.hip's split children, mcmc.hip's draws and noise):
// Philox4x32-10 and the Box-Muller transform include/splat.h states for splat_densify_geometry.  Binary32, one rounding per
// operation as written; tests/density_ref.py restates both.
#pragma once
#include "common.h"

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float philox_unit(uint32_t x) { return (float)(((double)x + 0.5) * 0x1p-32); } // (0, 1]

// three standard normals of the four words: (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1, sqrt(-2 ln u2) cos 2 pi u3)
__device__ __forceinline__ float3 philox_normals3(uint4 x) {
    const float ra = sqrtf(-2.0f * logf(philox_unit(x.x))), rb = sqrtf(-2.0f * logf(philox_unit(x.z)));
    float sa, ca;
    sincosf(6.283185307179586f * philox_unit(x.y), &sa, &ca);
    const float cb = cosf(6.283185307179586f * philox_unit(x.w));
    return make_float3(ra * ca, ra * sa, rb * cb);
}
