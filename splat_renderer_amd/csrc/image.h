// image.h — what the image-space kernels (loss.hip, depth_normals.hip) share: how a pixel of a strided float image is loaded, and
// the float64 wave sum their fixed-order reductions start from.
#pragma once

#include "common.h"

struct Px3 {
    float c[3];
};

// pixel i of an image; vec4: stride 4 on a 16-byte aligned base (workgroup-uniform)
__device__ __forceinline__ Px3 load_px(const float *__restrict__ p, uint32_t stride, bool vec4, size_t i) {
    Px3 r;
    if (vec4) {
        const float4 v = reinterpret_cast<const float4 *>(p)[i];
        r.c[0] = v.x; r.c[1] = v.y; r.c[2] = v.z;
    } else {
        const float *q = p + i * stride;
        r.c[0] = q[0]; r.c[1] = q[1]; r.c[2] = q[2];
    }
    return r;
}
__device__ __forceinline__ bool is_vec4(const float *p, uint32_t stride) { return stride == 4u && ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
