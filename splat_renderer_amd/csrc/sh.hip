// sh.hip — view-dependent colour of anisotropic Gaussians (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference counterpart):
// real spherical harmonics of degree 0-3 in the basis and constants of 3D Gaussian splatting, evaluated towards the camera.
//
//   dir = normalize(p - eye),  rgb = max(0.5 + sum_k Y_k(dir) sh_k, 0),  w = opacity
//   (dir = (0, 0, 0) where |p - eye| is not a positive finite number — a splat at the eye: rgb = max(0.5 + C0 sh_0, 0))
//
// Roofline: HBM.  Per splat 16 B of position + 12 (deg + 1)^2 B of coefficients + 4 B opacity in, 16 B out (degree 3: 228 B);
// one lane per splat.  Coefficient rows whose stride and base allow it are read as float4s (the row's 48 floats at degree 3
// are twelve 16-byte loads instead of 48 scalar ones).
#include "common.h"
#include "variant.h"

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                            -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

template <int DEG, bool VEC4>
__global__ __launch_bounds__(256) void k_sh_colors(float ex, float ey, float ez, const float4 *__restrict__ pos, uint32_t pos_stride,
                                                   const float *__restrict__ sh, uint32_t sh_stride, const float *__restrict__ opacity,
                                                   uint32_t n, float4 *__restrict__ out) {
    constexpr int NB = (DEG + 1) * (DEG + 1), NF = 3 * NB, NV = (NF + 3) / 4;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float co[NV * 4];
    const float *row = sh + (size_t)i * sh_stride;
    if (VEC4) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float4 f = reinterpret_cast<const float4 *>(row)[v];
            co[4 * v] = f.x; co[4 * v + 1] = f.y; co[4 * v + 2] = f.z; co[4 * v + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NF; ++k) co[k] = row[k];
    }
    const float4 p = pos[(size_t)i * pos_stride];
    const float op = opacity[i];
    float x = p.x - ex, y = p.y - ey, z = p.z - ez;
    // a splat at the eye (or a length that is not a positive finite number) has no direction: (0, 0, 0), not 0 * inf
    const float len = sqrtf((x * x + y * y) + z * z);
    const bool has_dir = len > 0.0f && len < INFINITY;
    const float il = has_dir ? 1.0f / len : 0.0f;
    x = has_dir ? x * il : 0.0f; y = has_dir ? y * il : 0.0f; z = has_dir ? z * il : 0.0f;
    float Y[NB];
    Y[0] = SH_C0;
    if (DEG > 0) {
        Y[1] = -SH_C1 * y;
        Y[2] = SH_C1 * z;
        Y[3] = -SH_C1 * x;
    }
    if (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = SH_C2[0] * (x * y);
        Y[5] = SH_C2[1] * (y * z);
        Y[6] = SH_C2[2] * ((2.0f * zz - xx) - yy);
        Y[7] = SH_C2[3] * (x * z);
        Y[8] = SH_C2[4] * (xx - yy);
        if (DEG > 2) {
            Y[9] = SH_C3[0] * (y * (3.0f * xx - yy));
            Y[10] = SH_C3[1] * ((x * y) * z);
            Y[11] = SH_C3[2] * (y * ((4.0f * zz - xx) - yy));
            Y[12] = SH_C3[3] * (z * ((2.0f * zz - 3.0f * xx) - 3.0f * yy));
            Y[13] = SH_C3[4] * (x * ((4.0f * zz - xx) - yy));
            Y[14] = SH_C3[5] * (z * (xx - yy));
            Y[15] = SH_C3[6] * (x * (xx - 3.0f * yy));
        }
    }
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        r += Y[k] * co[3 * k];
        g += Y[k] * co[3 * k + 1];
        b += Y[k] * co[3 * k + 2];
    }
    out[i] = make_float4(fmaxf(r + 0.5f, 0.0f), fmaxf(g + 0.5f, 0.0f), fmaxf(b + 0.5f, 0.0f), op);
}

extern "C" int splat_sh_colors(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                               uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, uint32_t n, void *color_opacity_out) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, eye3 && degree <= 3 && pos_stride_vec4 >= 1);
    ARG_CHECK(ctx, n == 0 || (positions && sh && opacity_f32 && color_opacity_out));
    ARG_CHECK(ctx, sh_stride_floats >= 3 * (degree + 1) * (degree + 1));
    ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)color_opacity_out) & 15) == 0 && (((uintptr_t)sh | (uintptr_t)opacity_f32) & 3) == 0);
    if (n == 0) return SPLAT_OK;
    const uint32_t nf = 3 * (degree + 1) * (degree + 1);
    // float4 rows: every row 16-byte aligned and its rounded-up length inside the stride
    const bool vec4 = (sh_stride_floats % 4) == 0 && (((uintptr_t)sh) & 15) == 0 && sh_stride_floats >= (nf + 3) / 4 * 4;
    const dim3 grid(div_up(n, 256)), block(256);
    variant_dispatch(
        [&](auto deg, auto v4) {
            launch_kernel(ctx, NO_STAGE, k_sh_colors<deg.value, v4.value>, grid, block, eye3[0], eye3[1], eye3[2], (const float4 *)positions,
                          pos_stride_vec4, (const float *)sh, sh_stride_floats, (const float *)opacity_f32, n, (float4 *)color_opacity_out);
        },
        OneOf<0, 1, 2, 3>{(int)degree}, vec4);
    LAUNCH_CHECK(ctx, "k_sh_colors");
    return SPLAT_OK;
}
