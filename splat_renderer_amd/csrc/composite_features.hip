// composite_features.hip — per-splat feature channels blended with a frame's own weights, and their backward (include/splat.h,
// "Feature channels of a frame"; an extension, no reference counterpart).  Each splat carries K floats f_i[0..K), 1 <= K <= 32;
// a pixel's F[k] = sum_i w_i f_i[k] over the entries it consumed, w_i = T_i alpha_i exactly as the kernel that drew the frame
// formed it: both kernels walk the tile's list with composite_walk.h's stage_chunk / entry_alpha / blend_step<PX>, so a pixel
// stops at the entry the image's pixel stopped at.  No background term, no division by sum w.  Compiled with contraction on,
// as composite_grad.hip is.
//
// k_composite_features<KW, PX>
//   composite_grad.hip's walk 1 with KW per-lane accumulators.  An entry's feature row is staged in LDS next to its
//   GradEntry, gathered by the entry's index; nothing is reduced over a wave, so a stopped lane leaves the chunk's loop.
//   Every lane stores its own pixel's K floats: out is written at every pixel of the screen.
// k_composite_features_backward<KW, PX>
//   Walk 1: L, T_{L-1}, T_L.  Walk 2, back to front with the empty-ballot skip: s_i = G_F . f_i, dL/dalpha_i =
//   T_i (s_i - S_i), S_{i-1} = alpha_i s_i + (1 - alpha_i) S_i from S = 0 behind the last consumed entry (every feature's
//   background is 0).  Per touched entry and wave 6 + KW numbers are summed with DPP: c.x, c.y, B00, B01, B11, opacity, then
//   w_i G_F[k]; the four waves meet in LDS as (w0 + w1) + (w2 + w3) and one float atomic add goes out per touched (entry,
//   number) with k < K: reproducible to rounding, not bit for bit.
// KW is K rounded up to one of FeatureWidths (one pass over all channels: a second pass over a channel group would repeat
// both walks and the six record sums; DESIGN.md has the resources of each width).  Rows of s_feat past K are zeros.
//
// k_surfel_features<KW, PX>, k_surfel_features_backward<KW, PX>   (cfg->footprint = SPLAT_FOOTPRINT_SURFEL)
//   The same two kernels over surfel_walk.h's SurfEntry / surf_alpha<PX>: the whole disc record's alpha, (u, v) = B d / (1 - q.d),
//   so the map carries the surfel image's own weights.  The backward sums 9 + KW numbers per touched entry: the record's eight
//   columns (surfel.hip's formulas), the opacity, then w_i G_F[k].  A second pair of kernels rather than a flag on the first: the
//   ellipsoid's instantiations are untouched by construction.
#include "common.h"
#include "variant.h"
#include "disc.h"
#include "composite.h"
#include "composite_walk.h"
#include "surfel_walk.h"
#include "wave_reduce.h"

namespace {

// the numbers the backward sums per (entry, pixel) before the channels, in the order of an entry's row in LDS
constexpr uint32_t FSUM_CX = 0, FSUM_CY = 1, FSUM_B00 = 2, FSUM_B01 = 3, FSUM_B11 = 4; // -> grad_records
constexpr uint32_t FSUM_OPACITY = 5;                                                     // -> grad_color_opacity column 3
constexpr int FNV = 6;                                                                   // then w G_F[k] -> grad_features
constexpr uint32_t FREC_ROW = 8, FREC_B11 = 5, FCOLOR_ROW = 4, FCOLOR_OPACITY = 3;
// the surfel backward's: the record's eight columns in order, then the opacity, then w G_F[k]
constexpr uint32_t SFSUM_OPACITY = 8;
constexpr int SFNV = 9;

// the instantiated widths: the smallest one >= channels is launched
using FeatureWidths = OneOf<1, 2, 3, 4, 6, 8, 12, 16, 24, 32>;
constexpr int FEATURE_WIDTHS[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
static_assert(FEATURE_WIDTHS[9] == SPLAT_MAX_FEATURE_CHANNELS, "the widest instantiation is the ABI's limit");

// the frame (BackParams; grad_img is not read) and the feature arguments of both kernels
struct FeatParams : BackParams {
    const float *features; uint32_t feature_stride, channels;
    float *out;            // forward: W H channels
    const float *grad_out; // backward: W H channels
    float *grad_features; uint32_t grad_feature_stride;
};

// the feature rows of entries [c0, c0 + m) of the tile's list, gathered by index (all threads; the index is read from the
// list again, so that no barrier is needed between this and stage_chunk)
template <int KW>
__device__ __forceinline__ void stage_features(const FeatParams &p, uint32_t off, uint32_t c0, uint32_t m, float (*s_feat)[KW]) {
    for (uint32_t q = threadIdx.x; q < m * KW; q += 256) {
        const uint32_t e = q / KW, k = q - e * KW;
        const size_t idx = p.indices[off + c0 + e];
        s_feat[e][k] = k < p.channels ? p.features[idx * p.feature_stride + k] : 0.0f;
    }
}

} // namespace

template <int KW, bool PX>
__global__ __launch_bounds__(256) void k_composite_features(FeatParams p) {
    __shared__ GradEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_feat[GCH][KW];

    TILE_PIXEL_PROLOGUE(p);

    bool live = pixel_ok;
    float T = 1.0f;
    float acc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = 0.0f;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        stage_features<KW>(p, off, c0, m, s_feat);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, dx, dy;
                const bool in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
                const float wgt = blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if (in) {
#pragma unroll
                    for (int k = 0; k < KW; ++k) acc[k] += wgt * s_feat[j][k];
                }
                if (T <= T_STOP) {
                    live = false;
                    break;
                }
            }
        }
        if (!__syncthreads_or(live)) break;
    }
    if (pixel_ok) {
        float *dst = p.out + ((size_t)py * p.width + px) * p.channels;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            if ((uint32_t)k < p.channels) dst[k] = acc[k];
        }
    }
}

template <int KW, bool PX>
__global__ __launch_bounds__(256) void k_composite_features_backward(FeatParams p) {
    constexpr int NV = FNV + KW;
    __shared__ GradEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_feat[GCH][KW];
    __shared__ float s_part[4][GCH][NV];
    __shared__ uint32_t s_touch[GCH];
    __shared__ uint32_t s_maxL;

    TILE_PIXEL_PROLOGUE(p);

    // ---- walk 1: front to back, the forward's stop rule (k_composite_backward's) ----
    bool live = pixel_ok;
    uint32_t L = 0;
    float T = 1.0f, T_last = 1.0f; // T_L, T_{L-1}
    if (tid == 0) s_maxL = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, dx, dy;
                const bool in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
                T_last = T;
                (void)blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if (T <= T_STOP) {
                    L = c0 + j + 1;
                    live = false;
                    break;
                }
            }
        }
        if (!__syncthreads_or(live)) break;
    }
    if (live) L = count; // never stopped: the whole list (T_last is the T before its last entry)
    if (L) atomicMax(&s_maxL, L);

    float G[KW]; // dL/dF of the pixel; zeros off the screen and past K
#pragma unroll
    for (int k = 0; k < KW; ++k) G[k] = 0.0f;
    if (pixel_ok) {
        const float *src = p.grad_out + ((size_t)py * p.width + px) * p.channels;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            if ((uint32_t)k < p.channels) G[k] = src[k];
        }
    }
    float S = 0.0f; // the blend of everything behind the entry: every feature's background is 0
    float Tn = T;   // T_{i+1} on the way back
    __syncthreads();
    const uint32_t maxL = s_maxL;

    // ---- walk 2: back to front from the tile's largest L ----
    for (uint32_t cend = maxL; cend > 0;) {
        const uint32_t c0 = cend > GCH ? cend - GCH : 0, m = cend - c0;
        __syncthreads(); // the previous chunk's sums are added
        stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        stage_features<KW>(p, off, c0, m, s_feat);
        if (tid < GCH) s_touch[tid] = 0;
        __syncthreads();
        for (int j = (int)m - 1; j >= 0; --j) {
            const uint32_t i = c0 + (uint32_t)j;
            float alpha = 0.0f, ge = 0.0f, u = 0.0f, v = 0.0f, dx = 0.0f, dy = 0.0f;
            bool in = false;
            if (i < L) in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
            const unsigned long long hit = __ballot(in);
            if (hit == 0) {
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) s_part[w][j][k] = 0.0f;
                }
                continue;
            }
            float vals[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) vals[k] = 0.0f;
            if (in) {
                const GradEntry &e = s_ent[j];
                const float Ti = (i + 1 == L) ? T_last : Tn / (1.0f - alpha);
                float s = 0.0f; // G_F . f_i
#pragma unroll
                for (int k = 0; k < KW; ++k) s += G[k] * s_feat[j][k];
                const float dA = Ti * (s - S);
                const float wgt = Ti * alpha;
#pragma unroll
                for (int k = 0; k < KW; ++k) vals[FNV + k] = wgt * G[k];
                vals[FSUM_OPACITY] = ge * dA;
                const float dd2 = -4.5f * alpha * dA;
                const float du = 2.0f * u * dd2, dv = 2.0f * v * dd2;
                vals[FSUM_CX] = -du * e.a.z;               // d2 / c.x
                vals[FSUM_CY] = -(du * e.a.w + dv * e.b.x); // d2 / c.y
                vals[FSUM_B00] = du * dx;                   // d2 / B00
                vals[FSUM_B01] = du * dy;                   // d2 / B01
                vals[FSUM_B11] = dv * dy;                   // d2 / B11
                S = alpha * s + (1.0f - alpha) * S;
                Tn = Ti;
            } else if (i + 1 == L) {
                Tn = T_last;
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) vals[k] = wave_sum63(vals[k]);
            if (lane == 63) {
#pragma unroll
                for (int k = 0; k < NV; ++k) s_part[w][j][k] = vals[k];
                s_touch[j] = 1;
            }
        }
        __syncthreads();
        // one atomic add per touched (entry, number); the numbers of the channels past K have no word
        for (uint32_t q = tid; q < m * NV; q += 256) {
            const uint32_t e = q / NV, k = q - e * NV;
            if (!s_touch[e] || k >= FNV + p.channels) continue;
            const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
            const size_t idx = s_idx[e];
            float *dst = k < FSUM_OPACITY ? p.grad_records + idx * FREC_ROW + (k < FSUM_B11 ? k : FREC_B11)
                         : k == FSUM_OPACITY ? p.grad_color + idx * FCOLOR_ROW + FCOLOR_OPACITY
                                             : p.grad_features + idx * p.grad_feature_stride + (k - FNV);
            atomicAdd(dst, sum);
        }
        cend = c0;
    }
}

// The surfel footprint's pair (file header): k_composite_features / _backward with SurfEntry and surf_alpha<PX>.
template <int KW, bool PX>
__global__ __launch_bounds__(256) void k_surfel_features(FeatParams p) {
    __shared__ SurfEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_feat[GCH][KW];

    TILE_PIXEL_PROLOGUE(p);
    (void)tid, (void)lane, (void)w, (void)tile_idx;

    bool live = pixel_ok;
    float T = 1.0f;
    float acc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[k] = 0.0f;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        surf_stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        stage_features<KW>(p, off, c0, m, s_feat);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, rd, dx, dy;
                const bool in = surf_alpha<PX>(s_ent[j], pxf, pyf, alpha, ge, u, v, rd, dx, dy);
                const float wgt = surf_blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if (in) {
#pragma unroll
                    for (int k = 0; k < KW; ++k) acc[k] += wgt * s_feat[j][k];
                }
                if (T <= T_STOP) {
                    live = false;
                    break;
                }
            }
        }
        if (!__syncthreads_or(live)) break;
    }
    if (pixel_ok) {
        float *dst = p.out + ((size_t)py * p.width + px) * p.channels;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            if ((uint32_t)k < p.channels) dst[k] = acc[k];
        }
    }
}

template <int KW, bool PX>
__global__ __launch_bounds__(256) void k_surfel_features_backward(FeatParams p) {
    constexpr int NV = SFNV + KW;
    __shared__ SurfEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_feat[GCH][KW];
    __shared__ float s_part[4][GCH][NV];
    __shared__ uint32_t s_touch[GCH];
    __shared__ uint32_t s_maxL;

    TILE_PIXEL_PROLOGUE(p);
    (void)tile_idx;

    // ---- walk 1: front to back, the forward's stop rule ----
    bool live = pixel_ok;
    uint32_t L = 0;
    float T = 1.0f, T_last = 1.0f; // T_L, T_{L-1}
    if (tid == 0) s_maxL = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        surf_stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, rd, dx, dy;
                const bool in = surf_alpha<PX>(s_ent[j], pxf, pyf, alpha, ge, u, v, rd, dx, dy);
                T_last = T;
                (void)surf_blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if (T <= T_STOP) {
                    L = c0 + j + 1;
                    live = false;
                    break;
                }
            }
        }
        if (!__syncthreads_or(live)) break;
    }
    if (live) L = count; // never stopped: the whole list (T_last is the T before its last entry)
    if (L) atomicMax(&s_maxL, L);

    float G[KW]; // dL/dF of the pixel; zeros off the screen and past K
#pragma unroll
    for (int k = 0; k < KW; ++k) G[k] = 0.0f;
    if (pixel_ok) {
        const float *src = p.grad_out + ((size_t)py * p.width + px) * p.channels;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            if ((uint32_t)k < p.channels) G[k] = src[k];
        }
    }
    float S = 0.0f; // the blend of everything behind the entry: every feature's background is 0
    float Tn = T;   // T_{i+1} on the way back
    __syncthreads();
    const uint32_t maxL = s_maxL;

    // ---- walk 2: back to front from the tile's largest L ----
    for (uint32_t cend = maxL; cend > 0;) {
        const uint32_t c0 = cend > GCH ? cend - GCH : 0, m = cend - c0;
        __syncthreads(); // the previous chunk's sums are added
        surf_stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        stage_features<KW>(p, off, c0, m, s_feat);
        if (tid < GCH) s_touch[tid] = 0;
        __syncthreads();
        for (int j = (int)m - 1; j >= 0; --j) {
            const uint32_t i = c0 + (uint32_t)j;
            float alpha = 0.0f, ge = 0.0f, u = 0.0f, v = 0.0f, rd = 0.0f, dx = 0.0f, dy = 0.0f;
            bool in = false;
            if (i < L) in = surf_alpha<PX>(s_ent[j], pxf, pyf, alpha, ge, u, v, rd, dx, dy);
            const unsigned long long hit = __ballot(in);
            if (hit == 0) {
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < NV; ++k) s_part[w][j][k] = 0.0f;
                }
                continue;
            }
            float vals[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) vals[k] = 0.0f;
            if (in) {
                const SurfEntry &e = s_ent[j];
                const float Ti = (i + 1 == L) ? T_last : Tn / (1.0f - alpha);
                float s = 0.0f; // G_F . f_i
#pragma unroll
                for (int k = 0; k < KW; ++k) s += G[k] * s_feat[j][k];
                const float dA = Ti * (s - S);
                const float wgt = Ti * alpha;
#pragma unroll
                for (int k = 0; k < KW; ++k) vals[SFNV + k] = wgt * G[k];
                vals[SFSUM_OPACITY] = ge * dA;
                const float dd2 = -4.5f * alpha * dA;
                const float du = 2.0f * u * dd2, dv = 2.0f * v * dd2;
                const float dur = du * rd, dvr = dv * rd;
                const float gq = (du * u + dv * v) * rd; // d / d(q.d)
                vals[0] = -(dur * (e.a.z + u * e.b.z) + dvr * (e.b.x + v * e.b.z)); // c.x
                vals[1] = -(dur * (e.a.w + u * e.b.w) + dvr * (e.b.y + v * e.b.w)); // c.y
                vals[2] = dur * dx; // B00
                vals[3] = dur * dy; // B01
                vals[4] = dvr * dx; // B10
                vals[5] = dvr * dy; // B11
                vals[6] = gq * dx;  // q0
                vals[7] = gq * dy;  // q1
                S = alpha * s + (1.0f - alpha) * S;
                Tn = Ti;
            } else if (i + 1 == L) {
                Tn = T_last;
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) vals[k] = wave_sum63(vals[k]);
            if (lane == 63) {
#pragma unroll
                for (int k = 0; k < NV; ++k) s_part[w][j][k] = vals[k];
                s_touch[j] = 1;
            }
        }
        __syncthreads();
        // one atomic add per touched (entry, number); the numbers of the channels past K have no word
        for (uint32_t q = tid; q < m * NV; q += 256) {
            const uint32_t e = q / NV, k = q - e * NV;
            if (!s_touch[e] || k >= SFNV + p.channels) continue;
            const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
            const size_t idx = s_idx[e];
            float *dst = k < SFSUM_OPACITY ? p.grad_records + idx * FREC_ROW + k
                         : k == SFSUM_OPACITY ? p.grad_color + idx * FCOLOR_ROW + FCOLOR_OPACITY
                                              : p.grad_features + idx * p.grad_feature_stride + (k - SFNV);
            atomicAdd(dst, sum);
        }
        cend = c0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {

// splat_composite_features and its backward: the frame, the feature rows, and the map (forward) or the map's gradient and the
// three gradient planes (backward)
struct FeatureArgs : FrameArgs {
    const void *features_f32;
    uint32_t feature_stride_floats, channels;
    void *out_f32;
    const void *grad_out_f32;
    void *grad_records, *grad_color_opacity, *grad_features_f32;
    uint32_t grad_feature_stride_floats;
    bool backward;

    int launch(splat_ctx *ctx) const {
        FeatParams p{};
        uint32_t nty = 0;
        const bool surfel = cfg && cfg->footprint == SPLAT_FOOTPRINT_SURFEL; // (the surfel pair: the whole record's alpha)
        const int rc_setup = setup(ctx, backward ? "splat_composite_features_backward" : "splat_composite_features", p, nty, surfel);
        if (rc_setup != SPLAT_OK) return rc_setup;
        ARG_CHECK(ctx, channels >= 1 && channels <= SPLAT_MAX_FEATURE_CHANNELS && feature_stride_floats >= channels);
        ARG_CHECK(ctx, color_opacity && records && tile_indices && tile_counts && tile_offsets && (n == 0 || features_f32));
        ARG_CHECK(ctx, (((uintptr_t)color_opacity | (uintptr_t)records) & 15) == 0);
        ARG_CHECK(ctx, (((uintptr_t)tile_indices | (uintptr_t)tile_counts | (uintptr_t)tile_offsets | (uintptr_t)features_f32) & 3) == 0);
        if (backward) {
            ARG_CHECK(ctx, grad_out_f32 && grad_feature_stride_floats >= channels);
            ARG_CHECK(ctx, n == 0 || (grad_records && grad_color_opacity && grad_features_f32));
            ARG_CHECK(ctx, (((uintptr_t)grad_records | (uintptr_t)grad_color_opacity) & 15) == 0);
            ARG_CHECK(ctx, (((uintptr_t)grad_out_f32 | (uintptr_t)grad_features_f32) & 3) == 0);
        } else {
            ARG_CHECK(ctx, out_f32 && ((uintptr_t)out_f32 & 3) == 0);
        }
        if (n == 0) { // no splat: every list is empty
            if (!backward) HIP_TRY(ctx, hipMemsetAsync(out_f32, 0, (size_t)width * height * channels * sizeof(float), ctx->stream));
            return SPLAT_OK;
        }
        p.features = (const float *)features_f32;
        p.feature_stride = feature_stride_floats;
        p.channels = channels;
        p.out = (float *)out_f32;
        p.grad_out = (const float *)grad_out_f32;
        p.grad_records = (float *)grad_records;
        p.grad_color = (float *)grad_color_opacity;
        p.grad_features = (float *)grad_features_f32;
        p.grad_feature_stride = grad_feature_stride_floats;
        int kw = 0;
        for (const int wdt : FEATURE_WIDTHS) {
            if ((uint32_t)wdt >= channels) {
                kw = wdt;
                break;
            }
        }
        const bool launched = variant_dispatch([&](auto kwc, auto px, auto back, auto surf) {
            if constexpr (surf.value && back.value)
                launch_kernel(ctx, NO_STAGE, k_surfel_features_backward<kwc.value, px.value>, dim3(p.ntx, nty), dim3(256), p);
            else if constexpr (surf.value) launch_kernel(ctx, NO_STAGE, k_surfel_features<kwc.value, px.value>, dim3(p.ntx, nty), dim3(256), p);
            else if constexpr (back.value) launch_kernel(ctx, NO_STAGE, k_composite_features_backward<kwc.value, px.value>, dim3(p.ntx, nty), dim3(256), p);
            else launch_kernel(ctx, NO_STAGE, k_composite_features<kwc.value, px.value>, dim3(p.ntx, nty), dim3(256), p);
            return true;
        }, FeatureWidths{kw}, composite_uses_px(ctx, p.ntx, nty), backward, surfel);
        if (!launched) return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_composite_features: no kernel of this width");
        return launch_check(ctx, backward ? "launch k_composite_features_backward" : "launch k_composite_features");
    }
};

} // namespace

extern "C" int splat_composite_features(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                        const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                        uint32_t width, uint32_t height, const void *features_f32, uint32_t feature_stride_floats,
                                        uint32_t channels, uint32_t n, void *out_f32) {
    FeatureArgs a{};
    FRAME_ARGS(a);
    a.features_f32 = features_f32, a.feature_stride_floats = feature_stride_floats, a.channels = channels;
    a.out_f32 = out_f32;
    return a.launch(ctx);
}

extern "C" int splat_composite_features_backward(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                                 uint32_t color_stride_vec4, const void *records, const void *tile_indices,
                                                 const void *tile_counts, const void *tile_offsets, uint32_t width, uint32_t height,
                                                 const void *features_f32, uint32_t feature_stride_floats, uint32_t channels,
                                                 const void *grad_out_f32, uint32_t n, void *grad_records, void *grad_color_opacity,
                                                 void *grad_features_f32, uint32_t grad_feature_stride_floats) {
    FeatureArgs a{};
    FRAME_ARGS(a);
    a.features_f32 = features_f32, a.feature_stride_floats = feature_stride_floats, a.channels = channels;
    a.grad_out_f32 = grad_out_f32, a.grad_records = grad_records, a.grad_color_opacity = grad_color_opacity;
    a.grad_features_f32 = grad_features_f32, a.grad_feature_stride_floats = grad_feature_stride_floats;
    a.backward = true;
    return a.launch(ctx);
}
