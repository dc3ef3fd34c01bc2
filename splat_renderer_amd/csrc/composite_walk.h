// composite_walk.h — what every per-tile kernel that replays a frame of anisotropic 3D Gaussians shares (composite_grad.hip:
// the composite's backward and the contribution scores; composite_features.hip: the feature channels and their backward):
// one 256-thread workgroup per 16x16 tile, one pixel per lane in k_composite's 8x8 quadrants (TILE_PIXEL_PROLOGUE); the tile's
// list staged in LDS GCH entries at a time (stage_chunk); an entry's alpha at a pixel (entry_alpha); the transmittance update
// and the weight w = T alpha (blend_step<PX>).  <PX = false> is k_composite's T -= T (g o), <PX = true> k_composite_px's
// T = fma(-o, T g, T): they round differently, and where T lands within an ulp or two of T_STOP they stop a pixel at
// different entries, so the update is written once and every kernel calls it.  A file that includes this is compiled with
// contraction on, as composite.hip is.  FrameArgs: the frame arguments, checks and kernel parameters of their entry points.
#pragma once
#include <string>

#include "common.h"
#include "disc.h"
#include "composite.h"

namespace {

constexpr int GT = 16;          // tile edge
constexpr int GCH = 64;         // list entries per staged chunk

struct GradEntry {
    float4 a;   // c.x, c.y, B00, B01
    float4 b;   // B11, opacity, r, g
    float4 c;   // b, z (DEPTH; else 0), -, -
    float4 bnd; // the record's exact 3-sigma box (all zeros: covers no pixel)
};

struct BackParams {
    const float4 *color; uint32_t color_stride;
    const float4 *records;
    const uint32_t *indices, *counts, *offsets;
    uint32_t width, height, ntx;
    const float4 *grad_img;
    float *grad_records;
    float *grad_color;
};

// stages entries [c0, c0 + m) of the tile's list (threads 0 .. m-1)
template <bool DEPTH, typename P>
__device__ __forceinline__ void stage_chunk(const P &p, uint32_t off, uint32_t c0, uint32_t m, GradEntry *s_ent, uint32_t *s_idx) {
    const uint32_t t = threadIdx.x;
    if (t < m) {
        const uint32_t idx = p.indices[off + c0 + t];
        const DiscRecord rec = {p.records[(size_t)idx * 2], p.records[(size_t)idx * 2 + 1]};
        float4 bnd;
        const bool ok = disc_bounds(rec, bnd); // all zeros when not: no pixel centre (>= 0.5) is inside
        const float4 col = p.color[(size_t)idx * p.color_stride];
        GradEntry e;
        e.a = rec.a;
        e.b = make_float4(rec.b.y, col.w, col.x, col.y);
        if constexpr (DEPTH) e.c = make_float4(col.z, p.z[(size_t)idx * p.z_stride], 0.0f, 0.0f);
        else e.c = make_float4(col.z, 0.0f, 0.0f, 0.0f);
        e.bnd = ok ? bnd : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_ent[t] = e;
        s_idx[t] = idx;
    }
}

// alpha of entry e at pixel centre (pxf, pyf) in k_composite's operation order (ELL, q = 0: rd = 1); ge = the exponential,
// d2, u, v and the pixel offset returned for the backward.  Outside the box or the cut: false.
__device__ __forceinline__ bool entry_alpha(const GradEntry &e, float pxf, float pyf, float &alpha, float &ge, float &u, float &v, float &dx,
                                            float &dy) {
    const bool in_box = !(pxf < e.bnd.x || pxf > e.bnd.z || pyf < e.bnd.y || pyf > e.bnd.w);
    dx = pxf - e.a.x;
    dy = pyf - e.a.y;
    u = e.a.z * dx + e.a.w * dy;
    v = e.b.x * dy; // (B10 = 0: the forward's 0 dx + B11 dy, the same value for a finite dx)
    const float d2 = u * u + v * v;
    ge = (d2 <= 1.0f) ? __builtin_amdgcn_exp2f(d2 * ELLIPSOID_EXP2_SCALE) : 0.0f;
    alpha = ge;
    alpha *= e.b.y;
    return in_box && d2 <= 1.0f;
}

// One forward step of a pixel over entry e (entry_alpha's in, alpha, ge): T becomes the transmittance behind the entry, and the
// entry's blend weight w = T alpha is returned.  The only place the two drawing kernels' update orders are written; a pixel
// stops once T <= T_STOP.
template <bool PX>
__device__ __forceinline__ float blend_step(const GradEntry &e, bool in, float alpha, float ge, float &T) {
    float wgt;
    if constexpr (PX) { // k_composite_px: the colour premultiplied by the opacity, w = T g, T = fma(-opacity, w, T)
        const float w = T * (in ? ge : 0.0f);
        wgt = w * e.b.y; // (its AOV's weight)
        T = __builtin_fmaf(-e.b.y, w, T);
    } else { // k_composite: alpha = g opacity, w = T alpha, T -= w
        const float g = in ? alpha : 0.0f;
        wgt = T * g;
        T -= wgt;
    }
    return wgt;
}

} // namespace

// The prologue of the tile kernels, declared in the kernel's own scope: the thread's wave w (the tile's 8x8 quadrant,
// k_composite's pixel mapping) and lane, its tile and the tile's list, its pixel, whether that is on the screen, and the
// pixel's centre.  (A macro: the same lines returned from a function as a struct moved two loop-invariant compares of
// k_composite_contribution into its chunk loop.)
#define TILE_PIXEL_PROLOGUE(p)                                                                                        \
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;                                                  \
    const uint32_t tx = blockIdx.x, ty = blockIdx.y;                                                                  \
    const uint32_t tile_idx = ty * (p).ntx + tx;                                                                      \
    const uint32_t count = (p).counts[tile_idx], off = (p).offsets[tile_idx];                                         \
    const uint32_t px = tx * GT + (w & 1) * 8 + (lane & 7), py = ty * GT + (w >> 1) * 8 + (lane >> 3);                \
    const bool pixel_ok = px < (p).width && py < (p).height;                                                          \
    const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  The argument structs carry the names of include/splat.h's arguments, because the argument checks quote them; a
// field an entry point does not have stays NULL / 0.

namespace {

// The frame every family reads, and the checks and kernel parameters they share.
struct FrameArgs {
    const splat_composite_cfg *cfg;
    const void *color_opacity, *records, *tile_indices, *tile_counts, *tile_offsets;
    uint32_t color_stride_vec4, width, height, n;

    // The cfg restrictions (who: the family's name in their error), the screen limits, the whole screen's tile rows and the
    // colour stride; then the frame's part of p (its gradient pointers are the backward's to set) and the screen's tile rows.
    // surfel: the caller's kernels evaluate the whole record (surfel.hip) and take SPLAT_FOOTPRINT_SURFEL, and only it; every
    // other family refuses that footprint by name (its kernels take B10 = 0, q = 0: entry_alpha).
    int setup(splat_ctx *ctx, const char *who, BackParams &p, uint32_t &nty, bool surfel = false) const {
        if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
        ARG_CHECK(ctx, cfg != nullptr);
        if (cfg->footprint == SPLAT_FOOTPRINT_SURFEL && !surfel)
            return ctx_fail(ctx, SPLAT_ERR_INVALID,
                            (std::string(who) + ": not built for SPLAT_FOOTPRINT_SURFEL (this entry point's kernels take B10 = 0 and q = 0 "
                                                "of every record; a surfel's are not)").c_str());
        if (cfg->footprint != (surfel ? SPLAT_FOOTPRINT_SURFEL : SPLAT_FOOTPRINT_ELLIPSOID) || cfg->mode != SPLAT_COMPOSITE_FRONT_TO_BACK || cfg->early_out != 1 ||
            cfg->tile_size != GT || cfg->record_format != SPLAT_RECORDS_PROJECTED)
            return ctx_fail(ctx, SPLAT_ERR_INVALID,
                            (std::string(who) + (surfel ? ": footprint SURFEL" : ": footprint ELLIPSOID") +
                             ", FRONT_TO_BACK, early_out = 1, tile_size = 16 and PROJECTED records only").c_str());
        ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= 65535u * GT && height <= 65535u * GT);
        nty = div_up(height, GT);
        ARG_CHECK(ctx, cfg->tile_row0 == 0 && cfg->tile_row1 >= nty); // the whole screen: no strict band
        ARG_CHECK(ctx, color_stride_vec4 >= 1);
        p.color = (const float4 *)color_opacity;
        p.color_stride = color_stride_vec4;
        p.records = (const float4 *)records;
        p.indices = (const uint32_t *)tile_indices;
        p.counts = (const uint32_t *)tile_counts;
        p.offsets = (const uint32_t *)tile_offsets;
        p.width = width;
        p.height = height;
        p.ntx = div_up(width, GT);
        return SPLAT_OK;
    }
};

} // namespace

// surfel.hip: splat_composite_backward / _depth with cfg->footprint = SPLAT_FOOTPRINT_SURFEL (composite_grad.hip's two entry
// points hand their arguments over under include/splat.h's names; depth: the _depth entry point, with its four arguments)
struct SurfelBackwardCall {
    const splat_composite_cfg *cfg;
    const void *color_opacity, *records, *tile_indices, *tile_counts, *tile_offsets, *grad_rgba32f;
    uint32_t color_stride_vec4, width, height, n;
    void *grad_records, *grad_color_opacity;
    const void *depth_f32, *grad_depth_f32;
    uint32_t depth_stride_floats;
    void *grad_depth;
    bool depth;
    // splat_composite_backward_distortion (surfel.hip's own entry point; dist implies depth, and grad_depth_f32 may be NULL)
    float near, far;
    const void *grad_distortion_f32;
    bool dist;
};
int surfel_composite_backward(splat_ctx *ctx, const SurfelBackwardCall &c);

// The frame's arguments of every entry point, by name (their parameter names are FrameArgs' field names)
#define FRAME_ARGS(a)                                                                                                          \
    a.cfg = cfg, a.color_opacity = color_opacity, a.color_stride_vec4 = color_stride_vec4, a.records = records,                \
    a.tile_indices = tile_indices, a.tile_counts = tile_counts, a.tile_offsets = tile_offsets, a.width = width, a.height = height, a.n = n
