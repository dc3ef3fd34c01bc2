// surfel_walk.h — what the per-tile kernels that replay a frame of 2D Gaussian surfels share (surfel.hip: the composite's backward
// and the intersection depth; composite_features.hip: the feature channels and their backward): composite_walk.h's staging,
// alpha and transmittance step over the whole disc record.  A staged entry (SurfEntry) holds the eight record floats;
// surf_alpha<PX> is an entry's alpha at a pixel in the drawing kernel's operation order: den = fma(-q0, dx, fma(-q1, dy, 1)),
// rd = rcp(den), then k_composite's (u, v) = (B d) rd, d2 = u^2 + v^2, or k_composite_px's d2 = (|B d|^2) rd^2 (PX_DISC_ROW):
// they round differently once q != 0, and a pixel must stop at the entry its forward stopped at.  Included after
// composite_walk.h by a file compiled with contraction on.
#pragma once
#include "composite_walk.h"

namespace {

struct SurfEntry {
    float4 a;   // c.x, c.y, B00, B01
    float4 b;   // B10, B11, q0, q1
    float4 c;   // r, g, b, opacity
    float4 bnd; // the record's exact 3-sigma box (all zeros: covers no pixel)
    float4 d;   // z (DEPTH; else 0), -, -, -
};

template <bool DEPTH, typename P>
__device__ __forceinline__ void surf_stage_chunk(const P &p, uint32_t off, uint32_t c0, uint32_t m, SurfEntry *s_ent, uint32_t *s_idx) {
    const uint32_t t = threadIdx.x;
    if (t < m) {
        const uint32_t idx = p.indices[off + c0 + t];
        const DiscRecord rec = {p.records[(size_t)idx * 2], p.records[(size_t)idx * 2 + 1]};
        float4 bnd;
        const bool ok = disc_bounds(rec, bnd); // all zeros when not: no pixel centre (>= 0.5) is inside
        SurfEntry e;
        e.a = rec.a;
        e.b = rec.b;
        e.c = p.color[(size_t)idx * p.color_stride];
        e.bnd = ok ? bnd : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float z = 0.0f;
        if constexpr (DEPTH) z = p.z[(size_t)idx * p.z_stride];
        e.d = make_float4(z, 0.0f, 0.0f, 0.0f);
        s_ent[t] = e;
        s_idx[t] = idx;
    }
}

// (file header) ge = the exponential; u, v, rd and the pixel offset returned for the backward.  Outside the box or the cut: false.
template <bool PX>
__device__ __forceinline__ bool surf_alpha(const SurfEntry &e, float pxf, float pyf, float &alpha, float &ge, float &u, float &v, float &rd,
                                           float &dx, float &dy) {
    const bool in_box = !(pxf < e.bnd.x || pxf > e.bnd.z || pyf < e.bnd.y || pyf > e.bnd.w);
    dx = pxf - e.a.x;
    dy = pyf - e.a.y;
    rd = __builtin_amdgcn_rcpf(__builtin_fmaf(-e.b.z, dx, __builtin_fmaf(-e.b.w, dy, 1.0f))); // 1 / (1 - q.d)
    const float nu = e.a.z * dx + e.a.w * dy, nv = e.b.x * dx + e.b.y * dy;                    // B d
    u = nu * rd;
    v = nv * rd;
    float d2;
    if constexpr (PX) d2 = (nu * nu + nv * nv) * (rd * rd);
    else d2 = u * u + v * v;
    ge = (d2 <= 1.0f) ? __builtin_amdgcn_exp2f(d2 * ELLIPSOID_EXP2_SCALE) : 0.0f; // (NaN: outside)
    alpha = ge;
    alpha *= e.c.w;
    return in_box && d2 <= 1.0f;
}

// blend_step<PX> over a SurfEntry (composite_walk.h's reads the opacity from GradEntry::b.y)
template <bool PX>
__device__ __forceinline__ float surf_blend_step(const SurfEntry &e, bool in, float alpha, float ge, float &T) {
    GradEntry g;
    g.b.y = e.c.w;
    return blend_step<PX>(g, in, alpha, ge, T);
}

} // namespace
