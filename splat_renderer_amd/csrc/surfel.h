// surfel.h — the 2D Gaussian surfel footprint (SPLAT_FOOTPRINT_SURFEL; an extension, no reference counterpart; 2DGS, Huang et
// al. 2024): one splat = centre p, two standard deviations s.x, s.y (world units; s.z, s.w ignored) along the tangent axes
// R[:,0], R[:,1] of a rotation quaternion (w, x, y, z); its normal is R[:,2].
//
// A surfel is a planar quad with half-axes e0 = 3 s.x R[:,0], e1 = 3 s.y R[:,1], so its record is the oriented disc's
// (disc.h: disc_record_axes, the same clip-space rows, cull and 8 floats {c.x, c.y, B00, B01, B10, B11, q0, q1}), the record's
// unit circle is the 3-sigma cut and the Gaussian is g = exp(-4.5 (u^2 + v^2)) — the ellipsoid's exponent scale
// (composite.h: ELLIPSOID_EXP2_SCALE), so the ellipsoid's forward composites draw surfel records as they are.  (u, v) =
// B d / (1 - q.d) is the exact ray-surfel intersection in the surfel's own coordinates (no affine approximation), and
// with c = VP [P; 1] for the plane point P = p + u e0 + v e1 a pixel sees, c.w = cw / (1 - q.d), cw the centre's clip w:
// the depth of the intersection costs one number per splat beside the record.
//
// Operation order (tests/surfel_ref.py restates it; one IEEE binary32 rounding per operator, no contraction):
//   quaternion   n2 = ((w w + x x) + y y) + z z,  k = 1 / sqrt(n2),  (w, x, y, z) *= k          (ellipsoid.h's)
//   R            R00 = 1 - 2 (y y + z z), R10 = 2 (x y + w z), R20 = 2 (x z - w y)
//                R01 = 2 (x y - w z),     R11 = 1 - 2 (x x + z z), R21 = 2 (y z + w x)
//   half-axes    a0 = 3 s.x, a1 = 3 s.y;  e0 = R[:,0] a0,  e1 = R[:,1] a1
//   record       disc_record_axes(m, w, h, p, e0, e1): culled (all zeros) when a corner of the quad has w <= 0, when det == 0
//                (edge-on, a zero scale) and when anything is not finite (a zero quaternion: k = inf, 0 inf = NaN)
// cw (optional): the centre's clip w where the record is kept, 0 where it is culled.
//
// Depth distortion (surfel.hip: k_surfel_depth<PX, DIST>, k_surfel_backward<DEPTH, PX, DIST>; 2DGS's term): per pixel
// Dist = sum_{i > j} w_i w_j (m_i - m_j)^2 over the consumed entries inside the cut whose t = z rd is finite and > 0 (the
// others draw the image and take no part), m = far (t - near) / ((far - near) t) = ka - c / t, ka = far / (far - near),
// c = near ka.  The term depends on differences of m only, and a sum of m's near 1 cancels in binary32 (W Q - M^2 and the
// unshifted prefix sums lose four digits), so every m is taken relative to the pixel's first participating entry, and ka is
// dropped before anything is rounded: m'_i = m_i - m_first = c (1 / t_first - 1 / t_i).
// Operation order (tests/surfel_distortion_ref.py restates it; one binary32 rounding per operator, no contraction; rcp is the
// hardware's reciprocal, a division in the restatement):
//   host         c = near when far = +inf, else the binary32 nearest to near far / (far - near) formed in binary64
//   per entry    t = z rd,  rt = rcp(t),  rt0 = rt of the first participating entry,  m' = c (rt0 - rt),  mm = m' m'
//                d = (mm A + Q) - (2 m') M,  Dist = Dist + w d,  A = A + w,  M = M + w m',  Q = Q + w mm
// with A = M = Q = Dist = 0 before the first entry and w the image's own weight (surfel_walk.h).
#pragma once
#include "disc.h"

// The distortion sums one pixel carries front to back (the order above), and one participating entry's step.
struct SurfDist {
    float dist = 0.0f, A = 0.0f, M = 0.0f, Q = 0.0f;
    float rt0 = -1.0f; // (negative: no entry has participated yet; a participating rt is >= 0)
};

__device__ __forceinline__ bool surf_dist_participates(float t) { return t > 0.0f && t < __builtin_inff(); }

// m' of an entry at depth t against the pixel's first (rt0 < 0: this is the first, and becomes it)
__device__ __forceinline__ float surf_dist_m(float c, float t, float &rt0, float &rt) {
#pragma clang fp contract(off)
    rt = __builtin_amdgcn_rcpf(t);
    if (rt0 < 0.0f) rt0 = rt;
    return c * (rt0 - rt);
}

__device__ __forceinline__ void surf_dist_step(SurfDist &s, float c, float t, float w) {
#pragma clang fp contract(off)
    float rt;
    const float mp = surf_dist_m(c, t, s.rt0, rt);
    const float mm = mp * mp;
    const float d = (mm * s.A + s.Q) - (2.0f * mp) * s.M;
    s.dist = s.dist + w * d;
    s.A = s.A + w;
    s.M = s.M + w * mp;
    s.Q = s.Q + w * mm;
}

__device__ __forceinline__ DiscRecord surfel_record(const float *m, float w, float h, float4 p, float4 s, float4 q, float *cw = nullptr) {
#pragma clang fp contract(off)
    if (cw) *cw = 0.0f;
    const float n2 = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    const float k = 1.0f / sqrtf(n2);
    const float qr = q.x * k, qx = q.y * k, qy = q.z * k, qz = q.w * k;
    const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r10 = 2.0f * (qx * qy + qr * qz), r20 = 2.0f * (qx * qz - qr * qy);
    const float r01 = 2.0f * (qx * qy - qr * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r21 = 2.0f * (qy * qz + qr * qx);
    const float a0 = 3.0f * s.x, a1 = 3.0f * s.y;
    return disc_record_axes(m, w, h, p, r00 * a0, r10 * a0, r20 * a0, r01 * a1, r11 * a1, r21 * a1, cw);
}
