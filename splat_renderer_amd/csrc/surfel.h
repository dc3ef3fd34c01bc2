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
#pragma once
#include "disc.h"

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
