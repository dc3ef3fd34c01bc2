// ellipsoid.h — the anisotropic 3D Gaussian footprint (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference counterpart):
// one splat = centre p, per-axis standard deviations s (world units) and a rotation quaternion (w, x, y, z).
//
// Its screen footprint is the EWA one of 3D Gaussian splatting: Sigma2 = J Sigma3 J^T + 0.3 I (px^2), J the exact
// derivative at the centre of the projector's own screen map to_screen() (project.hip), cut at 3 sigma.  It is written
// as a disc record (disc.h) with q = 0:
//      {c.x, c.y, B00, B01, 0, B11, 0, 0},   B = U / 3,   U upper-triangular with U^T U = Sigma2^-1
// so u^2 + v^2 = |B d|^2 = d^T Sigma2^-1 d / 9 and the disc composite's "inside when u^2 + v^2 <= 1" is the 3-sigma cut;
// only the exponent scale differs (composite.h: ELLIPSOID_EXP2_SCALE).  disc_bounds() of such a record is the exact
// 3-sigma box c -/+ 3 sqrt(Sigma2_xx), c -/+ 3 sqrt(Sigma2_yy).
//
// Operation order (tests/ellipsoid_ref.py restates it; one IEEE binary32 rounding per operator, no contraction):
//   quaternion   n2 = ((w w + x x) + y y) + z z,  k = 1 / sqrt(n2),  (w, x, y, z) *= k
//   R            the usual rotation matrix of a unit quaternion, e.g. R00 = 1 - 2 (y y + z z), R01 = 2 (x y - w z)
//   M = R S      M_ij = R_ij s_j                                  (Sigma3 = M M^T, never formed)
//   clip         c = VP [p; 1] as to_screen(); culled unless c.w > 0
//   w reach      v = M^T m3 (m3 the w row of VP), culled unless c.w - 3 sqrt(|v|^2) > 0  (the 3-sigma ellipsoid stays in front)
//   centre       nx = c.x / c.w, ny = c.y / c.w, screen centre as to_screen()
//   J            J0k = (hw / c.w)(m_xk - nx m_wk),  J1k = (hh / c.w)(ny m_wk - m_yk)   (hw / c.w = hw * (1 / c.w))
//   T = J M      Sigma2 = T T^T + 0.3 I:  a = |T0|^2 + 0.3, b = T0.T1, c = |T1|^2 + 0.3
//   U            det = a c - b b (culled unless > 0);  U00 = sqrt(c / det), U01 = -b / sqrt(c det), U11 = 1 / sqrt(c)
//   B            U / 3 (three IEEE divides); culled when anything is not finite
// Sums of three are ((t0 + t1) + t2).  q and -q give the same bits (every product of two components keeps them), and so
// does 2q (scaling by a power of two is exact throughout the normalisation).
//
// <RHO = true> (the antialiased mode: splat_project_ellipsoid_aa and its backward) also hands out the 2D Mip filter's
// compensation factor, from the values above and in the same arithmetic:
//   a0 = |T0|^2, c0 = |T1|^2 (so a = a0 + 0.3, c = c0 + 0.3: the sums the record itself forms),  det0 = a0 c0 - b b
//   rho = det0 > 0 ? sqrt(det0 / det) : 0;  0 for every splat whose record is all zeros
// rho^2 = det(Sigma2 - 0.3 I) / det Sigma2: the dilated Gaussian drawn at opacity * rho deposits what the undilated one would.
// a >= a0 and c >= c0 in binary32 (adding 0.3 rounds monotonically) and the b b is the same number, so det >= det0 and
// rho <= 1 with no clamp.  det0 cancels on needle splats (a0 c0 and b b agree in their leading digits): rho is then 0 or
// carries few correct digits; the record does not read it.  Without RHO the function is the one it was.
#pragma once
#include "disc.h"

// The ellipsoid planes the projector reads beside the positions (vec4 per splat, *_stride float4s apart).
struct EllIO {
    const float4 *scales;   // sigma x, y, z (w ignored)
    uint32_t scale_stride;
    const float4 *rotations; // quaternion (w, x, y, z), any non-zero length
    uint32_t rot_stride;
};

template <bool RHO = false>
__device__ __forceinline__ DiscRecord ellipsoid_record(const float *m, float w, float h, float4 p, float4 s, float4 q, float *rho = nullptr) {
#pragma clang fp contract(off)
    if (RHO) *rho = 0.0f;
    DiscRecord zero = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
    const float n2 = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    const float k = 1.0f / sqrtf(n2);
    const float qr = q.x * k, qx = q.y * k, qy = q.z * k, qz = q.w * k;
    const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r01 = 2.0f * (qx * qy - qr * qz), r02 = 2.0f * (qx * qz + qr * qy);
    const float r10 = 2.0f * (qx * qy + qr * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r12 = 2.0f * (qy * qz - qr * qx);
    const float r20 = 2.0f * (qx * qz - qr * qy), r21 = 2.0f * (qy * qz + qr * qx), r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
    const float m00 = r00 * s.x, m01 = r01 * s.y, m02 = r02 * s.z;
    const float m10 = r10 * s.x, m11 = r11 * s.y, m12 = r12 * s.z;
    const float m20 = r20 * s.x, m21 = r21 * s.y, m22 = r22 * s.z;
    const float cx = ((m[0] * p.x + m[4] * p.y) + m[8] * p.z) + m[12];
    const float cy = ((m[1] * p.x + m[5] * p.y) + m[9] * p.z) + m[13];
    const float cw = ((m[3] * p.x + m[7] * p.y) + m[11] * p.z) + m[15];
    if (!(cw > 0.0f)) return zero;
    const float v0 = (m[3] * m00 + m[7] * m10) + m[11] * m20;
    const float v1 = (m[3] * m01 + m[7] * m11) + m[11] * m21;
    const float v2 = (m[3] * m02 + m[7] * m12) + m[11] * m22;
    if (!(cw - 3.0f * sqrtf((v0 * v0 + v1 * v1) + v2 * v2) > 0.0f)) return zero; // the 3-sigma ellipsoid reaches w = 0
    const float nx = cx / cw, ny = cy / cw;
    const float scx = ((nx + 1.0f) * 0.5f) * w, scy = ((1.0f - ny) * 0.5f) * h; // to_screen()
    const float icw = 1.0f / cw;
    const float ax = (0.5f * w) * icw, ay = (0.5f * h) * icw;
    const float j00 = ax * (m[0] - nx * m[3]), j01 = ax * (m[4] - nx * m[7]), j02 = ax * (m[8] - nx * m[11]);
    const float j10 = ay * (ny * m[3] - m[1]), j11 = ay * (ny * m[7] - m[5]), j12 = ay * (ny * m[11] - m[9]);
    const float t00 = (j00 * m00 + j01 * m10) + j02 * m20, t01 = (j00 * m01 + j01 * m11) + j02 * m21, t02 = (j00 * m02 + j01 * m12) + j02 * m22;
    const float t10 = (j10 * m00 + j11 * m10) + j12 * m20, t11 = (j10 * m01 + j11 * m11) + j12 * m21, t12 = (j10 * m02 + j11 * m12) + j12 * m22;
    const float a = ((t00 * t00 + t01 * t01) + t02 * t02) + 0.3f;
    const float b = (t00 * t10 + t01 * t11) + t02 * t12;
    const float c = ((t10 * t10 + t11 * t11) + t12 * t12) + 0.3f;
    const float det = a * c - b * b;
    if (!(det > 0.0f)) return zero; // (also NaN)
    const float b00 = sqrtf(c / det) / 3.0f, b01 = ((-b) / sqrtf(c * det)) / 3.0f, b11 = (1.0f / sqrtf(c)) / 3.0f;
    DiscRecord o;
    o.a = make_float4(scx, scy, b00, b01);
    o.b = make_float4(0.0f, b11, 0.0f, 0.0f);
    if (!disc_finite4(scx, scy, b00, b01) || !disc_finite4(b11, det, 0.0f, 0.0f)) return zero;
    if (RHO) { // (a0, c0: the sums a and c were formed from, the same bits)
        const float a0 = (t00 * t00 + t01 * t01) + t02 * t02, c0 = (t10 * t10 + t11 * t11) + t12 * t12;
        const float det0 = a0 * c0 - b * b;
        *rho = det0 > 0.0f ? sqrtf(det0 / det) : 0.0f;
    }
    return o;
}
