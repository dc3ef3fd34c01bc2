// surfel.hip — replaying a frame of 2D Gaussian surfels (SPLAT_FOOTPRINT_SURFEL; surfel.h): the composite's backward with
// the whole disc record's alpha, the ray-surfel intersection depth map, and the projector's backward.  The forward image
// needs no kernel of its own (the ellipsoid's composites draw surfel records); what this file adds is everything that
// composite_walk.h's entry_alpha cannot replay, because it takes B10 = 0 and q = 0.
//
// The tile kernels keep composite_walk.h's shape: one 256-thread workgroup per 16x16 tile, TILE_PIXEL_PROLOGUE's pixel
// mapping, the list staged GCH entries at a time, blend_step<PX> for the transmittance (compiled with contraction on, as
// composite.hip is).  The staged entry (SurfEntry: the eight record floats instead of five), its staging and its alpha
// (surf_alpha<PX>) are surfel_walk.h's, shared with the feature channels' kernels (composite_features.hip).
// k_surfel_backward<DEPTH, PX>   k_composite_backward's two walks (composite_grad.hip's header).  Per consumed pair, with
//   dd2 = -4.5 alpha dL/dalpha, du = 2 u dd2, dv = 2 v dd2:
//     B00 += du rd dx   B01 += du rd dy   B10 += dv rd dx   B11 += dv rd dy   q_k += (du u + dv v) rd d_k
//     c.x -= rd (du (B00 + u q0) + dv (B10 + v q0))         c.y: the same with B01, B11, q1
//   DEPTH: the map is D = sum w z rd / sum w (z the caller's per-splat float, by default the centre's clip w: z rd is the clip w
//   of the point the pixel's ray meets the surfel at).  Its channel z rd - D joins cg with upstream G_D / sum w, and
//     z += w GDn rd     q_k += w GDn z rd^2 d_k     c_k -= w GDn z rd^2 q_k
//   Twelve numbers per entry (thirteen with DEPTH) go through the wave DPP tree and LDS, then one float atomic add per touched
//   (entry, number): reproducible to rounding.
//   DIST (with DEPTH): the depth-distortion map of surfel.h joins the same launch.  Walk 1 carries Dist, A, M, Q and rt0 in
//   surfel.h's order; with the pixel's totals W = A, Mb = M / W, and upstream G_Dist, an entry that participates has
//     dm = m' - Mb     e = W dm^2 + Dist / W (= sum_j w_j (m_i - m_j)^2, without the cancelling W m'^2 - 2 M m' + Q)
//   G_Dist e joins cg as one more colour channel with background 0, and through m_i, dm/dt = c / t^2,
//     gt = G_Dist 2 w W dm c rt^2
//   joins w GDn as dL / d(z rd).  m_first is a constant (the term is shift invariant).  grad_depth_img may be NULL: GDn = 0.
//   No number more than DEPTH's thirteen.
// k_surfel_depth<PX, DIST>   walk 1 alone: D (+inf where nothing contributed) and optionally alpha = 1 - T; DIST: the
//   distortion map too (0 where nothing participated), each of D and alpha optional.
// k_project_surfel_backward   one thread per splat, float64: surfel_record's chain reversed — the record's eight gradients and
//   the clip w's to position, scales x and y (z, w: exact zeros) and the quaternion through its normalisation.  The cull is
//   surfel_record's own (binary32): a culled surfel gets exact zeros.
#include "common.h"
#include "variant.h"
#include "disc.h"
#include "surfel.h"
#include "composite.h"
#include "composite_walk.h"
#include "surfel_walk.h"
#include "wave_reduce.h"

namespace {

// the numbers summed per (entry, pixel): 0-7 the record's columns in order, then colour and opacity, then (DEPTH) z
constexpr uint32_t SF_R = 8, SF_OPACITY = 11, SF_Z = 12;
constexpr int surf_nv(bool depth) { return depth ? 13 : 12; }

struct SurfDepthParams : BackParams {
    const float *z; uint32_t z_stride;
    const float *grad_depth_img;
    float *grad_depth;
    float *out_depth, *out_alpha; // (k_surfel_depth)
    // DIST: surfel.h's c, the map's upstream (k_surfel_backward) and the map (k_surfel_depth)
    float dist_c;
    const float *grad_dist_img;
    float *out_dist;
};

} // namespace

template <bool DEPTH, bool PX, bool DIST = false>
__global__ __launch_bounds__(256) void k_surfel_backward(SurfDepthParams p) {
    static_assert(DEPTH || !DIST, "the distortion's gradient reaches z and rd: DEPTH's numbers");
    constexpr int NV = surf_nv(DEPTH);
    __shared__ SurfEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_part[4][GCH][NV];
    __shared__ uint32_t s_touch[GCH];
    __shared__ uint32_t s_maxL;

    TILE_PIXEL_PROLOGUE(p);

    // ---- walk 1: front to back, the forward's stop rule ----
    bool live = pixel_ok;
    uint32_t L = 0;
    float T = 1.0f, T_last = 1.0f; // T_L, T_{L-1}
    float zw = 0.0f, ws = 0.0f;    // (DEPTH) sum w z rd, sum w over the consumed entries
    [[maybe_unused]] SurfDist ds;  // (DIST)
    if (tid == 0) s_maxL = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        surf_stage_chunk<DEPTH>(p, off, c0, m, s_ent, s_idx);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, rd, dx, dy;
                const bool in = surf_alpha<PX>(s_ent[j], pxf, pyf, alpha, ge, u, v, rd, dx, dy);
                T_last = T;
                [[maybe_unused]] const float wgt = surf_blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if constexpr (DEPTH) {
                    if (in) { // (outside the cut wgt is 0, and rd may be inf there: 0 inf)
                        zw += (s_ent[j].d.x * rd) * wgt;
                        ws += wgt;
                        if constexpr (DIST) {
                            const float t = s_ent[j].d.x * rd;
                            if (surf_dist_participates(t)) surf_dist_step(ds, p.dist_c, t, wgt);
                        }
                    }
                }
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

    const float4 G = pixel_ok ? p.grad_img[(size_t)py * p.width + px] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float S = (G.x * 0.05f + G.y * 0.05f) + G.z * 0.1f; // G . bg (the background's alpha and depth channels are 0)
    float D = 0.0f, GDn = 0.0f;                         // (DEPTH) D and G_D / ws; no gradient, and G_D not read, where nothing contributed
    if constexpr (DEPTH) {
        if (pixel_ok && ws > 0.0f) {
            D = zw / ws;
            if constexpr (DIST) GDn = p.grad_depth_img ? p.grad_depth_img[(size_t)py * p.width + px] / ws : 0.0f;
            else GDn = p.grad_depth_img[(size_t)py * p.width + px] / ws;
        }
    }
    // (DIST) G_Dist, W, M / W, Dist / W; G_Dist = 0, and not read, where nothing participated
    [[maybe_unused]] float GDist = 0.0f, dW = 0.0f, dMb = 0.0f, dDW = 0.0f;
    if constexpr (DIST) {
        if (pixel_ok && ds.A > 0.0f) {
            GDist = p.grad_dist_img[(size_t)py * p.width + px];
            dW = ds.A;
            dMb = ds.M / ds.A;
            dDW = ds.dist / ds.A;
        }
    }
    float Tn = T; // T_{i+1} on the way back
    __syncthreads();
    const uint32_t maxL = s_maxL;

    // ---- walk 2: back to front from the tile's largest L ----
    for (uint32_t cend = maxL; cend > 0;) {
        const uint32_t c0 = cend > GCH ? cend - GCH : 0, m = cend - c0;
        __syncthreads(); // the previous chunk's sums are added
        surf_stage_chunk<DEPTH>(p, off, c0, m, s_ent, s_idx);
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
                float cg = ((G.x * e.c.x + G.y * e.c.y) + G.z * e.c.z) + G.w; // G . (c, 1)
                if constexpr (DEPTH) cg += GDn * (e.d.x * rd - D);             // the centred depth channel
                const float wgt = Ti * alpha;
                [[maybe_unused]] float gt = 0.0f; // (DIST) dL / d(z rd) through m_i
                if constexpr (DIST) {
                    const float t = e.d.x * rd;
                    if (GDist != 0.0f && surf_dist_participates(t)) {
                        float rt;
                        const float dm = surf_dist_m(p.dist_c, t, ds.rt0, rt) - dMb;
                        cg += GDist * (dW * (dm * dm) + dDW);
                        gt = ((GDist * 2.0f) * (wgt * dW)) * (dm * ((p.dist_c * rt) * rt));
                    }
                }
                const float dA = Ti * (cg - S);
                vals[SF_R] = wgt * G.x;
                vals[SF_R + 1] = wgt * G.y;
                vals[SF_R + 2] = wgt * G.z;
                vals[SF_OPACITY] = ge * dA;
                const float dd2 = -4.5f * alpha * dA;
                const float du = 2.0f * u * dd2, dv = 2.0f * v * dd2;
                const float dur = du * rd, dvr = dv * rd;
                float gq = (du * u + dv * v) * rd; // d / d(q.d)
                float gcx = -(dur * (e.a.z + u * e.b.z) + dvr * (e.b.x + v * e.b.z));
                float gcy = -(dur * (e.a.w + u * e.b.w) + dvr * (e.b.y + v * e.b.w));
                if constexpr (DEPTH) {
                    float gz = wgt * GDn;          // dL / d(z rd)
                    if constexpr (DIST) gz += gt;
                    vals[SF_Z] = gz * rd;
                    const float grd = (gz * e.d.x) * (rd * rd); // d / d(q.d) through rd
                    gq += grd;
                    gcx -= grd * e.b.z;
                    gcy -= grd * e.b.w;
                }
                vals[0] = gcx;
                vals[1] = gcy;
                vals[2] = dur * dx; // B00
                vals[3] = dur * dy; // B01
                vals[4] = dvr * dx; // B10
                vals[5] = dvr * dy; // B11
                vals[6] = gq * dx;  // q0
                vals[7] = gq * dy;  // q1
                S = alpha * cg + (1.0f - alpha) * S;
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
        // one atomic add per touched (entry, number)
        for (uint32_t q = tid; q < m * NV; q += 256) {
            const uint32_t e = q / NV, k = q - e * NV;
            if (!s_touch[e]) continue;
            const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
            const size_t idx = s_idx[e];
            float *dst = k < SF_R ? p.grad_records + idx * 8 + k : p.grad_color + idx * 4 + (k - SF_R);
            if constexpr (DEPTH) dst = k == SF_Z ? p.grad_depth + idx : dst;
            atomicAdd(dst, sum);
        }
        cend = c0;
    }
}

template <bool PX, bool DIST = false>
__global__ __launch_bounds__(256) void k_surfel_depth(SurfDepthParams p) {
    __shared__ SurfEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];

    TILE_PIXEL_PROLOGUE(p);
    (void)tid, (void)lane, (void)w, (void)tile_idx;

    bool live = pixel_ok;
    float T = 1.0f, zw = 0.0f, ws = 0.0f;
    [[maybe_unused]] SurfDist ds; // (DIST)
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        surf_stage_chunk<true>(p, off, c0, m, s_ent, s_idx);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, rd, dx, dy;
                const bool in = surf_alpha<PX>(s_ent[j], pxf, pyf, alpha, ge, u, v, rd, dx, dy);
                const float wgt = surf_blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if (in) {
                    zw += (s_ent[j].d.x * rd) * wgt;
                    ws += wgt;
                    if constexpr (DIST) {
                        const float t = s_ent[j].d.x * rd;
                        if (surf_dist_participates(t)) surf_dist_step(ds, p.dist_c, t, wgt);
                    }
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
        const size_t o = (size_t)py * p.width + px;
        if constexpr (DIST) {
            if (p.out_depth) p.out_depth[o] = ws > 0.0f ? zw / ws : __builtin_inff();
            p.out_dist[o] = ds.dist;
        } else {
            p.out_depth[o] = ws > 0.0f ? zw / ws : __builtin_inff();
        }
        if (p.out_alpha) p.out_alpha[o] = 1.0f - T;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The projector's backward.

namespace {
struct SurfUniforms {
    float m[16], eye[3], time, w, h;
};
} // namespace

__global__ __launch_bounds__(256) void k_project_surfel_backward(SurfUniforms U, const float4 *__restrict__ pos, uint32_t ps,
                                                                 const float4 *__restrict__ scl, uint32_t ss, const float4 *__restrict__ rot,
                                                                 uint32_t rs, uint32_t n, const float4 *__restrict__ grec,
                                                                 const float *__restrict__ gcw, float4 *__restrict__ gpos,
                                                                 float4 *__restrict__ gscl, float4 *__restrict__ grot) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 pf = pos[(size_t)i * ps], sf = scl[(size_t)i * ss], qf = rot[(size_t)i * rs];
    const DiscRecord r = surfel_record(U.m, U.w, U.h, pf, sf, qf);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // culled: a kept record has det != 0, so B is not all zeros
    if (r.a.z == 0.0f && r.a.w == 0.0f && r.b.x == 0.0f && r.b.y == 0.0f) {
        gpos[i] = zero; gscl[i] = zero; grot[i] = zero;
        return;
    }
    const float4 g0 = grec[(size_t)i * 2], g1 = grec[(size_t)i * 2 + 1];
    const double g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const double gw = gcw ? (double)gcw[i] : 0.0;
    double m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = (double)U.m[k];
    // forward in float64
    const double qn = sqrt(((double)qf.x * qf.x + (double)qf.y * qf.y) + ((double)qf.z * qf.z + (double)qf.w * qf.w));
    const double qr = qf.x / qn, qx = qf.y / qn, qy = qf.z / qn, qz = qf.w / qn;
    const double R0[3] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy + qr * qz), 2.0 * (qx * qz - qr * qy)};
    const double R1[3] = {2.0 * (qx * qy - qr * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz + qr * qx)};
    const double a0 = 3.0 * sf.x, a1 = 3.0 * sf.y;
    const double e0[3] = {R0[0] * a0, R0[1] * a0, R0[2] * a0}, e1[3] = {R1[0] * a1, R1[1] * a1, R1[2] * a1};
    const double p[3] = {pf.x, pf.y, pf.z};
    // rows x, y, w of VP applied to a direction, and to the point
    const double ctx = m[0] * e0[0] + m[4] * e0[1] + m[8] * e0[2], cty = m[1] * e0[0] + m[5] * e0[1] + m[9] * e0[2];
    const double ctw = m[3] * e0[0] + m[7] * e0[1] + m[11] * e0[2];
    const double cbx = m[0] * e1[0] + m[4] * e1[1] + m[8] * e1[2], cby = m[1] * e1[0] + m[5] * e1[1] + m[9] * e1[2];
    const double cbw = m[3] * e1[0] + m[7] * e1[1] + m[11] * e1[2];
    const double cpx = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12], cpy = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    const double cpw = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15];
    const double hw = 0.5 * U.w, hh = 0.5 * U.h;
    const double m00 = hw * (ctx + ctw), m01 = hw * (cbx + cbw), m02 = hw * (cpx + cpw);
    const double m10 = hh * (ctw - cty), m11 = hh * (cbw - cby), m12 = hh * (cpw - cpy);
    const double icw = 1.0 / cpw;
    const double scx = m02 * icw, scy = m12 * icw;
    const double a00 = m00 - scx * ctw, a01 = m01 - scx * cbw, a10 = m10 - scy * ctw, a11 = m11 - scy * cbw;
    const double det = a00 * a11 - a01 * a10;
    const double idet = 1.0 / det, k = cpw * idet;
    // the record {scx, scy, a11 k, -a01 k, -a10 k, a00 k, (a11 ctw - a10 cbw) idet, (a00 cbw - a01 ctw) idet}, reversed
    double g_a11 = g[2] * k + g[6] * ctw * idet, g_a01 = -g[3] * k - g[7] * ctw * idet;
    double g_a10 = -g[4] * k - g[6] * cbw * idet, g_a00 = g[5] * k + g[7] * cbw * idet;
    const double g_k = ((g[2] * a11 - g[3] * a01) - g[4] * a10) + g[5] * a00;
    double g_ctw = (g[6] * a11 - g[7] * a01) * idet, g_cbw = (g[7] * a00 - g[6] * a10) * idet;
    const double g_idet = g[6] * (a11 * ctw - a10 * cbw) + g[7] * (a00 * cbw - a01 * ctw) + g_k * cpw;
    double g_cpw = g_k * idet + gw;
    const double g_det = -g_idet * idet * idet;
    g_a00 += g_det * a11; g_a11 += g_det * a00; g_a01 -= g_det * a10; g_a10 -= g_det * a01;
    double g_scx = g[0] - (g_a00 * ctw + g_a01 * cbw), g_scy = g[1] - (g_a10 * ctw + g_a11 * cbw);
    g_ctw -= g_a00 * scx + g_a10 * scy;
    g_cbw -= g_a01 * scx + g_a11 * scy;
    const double g_m02 = g_scx * icw, g_m12 = g_scy * icw;
    g_cpw -= (g_scx * m02 + g_scy * m12) * icw * icw;
    const double g_ctx = hw * g_a00, g_cbx = hw * g_a01, g_cpx = hw * g_m02;
    const double g_cty = -hh * g_a10, g_cby = -hh * g_a11, g_cpy = -hh * g_m12;
    g_ctw += hw * g_a00 + hh * g_a10;
    g_cbw += hw * g_a01 + hh * g_a11;
    g_cpw += hw * g_m02 + hh * g_m12;
    double ge0[3], ge1[3], gp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ge0[c] = m[4 * c] * g_ctx + m[4 * c + 1] * g_cty + m[4 * c + 3] * g_ctw;
        ge1[c] = m[4 * c] * g_cbx + m[4 * c + 1] * g_cby + m[4 * c + 3] * g_cbw;
        gp[c] = m[4 * c] * g_cpx + m[4 * c + 1] * g_cpy + m[4 * c + 3] * g_cpw;
    }
    const double gs0 = 3.0 * (R0[0] * ge0[0] + R0[1] * ge0[1] + R0[2] * ge0[2]);
    const double gs1 = 3.0 * (R1[0] * ge1[0] + R1[1] * ge1[1] + R1[2] * ge1[2]);
    const double G00 = a0 * ge0[0], G10 = a0 * ge0[1], G20 = a0 * ge0[2], G01 = a1 * ge1[0], G11 = a1 * ge1[1], G21 = a1 * ge1[2];
    // R's first two columns to the unit quaternion (r, x, y, z), then through q / |q|
    const double gqr = 2.0 * (((qz * G10 - qy * G20) - qz * G01) + qx * G21);
    const double gqx = 2.0 * ((qy * G10 + qz * G20) + qy * G01) - 4.0 * qx * G11 + 2.0 * qr * G21;
    const double gqy = -4.0 * qy * G00 + 2.0 * ((qx * G10 - qr * G20) + qx * G01) + 2.0 * qz * G21;
    const double gqz = -4.0 * qz * G00 + 2.0 * ((qr * G10 + qx * G20) - qr * G01) - 4.0 * qz * G11 + 2.0 * qy * G21;
    const double dot = ((qr * gqr + qx * gqx) + qy * gqy) + qz * gqz;
    gpos[i] = make_float4((float)gp[0], (float)gp[1], (float)gp[2], 0.0f);
    gscl[i] = make_float4((float)gs0, (float)gs1, 0.0f, 0.0f);
    grot[i] = make_float4((float)((gqr - qr * dot) / qn), (float)((gqx - qx * dot) / qn), (float)((gqy - qy * dot) / qn),
                          (float)((gqz - qz * dot) / qn));
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.

namespace {

int surf_frame_checks(splat_ctx *ctx, const FrameArgs &f) {
    ARG_CHECK(ctx, f.color_opacity && f.records && f.tile_indices && f.tile_counts && f.tile_offsets);
    ARG_CHECK(ctx, (((uintptr_t)f.color_opacity | (uintptr_t)f.records) & 15) == 0);
    ARG_CHECK(ctx, (((uintptr_t)f.tile_indices | (uintptr_t)f.tile_counts | (uintptr_t)f.tile_offsets) & 3) == 0);
    return SPLAT_OK;
}

// surfel.h's c of a call's (near, far): 0 < near < far, far = +inf allowed
int surf_dist_constant(splat_ctx *ctx, float near, float far, float &c) {
    if (!(near > 0.0f && near < far && near < __builtin_inff()))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "the depth distortion needs 0 < near < far (far = +inf: m = 1 - near / t)");
    c = far == __builtin_inff() ? near : (float)((double)near * (double)far / ((double)far - (double)near));
    return SPLAT_OK;
}

} // namespace

int surfel_composite_backward(splat_ctx *ctx, const SurfelBackwardCall &c) {
    FrameArgs f{};
    f.cfg = c.cfg, f.color_opacity = c.color_opacity, f.color_stride_vec4 = c.color_stride_vec4, f.records = c.records;
    f.tile_indices = c.tile_indices, f.tile_counts = c.tile_counts, f.tile_offsets = c.tile_offsets, f.width = c.width, f.height = c.height, f.n = c.n;
    SurfDepthParams p{};
    uint32_t nty = 0;
    const char *who = c.dist ? "splat_composite_backward_distortion" : c.depth ? "splat_composite_backward_depth" : "splat_composite_backward";
    const int rc_setup = f.setup(ctx, who, p, nty, true);
    if (rc_setup != SPLAT_OK) return rc_setup;
    const int rc_frame = surf_frame_checks(ctx, f);
    if (rc_frame != SPLAT_OK) return rc_frame;
    ARG_CHECK(ctx, c.grad_rgba32f && (c.n == 0 || (c.grad_records && c.grad_color_opacity)));
    ARG_CHECK(ctx, (((uintptr_t)c.grad_rgba32f | (uintptr_t)c.grad_records | (uintptr_t)c.grad_color_opacity) & 15) == 0);
    if (c.depth) {
        ARG_CHECK(ctx, c.depth_f32 && (c.grad_depth_f32 || c.dist) && (c.n == 0 || c.grad_depth) && c.depth_stride_floats >= 1);
        ARG_CHECK(ctx, (((uintptr_t)c.depth_f32 | (uintptr_t)c.grad_depth_f32 | (uintptr_t)c.grad_depth) & 3) == 0);
    }
    if (c.dist) {
        ARG_CHECK(ctx, c.depth && c.grad_distortion_f32 && ((uintptr_t)c.grad_distortion_f32 & 3) == 0);
        const int rc_dist = surf_dist_constant(ctx, c.near, c.far, p.dist_c);
        if (rc_dist != SPLAT_OK) return rc_dist;
        p.grad_dist_img = (const float *)c.grad_distortion_f32;
    }
    if (c.n == 0) return SPLAT_OK; // (no splat: every list is empty)
    p.grad_img = (const float4 *)c.grad_rgba32f;
    p.grad_records = (float *)c.grad_records;
    p.grad_color = (float *)c.grad_color_opacity;
    p.z = (const float *)c.depth_f32;
    p.z_stride = c.depth_stride_floats;
    p.grad_depth_img = (const float *)c.grad_depth_f32;
    p.grad_depth = (float *)c.grad_depth;
    variant_dispatch([&](auto d, auto px, auto dist) {
        if constexpr (d.value || !dist.value) // (DIST is a flag on DEPTH's kernel)
            launch_kernel(ctx, NO_STAGE, k_surfel_backward<d.value, px.value, dist.value>, dim3(p.ntx, nty), dim3(256), p);
    }, c.depth, composite_uses_px(ctx, p.ntx, nty), c.dist);
    return launch_check(ctx, c.dist ? "launch k_surfel_backward<DEPTH, DIST>" : c.depth ? "launch k_surfel_backward<DEPTH>" : "launch k_surfel_backward");
}

extern "C" int splat_composite_backward_distortion(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                                   uint32_t color_stride_vec4, const void *records, const void *tile_indices,
                                                   const void *tile_counts, const void *tile_offsets, uint32_t width, uint32_t height,
                                                   const void *grad_rgba32f, uint32_t n, void *grad_records, void *grad_color_opacity,
                                                   const void *depth_f32, uint32_t depth_stride_floats, const void *grad_depth_f32,
                                                   void *grad_depth, float near, float far, const void *grad_distortion_f32) {
    SurfelBackwardCall a{};
    FRAME_ARGS(a);
    a.grad_rgba32f = grad_rgba32f, a.grad_records = grad_records, a.grad_color_opacity = grad_color_opacity;
    a.depth_f32 = depth_f32, a.depth_stride_floats = depth_stride_floats, a.grad_depth_f32 = grad_depth_f32, a.grad_depth = grad_depth;
    a.near = near, a.far = far, a.grad_distortion_f32 = grad_distortion_f32;
    a.depth = a.dist = true;
    return surfel_composite_backward(ctx, a);
}

namespace {

// splat_composite_surfel_depth, and (out_distortion_f32 given: dist) splat_composite_surfel_distortion: one walk, one launch
int surfel_depth_forward(splat_ctx *ctx, const FrameArgs &f, const void *depth_f32, uint32_t depth_stride_floats, void *out_depth_f32,
                         void *out_alpha_f32, bool dist, float near, float far, void *out_distortion_f32) {
    SurfDepthParams p{};
    uint32_t nty = 0;
    const int rc_setup = f.setup(ctx, dist ? "splat_composite_surfel_distortion" : "splat_composite_surfel_depth", p, nty, true);
    if (rc_setup != SPLAT_OK) return rc_setup;
    const int rc_frame = surf_frame_checks(ctx, f);
    if (rc_frame != SPLAT_OK) return rc_frame;
    ARG_CHECK(ctx, depth_f32 && depth_stride_floats >= 1 && (out_depth_f32 || dist));
    ARG_CHECK(ctx, (((uintptr_t)depth_f32 | (uintptr_t)out_depth_f32 | (uintptr_t)out_alpha_f32) & 3) == 0);
    if (dist) {
        ARG_CHECK(ctx, out_distortion_f32 && ((uintptr_t)out_distortion_f32 & 3) == 0);
        const int rc_dist = surf_dist_constant(ctx, near, far, p.dist_c);
        if (rc_dist != SPLAT_OK) return rc_dist;
        p.out_dist = (float *)out_distortion_f32;
    }
    p.z = (const float *)depth_f32;
    p.z_stride = depth_stride_floats;
    p.out_depth = (float *)out_depth_f32;
    p.out_alpha = (float *)out_alpha_f32;
    variant_dispatch([&](auto px, auto d) { launch_kernel(ctx, NO_STAGE, k_surfel_depth<px.value, d.value>, dim3(p.ntx, nty), dim3(256), p); },
                     composite_uses_px(ctx, p.ntx, nty), dist);
    return launch_check(ctx, dist ? "launch k_surfel_depth<DIST>" : "launch k_surfel_depth");
}

} // namespace

extern "C" int splat_composite_surfel_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                            const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                            uint32_t width, uint32_t height, const void *depth_f32, uint32_t depth_stride_floats, uint32_t n,
                                            void *out_depth_f32, void *out_alpha_f32) {
    FrameArgs f{};
    FRAME_ARGS(f);
    return surfel_depth_forward(ctx, f, depth_f32, depth_stride_floats, out_depth_f32, out_alpha_f32, false, 0.0f, 0.0f, nullptr);
}

extern "C" int splat_composite_surfel_distortion(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                                 uint32_t color_stride_vec4, const void *records, const void *tile_indices,
                                                 const void *tile_counts, const void *tile_offsets, uint32_t width, uint32_t height,
                                                 const void *depth_f32, uint32_t depth_stride_floats, uint32_t n, void *out_depth_f32,
                                                 void *out_alpha_f32, float near, float far, void *out_distortion_f32) {
    FrameArgs f{};
    FRAME_ARGS(f);
    return surfel_depth_forward(ctx, f, depth_f32, depth_stride_floats, out_depth_f32, out_alpha_f32, true, near, far, out_distortion_f32);
}

extern "C" int splat_project_surfel_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                             const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                             uint32_t n, const void *grad_records, const void *grad_clip_w, void *grad_positions, void *grad_scales,
                                             void *grad_rotations) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (positions && scales && rotations && grad_records && grad_positions && grad_scales && grad_rotations)));
    ARG_CHECK(ctx, pos_stride_vec4 >= 1 && scale_stride_vec4 >= 1 && rot_stride_vec4 >= 1);
    ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)scales | (uintptr_t)rotations | (uintptr_t)grad_records | (uintptr_t)grad_positions |
                     (uintptr_t)grad_scales | (uintptr_t)grad_rotations) & 15) == 0 && ((uintptr_t)grad_clip_w & 3) == 0);
    if (n == 0) return SPLAT_OK;
    SurfUniforms u;
    for (int k = 0; k < 22; ++k) (&u.m[0])[k] = uniforms[k];
    launch_kernel(ctx, NO_STAGE, k_project_surfel_backward, dim3(div_up(n, 256)), dim3(256), u, (const float4 *)positions, pos_stride_vec4,
                  (const float4 *)scales, scale_stride_vec4, (const float4 *)rotations, rot_stride_vec4, n, (const float4 *)grad_records,
                  (const float *)grad_clip_w, (float4 *)grad_positions, (float4 *)grad_scales, (float4 *)grad_rotations);
    return launch_check(ctx, "launch k_project_surfel_backward");
}
