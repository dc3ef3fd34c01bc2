// splat_grad.hip — the per-splat kernels behind the gradients of a frame of anisotropic 3D Gaussians
// (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference counterpart): one thread per splat takes the gradient of its record
// and of its colour (what composite_grad.hip's per-tile kernels sum) on to the splat's parameters, in float64 where the chain
// is long.  The results are held to float64 references within bounds, not bit for bit against anything.
//
// k_project_ellipsoid_backward<DEPTH, CAM, AA>
//   The record's gradient through B = U / 3, U(a, b, c), Sigma2 = T T^T + 0.3 I, T = J M, M = R S, the quaternion's
//   normalisation and J's and the centre's dependence on the position, in float64.  The cull decisions are
//   ellipsoid_record's own (binary32); a culled splat gets exact zeros.
//     flag   entry points             adds                                                            argument struct
//     DEPTH  _depth; _camera and _aa  the ProjectedSplat depth's term, dL/dz (p - eye) / |p - eye|,   GradUniforms
//            given grad_depth         in dL/dposition
//     CAM    _camera; _aa given       the splat's own dL/d(VP, eye), 12 numbers (15 with DEPTH),      GradUniformsCam
//            grad_uniforms            summed over its wave into the partials (below)
//     AA     _aa                      the gradient of the 2D Mip filter's factor rho (ellipsoid.h:    GradUniformsAa
//                                     <RHO>), whose term joins dL/d(A, B, C) before gT is formed;
//                                     zero where the forward's binary32 rho is 0
// k_sh_colors_backward<DEG, CAM>
//   sh.hip's basis and constants of degree DEG, dir = normalize(p - eye), zero where the forward's max(., 0) clamped
//   (sh_forward_sums: the forward's sums with the forward's roundings, so that the decision is the forward's).
//   <CAM> (_camera): also dL/deye = -sum_i gpos[i], each splat's binary32 gpos summed in float64 (ShOpacityCam).
// k_camera_sum_slices<NV>, k_camera_sum<MODE>
//   The camera's gradient, dL/d(VP, eye), summed over all splats in a fixed order: the lanes of a wave by DPP
//   (wave_reduce.h), the per-wave partials in the context's scratch, then the partials slice by slice in index order.  The
//   same inputs give the same bits on every run.
#include "common.h"
#include "variant.h"
#include "disc.h"
#include "ellipsoid.h"
#include "wave_reduce.h"

struct GradUniforms {
    float m[16];
    float eye[3];
    float time;
    float w, h;
};

// The camera's share of a frame's gradient (splat_project_ellipsoid_backward_camera, splat_sh_colors_backward_camera): numbers
// summed over all splats, in float64 and in a fixed order, so that the result is the same bits on every run.
constexpr int CAM_NV = 15;      // 12 of VP (column k = 0..3, rows 0, 1, 3: number 3 k + {0, 1, 2}), then 3 of the eye
constexpr int CAM_SLOTS = 16;   // doubles per wave in the partials buffer (128 bytes: one line)
constexpr uint32_t CAM_SLICES = 64; // k_camera_sum: slices of the partials summed side by side (16 threads each)
constexpr uint32_t CAM_DIRECT = 1024; // partials k_camera_sum takes directly; more go through k_camera_sum_slices first

// One thread's NV numbers summed over its wave, a DPP sum per number, and stored by lane 63 as the wave's partial:
// part[4 blockIdx.x + wave][0 .. NV).  `any` is wave-uniform (a ballot): a wave whose lanes all hold zeros stores them without
// summing.  Per wave, not per workgroup: meeting the four waves in LDS first (a barrier at the end of the kernel, 512 bytes of
// LDS, a quarter of the partials) measured the same at C2, so the kernels carry neither.
template <int NV>
__device__ __forceinline__ void cam_wave_sum(const double (&v)[NV], bool any, double *__restrict__ part) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    double *dst = part + ((size_t)blockIdx.x * 4u + wave) * CAM_SLOTS;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const double t = any ? wave_sum63_f64(v[j]) : 0.0;
        if (lane == 63u) dst[j] = t;
    }
}

// part[b0 .. b1)'s number j, added in index order with 16 loads in flight (one load per add would wait out a memory latency each)
__device__ __forceinline__ double cam_sum_range(const double *__restrict__ part, uint32_t b0, uint32_t b1, uint32_t j) {
    double acc = 0.0;
    uint32_t b = b0;
    for (; b + 16 <= b1; b += 16) {
        double v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = part[(size_t)(b + q) * CAM_SLOTS + j];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += v[q];
    }
    for (; b < b1; ++b) acc += part[(size_t)b * CAM_SLOTS + j];
    return acc;
}

// The second stage for many partials (more than CAM_DIRECT): CAM_SLICES workgroups, workgroup s sums the partials
// [s per, (s + 1) per), per = ceil(nparts / CAM_SLICES), into part2[s]: thread 16 q + j adds number j of the slice's q-th
// sixteenth in index order, then the sixteen are added in order.  (One workgroup reading 20 000 partials took 0.09 ms: half
// of the projector's backward at C2.)
template <int NV>
__global__ __launch_bounds__(256) void k_camera_sum_slices(const double *__restrict__ part, uint32_t nparts, double *__restrict__ part2) {
    __shared__ double s_sum[16][CAM_SLOTS];
    const uint32_t q = threadIdx.x >> 4, j = threadIdx.x & 15u;
    const uint32_t per = (nparts + (CAM_SLICES - 1u)) / CAM_SLICES, per2 = (per + 15u) / 16u;
    const uint32_t s0 = min(blockIdx.x * per, nparts), s1 = min(s0 + per, nparts);
    const uint32_t b0 = min(s0 + q * per2, s1), b1 = min(b0 + per2, s1);
    s_sum[q][j] = j < (uint32_t)NV ? cam_sum_range(part, b0, b1, j) : 0.0;
    __syncthreads();
    if (threadIdx.x < CAM_SLOTS) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += s_sum[k][threadIdx.x];
        part2[(size_t)blockIdx.x * CAM_SLOTS + threadIdx.x] = t;
    }
}

// The last stage, one workgroup of 1024: thread 16 s + j adds number j of the partials [s per, (s + 1) per), per =
// ceil(nparts / 64), in index order; then the 64 slices' sums are added in slice order and rounded once to binary32.
// MODE 0: 15 numbers to the uniform block's 22 floats {VP column-major with row 2 zero, eye, 0, 0, 0}; 1: 12 numbers (no depth
// gradient: the eye's part zero, its slots in the partials not read); 2: 3 numbers to 4 floats {eye xyz, 0}.  nparts = 0
// writes the zeros.
template <int MODE>
__global__ __launch_bounds__(1024) void k_camera_sum(const double *__restrict__ part, uint32_t nparts, float *__restrict__ out) {
    constexpr uint32_t NV = MODE == 0 ? CAM_NV : MODE == 1 ? 12 : 3;
    __shared__ double s_sum[CAM_SLICES][CAM_SLOTS];
    __shared__ double s_tot[CAM_SLOTS];
    const uint32_t s = threadIdx.x >> 4, j = threadIdx.x & 15u;
    const uint32_t per = (nparts + (CAM_SLICES - 1u)) / CAM_SLICES;
    const uint32_t b0 = min(s * per, nparts), b1 = min(b0 + per, nparts);
    const double acc = j < NV ? cam_sum_range(part, b0, b1, j) : 0.0;
    s_sum[s][j] = acc;
    __syncthreads();
    if (threadIdx.x < CAM_SLOTS) {
        double t = 0.0;
        for (uint32_t q = 0; q < CAM_SLICES; ++q) t += s_sum[q][threadIdx.x];
        s_tot[threadIdx.x] = t;
    }
    __syncthreads();
    const uint32_t o = threadIdx.x;
    if (MODE == 2) {
        if (o < 4) out[o] = o < 3 ? (float)s_tot[o] : 0.0f;
    } else if (o < 22) {
        const uint32_t k = o >> 2, r = o & 3u;
        float v = 0.0f;
        if (o < 16) v = r == 2 ? 0.0f : (float)s_tot[3 * k + (r == 3 ? 2 : r)];
        else if (o < 19) v = (float)s_tot[12 + (o - 16)];
        out[o] = v;
    }
}

// the camera variant's further argument: per wave CAM_SLOTS doubles
struct GradUniformsCam : GradUniforms {
    double *part;
};

// the antialiased variant's further argument (splat_project_ellipsoid_backward_aa): dL/drho, n floats
struct GradUniformsAa : GradUniformsCam {
    const float *grho;
};

// (DEPTH: gdep[i] = dL/dz_i of the ProjectedSplat depth z = |p - eye|; not read otherwise)
// <CAM = true> (splat_project_ellipsoid_backward_camera): the same per-splat work, and each splat's own dL/d(VP, eye), still in
// float64, summed over each wave into U.part[4 blockIdx.x + wave] (12 numbers, 15 with DEPTH; a culled splat adds zeros).  One
// splat per thread there too: a loop over several splats per thread would shrink the partials, but the compiler then keeps
// the loop's invariants (VP in float64 among them) in registers across it: 208 / 216 VGPRs and two waves per SIMD, where one
// splat per thread holds the three of the kernel without the sums (the launch bound asks for them: 165 / 166 VGPRs).
// <AA = true> (splat_project_ellipsoid_backward_aa): the record's gradient and that of the 2D Mip filter's factor rho
// (ellipsoid.h: <RHO>), whose term joins dL/d(A, B, C) before gT is formed; the chain from there, the camera's numbers
// included, is the one below (rho reads VP through J only).  Zero where the forward's binary32 rho is 0.
template <bool DEPTH, bool CAM = false, bool AA = false>
__global__ __launch_bounds__(256, CAM ? 3 : 1) void k_project_ellipsoid_backward(
                                                                    std::conditional_t<AA, GradUniformsAa, std::conditional_t<CAM, GradUniformsCam, GradUniforms>> U,
                                                                    const float4 *__restrict__ pos, uint32_t ps,
                                                                    const float4 *__restrict__ scl, uint32_t ss, const float4 *__restrict__ rot,
                                                                    uint32_t rs, uint32_t n, const float4 *__restrict__ grec,
                                                                    float4 *__restrict__ gpos, float4 *__restrict__ gscl, float4 *__restrict__ grot,
                                                                    const float *__restrict__ gdep) {
    constexpr int NV = CAM ? (DEPTH ? CAM_NV : 12) : 1;
    double cam[NV];
    bool live = false;
    if constexpr (CAM) {
        for (int j = 0; j < NV; ++j) cam[j] = 0.0;
    }
    do { // (CAM leaves this block where the kernel without the sums returns)
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        if (i >= n) {
            if constexpr (CAM) break;
            else return;
        }
        const float4 pf = pos[(size_t)i * ps], sf = scl[(size_t)i * ss], qf = rot[(size_t)i * rs];
        float rho32 = 0.0f; // (AA) the forward's own rho
        DiscRecord r;
        if constexpr (AA) r = ellipsoid_record<true>(U.m, U.w, U.h, pf, sf, qf, &rho32);
        else r = ellipsoid_record(U.m, U.w, U.h, pf, sf, qf);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r.b.y == 0.0f) { // culled (B11 = 1 / (3 sqrt(c)) > 0 in every record that is not)
            gpos[i] = zero; gscl[i] = zero; grot[i] = zero;
            if constexpr (CAM) break;
            else return;
        }
        const float4 g0 = grec[(size_t)i * 2], g1 = grec[(size_t)i * 2 + 1];
        double m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = (double)U.m[k];
        const double W = U.w, H = U.h;
        // forward in float64
        const double qn = sqrt(((double)qf.x * qf.x + (double)qf.y * qf.y) + ((double)qf.z * qf.z + (double)qf.w * qf.w));
        const double qr = qf.x / qn, qx = qf.y / qn, qy = qf.z / qn, qz = qf.w / qn;
        const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qr * qz), 2.0 * (qx * qz + qr * qy)},
                                {2.0 * (qx * qy + qr * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qr * qx)},
                                {2.0 * (qx * qz - qr * qy), 2.0 * (qy * qz + qr * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
        const double s[3] = {sf.x, sf.y, sf.z};
        double M[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) M[a][b] = R[a][b] * s[b];
        const double p[3] = {pf.x, pf.y, pf.z};
        const double cx = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
        const double cy = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
        const double cw = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15];
        const double nx = cx / cw, ny = cy / cw;
        const double ax = 0.5 * W / cw, ay = 0.5 * H / cw;
        double J[2][3];
        for (int k = 0; k < 3; ++k) {
            J[0][k] = ax * (m[4 * k] - nx * m[4 * k + 3]);
            J[1][k] = ay * (ny * m[4 * k + 3] - m[4 * k + 1]);
        }
        double T[2][3];
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 3; ++b) T[a][b] = J[a][0] * M[0][b] + J[a][1] * M[1][b] + J[a][2] * M[2][b];
        const double A = T[0][0] * T[0][0] + T[0][1] * T[0][1] + T[0][2] * T[0][2] + 0.3;
        const double Bc = T[0][0] * T[1][0] + T[0][1] * T[1][1] + T[0][2] * T[1][2];
        const double C = T[1][0] * T[1][0] + T[1][1] * T[1][1] + T[1][2] * T[1][2] + 0.3;
        const double det = A * C - Bc * Bc;
        const double b00 = sqrt(C / det) / 3.0, b01 = -Bc / sqrt(C * det) / 3.0, b11 = 1.0 / sqrt(C) / 3.0;
        // backward: B -> (a, b, c)
        const double gB00 = g0.z, gB01 = g0.w, gB11 = g1.y, gsx = g0.x, gsy = g0.y;
        const double gdet = -(gB00 * b00 + gB01 * b01) / (2.0 * det);
        double gC = (gB00 * b00 - gB01 * b01 - gB11 * b11) / (2.0 * C) + gdet * A;
        double gA = gdet * C;
        double gB = gB01 * (-1.0 / (3.0 * sqrt(C * det))) - 2.0 * Bc * gdet;
        if constexpr (AA) {
            // rho^2 = det0 / det, det0 = A0 C0 - B^2, A0 = |T0|^2, C0 = |T1|^2 (A = A0 + 0.3, C = C0 + 0.3):  d(rho^2) = d(det0) / det - rho^2 d(det) / det.
            // (grho = 0 leaves gA, gB, gC as they are, bit for bit; so does a splat whose binary32 rho is 0: not differentiable
            // there.  det0 <= 0 in float64 beside a binary32 rho > 0 is the needle splats' cancellation: no term either.)
            // (A0, C0: the undilated sums A and C were formed from, not A - 0.3: a strongly minified splat's |T0|^2 would lose
            // its low bits under the 0.3)
            const double gr = U.grho[i];
            const double A0 = T[0][0] * T[0][0] + T[0][1] * T[0][1] + T[0][2] * T[0][2];
            const double C0 = T[1][0] * T[1][0] + T[1][1] * T[1][1] + T[1][2] * T[1][2];
            const double rho2 = (A0 * C0 - Bc * Bc) / det;
            const bool on = gr != 0.0 && rho32 > 0.0f && rho2 > 0.0;
            const double h = gr / (2.0 * sqrt(rho2));
            gA = on ? gA + h * (C0 / det - rho2 * C / det) : gA;
            gC = on ? gC + h * (A0 / det - rho2 * A / det) : gC;
            gB = on ? gB + h * ((-2.0 * Bc / det) * (1.0 - rho2)) : gB;
        }
        double gT[2][3];
        for (int k = 0; k < 3; ++k) {
            gT[0][k] = 2.0 * gA * T[0][k] + gB * T[1][k];
            gT[1][k] = 2.0 * gC * T[1][k] + gB * T[0][k];
        }
        // T = J M
        double gJ[2][3], gM[3][3];
        for (int a = 0; a < 2; ++a)
            for (int k = 0; k < 3; ++k) gJ[a][k] = gT[a][0] * M[k][0] + gT[a][1] * M[k][1] + gT[a][2] * M[k][2];
        for (int k = 0; k < 3; ++k)
            for (int b = 0; b < 3; ++b) gM[k][b] = J[0][k] * gT[0][b] + J[1][k] * gT[1][b];
        // M = R S
        double gs[3] = {0.0, 0.0, 0.0}, gR[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                gs[b] += gM[a][b] * R[a][b];
                gR[a][b] = gM[a][b] * s[b];
            }
        // R(unit quaternion)
        const double gqr = 2.0 * (-qz * gR[0][1] + qy * gR[0][2] + qz * gR[1][0] - qx * gR[1][2] - qy * gR[2][0] + qx * gR[2][1]);
        const double gqx = 2.0 * (qy * gR[0][1] + qz * gR[0][2] + qy * gR[1][0] - 2.0 * qx * gR[1][1] - qr * gR[1][2] + qz * gR[2][0] +
                                  qr * gR[2][1] - 2.0 * qx * gR[2][2]);
        const double gqy = 2.0 * (-2.0 * qy * gR[0][0] + qx * gR[0][1] + qr * gR[0][2] + qx * gR[1][0] + qz * gR[1][2] - qr * gR[2][0] +
                                  qz * gR[2][1] - 2.0 * qy * gR[2][2]);
        const double gqz = 2.0 * (-2.0 * qz * gR[0][0] - qr * gR[0][1] + qx * gR[0][2] + qr * gR[1][0] - 2.0 * qz * gR[1][1] +
                                  qy * gR[1][2] + qx * gR[2][0] + qy * gR[2][1]);
        // q / |q|
        const double dotq = qr * gqr + qx * gqx + qy * gqy + qz * gqz;
        grot[i] = make_float4((float)((gqr - qr * dotq) / qn), (float)((gqx - qx * dotq) / qn), (float)((gqy - qy * dotq) / qn),
                              (float)((gqz - qz * dotq) / qn));
        gscl[i] = make_float4((float)gs[0], (float)gs[1], (float)gs[2], 0.0f);
        // J(nx, ny, cw) and the screen centre
        double gax = 0.0, gay = 0.0, gnx = 0.5 * W * gsx, gny = -0.5 * H * gsy;
        for (int k = 0; k < 3; ++k) {
            gax += gJ[0][k] * (m[4 * k] - nx * m[4 * k + 3]);
            gnx -= gJ[0][k] * ax * m[4 * k + 3];
            gay += gJ[1][k] * (ny * m[4 * k + 3] - m[4 * k + 1]);
            gny += gJ[1][k] * ay * m[4 * k + 3];
        }
        const double gcx = gnx / cw, gcy = gny / cw;
        const double gcw = -(gax * ax + gay * ay) / cw - (gnx * nx + gny * ny) / cw;
        double gp[3];
        for (int k = 0; k < 3; ++k) gp[k] = gcx * m[4 * k] + gcy * m[4 * k + 1] + gcw * m[4 * k + 3];
        if constexpr (CAM) {
            // c = VP [p; 1]: column k of rows 0, 1, 3 through (c.x, c.y, c.w), times p[k] (the translation column: times 1);
            // J[0][k] = ax (m[4k] - nx m[4k+3]) and J[1][k] = ay (ny m[4k+3] - m[4k+1]) read the three rotation columns directly
            for (int k = 0; k < 3; ++k) {
                cam[3 * k] = gcx * p[k] + gJ[0][k] * ax;
                cam[3 * k + 1] = gcy * p[k] - gJ[1][k] * ay;
                cam[3 * k + 2] = gcw * p[k] + (gJ[1][k] * ay * ny - gJ[0][k] * ax * nx);
            }
            cam[9] = gcx;
            cam[10] = gcy;
            cam[11] = gcw;
            live = true;
        }
        if constexpr (DEPTH) {
            // z = |p - eye|: dz/dp = (p - eye) / z.  (gz = 0 leaves gp as it is, bit for bit: no -0 + 0)
            const double gz = gdep[i];
            const double d[3] = {p[0] - (double)U.eye[0], p[1] - (double)U.eye[1], p[2] - (double)U.eye[2]};
            const double z = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; ++k) gp[k] = gz != 0.0 ? gp[k] + gz * (d[k] / z) : gp[k];
            if constexpr (CAM) // dz/deye = -(p - eye) / z
                for (int k = 0; k < 3; ++k) cam[12 + k] = -gz * (d[k] / z);
        }
        gpos[i] = make_float4((float)gp[0], (float)gp[1], (float)gp[2], 0.0f);
    } while (false);
    if constexpr (CAM) cam_wave_sum<NV>(cam, __ballot(live) != 0, U.part);
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr float GSH_C0 = 0.28209479177387814f;
constexpr float GSH_C1 = 0.4886025119029199f;
constexpr float GSH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float GSH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                             -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

// k_sh_colors' sums 0.5 + sum_k Y_k sh_k, bit for bit: sh.hip's operations with one rounding each, as sh.hip is built
// (-ffp-contract=off).  The backward's clamp must be the forward's decision, and this file is built with contraction on: its own
// sum, contracted to FMAs, lands on the other side of 0 for a channel within a few roundings of the edge.
template <int DEG>
__device__ __forceinline__ void sh_forward_sums(float vx, float vy, float vz, const float *__restrict__ row, float &r, float &g, float &b) {
#pragma clang fp contract(off)
    const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
    const bool has_dir = len > 0.0f && len < INFINITY;
    const float il = has_dir ? 1.0f / len : 0.0f;
    const float x = has_dir ? vx * il : 0.0f, y = has_dir ? vy * il : 0.0f, z = has_dir ? vz * il : 0.0f;
    constexpr int NB = (DEG + 1) * (DEG + 1);
    float Y[NB];
    Y[0] = GSH_C0;
    if (DEG > 0) {
        Y[1] = -GSH_C1 * y;
        Y[2] = GSH_C1 * z;
        Y[3] = -GSH_C1 * x;
    }
    if (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = GSH_C2[0] * (x * y);
        Y[5] = GSH_C2[1] * (y * z);
        Y[6] = GSH_C2[2] * ((2.0f * zz - xx) - yy);
        Y[7] = GSH_C2[3] * (x * z);
        Y[8] = GSH_C2[4] * (xx - yy);
        if (DEG > 2) {
            Y[9] = GSH_C3[0] * (y * (3.0f * xx - yy));
            Y[10] = GSH_C3[1] * ((x * y) * z);
            Y[11] = GSH_C3[2] * (y * ((4.0f * zz - xx) - yy));
            Y[12] = GSH_C3[3] * (z * ((2.0f * zz - 3.0f * xx) - 3.0f * yy));
            Y[13] = GSH_C3[4] * (x * ((4.0f * zz - xx) - yy));
            Y[14] = GSH_C3[5] * (z * (xx - yy));
            Y[15] = GSH_C3[6] * (x * (xx - 3.0f * yy));
        }
    }
    r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        r += Y[k] * row[3 * k];
        g += Y[k] * row[3 * k + 1];
        b += Y[k] * row[3 * k + 2];
    }
    r += 0.5f, g += 0.5f, b += 0.5f;
}

// the camera variant's last argument: grad_opacity, and per wave CAM_SLOTS doubles
struct ShOpacityCam {
    float *gop;
    double *part;
};

// <CAM = true> (splat_sh_colors_backward_camera): also dL/deye = -sum_i gpos[i] (each splat's binary32 gpos, summed in
// float64), per wave into part[4 blockIdx.x + wave][0 .. 3)
template <int DEG, bool CAM = false>
__global__ __launch_bounds__(256) void k_sh_colors_backward(float ex, float ey, float ez, const float4 *__restrict__ pos, uint32_t pos_stride,
                                                            const float *__restrict__ sh, uint32_t sh_stride, const float4 *__restrict__ gcol,
                                                            uint32_t n, float *__restrict__ gsh, float4 *__restrict__ gpos,
                                                            std::conditional_t<CAM, ShOpacityCam, float *__restrict__> gop) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
    double cam[3] = {0.0, 0.0, 0.0};
    do { // (CAM leaves this block where the kernel without the sum returns)
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        if (i >= n) {
            if constexpr (CAM) break;
            else return;
        }
        const float *row = sh + (size_t)i * sh_stride;
        const float4 p = pos[(size_t)i * pos_stride];
        const float4 gc = gcol[i];
        float vx = p.x - ex, vy = p.y - ey, vz = p.z - ez;
        // the clamp: no gradient where the forward's max(., 0) took the 0 (decided on the forward's own bits, not on this
        // kernel's contracted Y: everything below keeps the bits it had)
        float r, g, b;
        sh_forward_sums<DEG>(vx, vy, vz, row, r, g, b);
        const float gr = (r > 0.0f) ? gc.x : 0.0f, gg = (g > 0.0f) ? gc.y : 0.0f, gb = (b > 0.0f) ? gc.z : 0.0f;
        const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
        // the forward's rule: no direction where |p - eye| is not a positive finite number (a splat at the eye).  Then Y_0 alone
        // is non-zero, and il = 0 makes grad_positions and the term of dL/deye zeros
        const bool has_dir = len > 0.0f && len < INFINITY;
        const float il = has_dir ? 1.0f / len : 0.0f;
        const float x = has_dir ? vx * il : 0.0f, y = has_dir ? vy * il : 0.0f, z = has_dir ? vz * il : 0.0f;
        float Y[NB], Yx[NB], Yy[NB], Yz[NB];
        Y[0] = GSH_C0; Yx[0] = 0.0f; Yy[0] = 0.0f; Yz[0] = 0.0f;
        if (DEG > 0) {
            Y[1] = -GSH_C1 * y; Yx[1] = 0.0f; Yy[1] = -GSH_C1; Yz[1] = 0.0f;
            Y[2] = GSH_C1 * z;  Yx[2] = 0.0f; Yy[2] = 0.0f;    Yz[2] = GSH_C1;
            Y[3] = -GSH_C1 * x; Yx[3] = -GSH_C1; Yy[3] = 0.0f; Yz[3] = 0.0f;
        }
        if (DEG > 1) {
            const float xx = x * x, yy = y * y, zz = z * z;
            Y[4] = GSH_C2[0] * (x * y);            Yx[4] = GSH_C2[0] * y;         Yy[4] = GSH_C2[0] * x;          Yz[4] = 0.0f;
            Y[5] = GSH_C2[1] * (y * z);            Yx[5] = 0.0f;                  Yy[5] = GSH_C2[1] * z;          Yz[5] = GSH_C2[1] * y;
            Y[6] = GSH_C2[2] * ((2.0f * zz - xx) - yy); Yx[6] = -2.0f * GSH_C2[2] * x; Yy[6] = -2.0f * GSH_C2[2] * y; Yz[6] = 4.0f * GSH_C2[2] * z;
            Y[7] = GSH_C2[3] * (x * z);            Yx[7] = GSH_C2[3] * z;         Yy[7] = 0.0f;                   Yz[7] = GSH_C2[3] * x;
            Y[8] = GSH_C2[4] * (xx - yy);          Yx[8] = 2.0f * GSH_C2[4] * x;  Yy[8] = -2.0f * GSH_C2[4] * y;  Yz[8] = 0.0f;
            if (DEG > 2) {
                Y[9] = GSH_C3[0] * (y * (3.0f * xx - yy));
                Yx[9] = GSH_C3[0] * 6.0f * x * y; Yy[9] = GSH_C3[0] * 3.0f * (xx - yy); Yz[9] = 0.0f;
                Y[10] = GSH_C3[1] * ((x * y) * z);
                Yx[10] = GSH_C3[1] * y * z; Yy[10] = GSH_C3[1] * x * z; Yz[10] = GSH_C3[1] * x * y;
                Y[11] = GSH_C3[2] * (y * ((4.0f * zz - xx) - yy));
                Yx[11] = -2.0f * GSH_C3[2] * x * y; Yy[11] = GSH_C3[2] * ((4.0f * zz - xx) - 3.0f * yy); Yz[11] = 8.0f * GSH_C3[2] * y * z;
                Y[12] = GSH_C3[3] * (z * ((2.0f * zz - 3.0f * xx) - 3.0f * yy));
                Yx[12] = -6.0f * GSH_C3[3] * x * z; Yy[12] = -6.0f * GSH_C3[3] * y * z; Yz[12] = GSH_C3[3] * ((6.0f * zz - 3.0f * xx) - 3.0f * yy);
                Y[13] = GSH_C3[4] * (x * ((4.0f * zz - xx) - yy));
                Yx[13] = GSH_C3[4] * ((4.0f * zz - 3.0f * xx) - yy); Yy[13] = -2.0f * GSH_C3[4] * x * y; Yz[13] = 8.0f * GSH_C3[4] * x * z;
                Y[14] = GSH_C3[5] * (z * (xx - yy));
                Yx[14] = 2.0f * GSH_C3[5] * x * z; Yy[14] = -2.0f * GSH_C3[5] * y * z; Yz[14] = GSH_C3[5] * (xx - yy);
                Y[15] = GSH_C3[6] * (x * (xx - 3.0f * yy));
                Yx[15] = GSH_C3[6] * 3.0f * (xx - yy); Yy[15] = -6.0f * GSH_C3[6] * x * y; Yz[15] = 0.0f;
            }
        }
        float *orow = gsh + (size_t)i * sh_stride;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            orow[3 * k] = Y[k] * gr;
            orow[3 * k + 1] = Y[k] * gg;
            orow[3 * k + 2] = Y[k] * gb;
            const float gY = (gr * row[3 * k] + gg * row[3 * k + 1]) + gb * row[3 * k + 2];
            gx += gY * Yx[k];
            gy += gY * Yy[k];
            gz += gY * Yz[k];
        }
        // dir = v / |v|:  dL/dv = (g - dir (dir . g)) / |v|
        const float dg = (x * gx + y * gy) + z * gz;
        gpos[i] = make_float4((gx - x * dg) * il, (gy - y * dg) * il, (gz - z * dg) * il, 0.0f);
        if constexpr (CAM) gop.gop[i] = gc.w;
        else gop[i] = gc.w;
        if constexpr (CAM) {
            cam[0] = -(double)((gx - x * dg) * il); cam[1] = -(double)((gy - y * dg) * il); cam[2] = -(double)((gz - z * dg) * il);
        }
    } while (false);
    if constexpr (CAM) cam_wave_sum<3>(cam, true, gop.part);
}

// ---------------------------------------------------------------------------------------------------------------------
// The camera variants' grid and partials: ceil(n / 256) workgroups, one 128-byte line of the context's scratch per wave, and
// CAM_SLICES more lines for k_camera_sum_slices
static int camera_partials(splat_ctx *ctx, uint32_t n, uint32_t &nparts, double *&part) {
    nparts = div_up(n, 256) * 4u; // (n <= 2^32 - 1: at most 2^26 lines)
    const int rc = ctx_ensure_scan_ws(ctx, ((size_t)nparts + CAM_SLICES) * CAM_SLOTS * sizeof(double));
    part = (double *)ctx->scan_ws;
    return rc;
}

// The sums' later stages: MODE as k_camera_sum's.  Which kernels run, and so the order of the sum, depends on n only.
template <int MODE>
static void camera_sum_launch(splat_ctx *ctx, const double *part, uint32_t nparts, float *out) {
    constexpr int NV = MODE == 0 ? CAM_NV : MODE == 1 ? 12 : 3;
    if (nparts > CAM_DIRECT) {
        double *part2 = const_cast<double *>(part) + (size_t)nparts * CAM_SLOTS;
        hipLaunchKernelGGL(k_camera_sum_slices<NV>, dim3(CAM_SLICES), dim3(256), 0, ctx->stream, part, nparts, part2);
        part = part2;
        nparts = CAM_SLICES;
    }
    hipLaunchKernelGGL(k_camera_sum<MODE>, dim3(1), dim3(16 * CAM_SLICES), 0, ctx->stream, part, nparts, out);
}

namespace {

// What the four ellipsoid projector backwards hand to their one launch, under the names of include/splat.h's arguments (the
// argument checks quote them); a field an entry point does not have stays NULL.  need_depth: grad_depth is required (else
// optional: NULL = none); cam: also dL/duniforms into grad_uniforms, summed from per-wave partials; aa: the antialiased
// variant, with grad_rho; what: the launch's name in an error.
struct ProjectBackwardArgs {
    const float *uniforms;
    const void *positions, *scales, *rotations;
    uint32_t pos_stride_vec4, scale_stride_vec4, rot_stride_vec4, n;
    const void *grad_records;
    void *grad_positions, *grad_scales, *grad_rotations;
    const void *grad_depth;
    void *grad_uniforms;
    const void *grad_rho;
    bool need_depth, cam, aa;
    const char *what;

    int launch(splat_ctx *ctx) const {
        if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
        ARG_CHECK(ctx, uniforms && (!cam || grad_uniforms) &&
                           (n == 0 || (positions && scales && rotations && grad_records && grad_positions && grad_scales && grad_rotations &&
                                       (!need_depth || grad_depth) && (!aa || grad_rho))));
        ARG_CHECK(ctx, pos_stride_vec4 >= 1 && scale_stride_vec4 >= 1 && rot_stride_vec4 >= 1);
        ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)scales | (uintptr_t)rotations | (uintptr_t)grad_records | (uintptr_t)grad_positions |
                         (uintptr_t)grad_scales | (uintptr_t)grad_rotations | (uintptr_t)grad_uniforms) & 15) == 0 &&
                           (((uintptr_t)grad_depth | (uintptr_t)grad_rho) & 3) == 0);
        GradUniformsAa u;
        u.grho = (const float *)grad_rho;
        uint32_t nparts = 0;
        u.part = nullptr;
        if (cam) {
            const int rc = camera_partials(ctx, n, nparts, u.part);
            if (rc != SPLAT_OK) return rc;
        }
        if (n) {
            for (int k = 0; k < 22; ++k) (&u.m[0])[k] = uniforms[k];
            // (<DEPTH, CAM, AA>: the kernel without AA takes the GradUniformsCam part of u, the one without CAM its GradUniforms part)
            variant_dispatch(
                [&](auto depth, auto cam_, auto aa_) {
                    launch_kernel(ctx, NO_STAGE, k_project_ellipsoid_backward<depth.value, cam_.value, aa_.value>, dim3(div_up(n, 256)), dim3(256),
                                  u, (const float4 *)positions, pos_stride_vec4, (const float4 *)scales, scale_stride_vec4,
                                  (const float4 *)rotations, rot_stride_vec4, n, (const float4 *)grad_records, (float4 *)grad_positions,
                                  (float4 *)grad_scales, (float4 *)grad_rotations, (const float *)grad_depth);
                },
                grad_depth != nullptr, cam, aa);
            const int rc = launch_check(ctx, what);
            if (rc != SPLAT_OK) return rc;
        }
        if (!cam) return SPLAT_OK;
        // (without grad_depth the kernel leaves numbers 12-14 of its partials unwritten: the sum reads 12 then)
        if (grad_depth || n == 0) camera_sum_launch<0>(ctx, u.part, nparts, (float *)grad_uniforms);
        else camera_sum_launch<1>(ctx, u.part, nparts, (float *)grad_uniforms);
        LAUNCH_CHECK(ctx, "k_camera_sum");
        return SPLAT_OK;
    }
};

} // namespace

// The arguments every projector backward has, by name (the entry points' parameter names are the struct's field names)
#define PROJECT_BACKWARD_COMMON(a)                                                                                             \
    a.uniforms = uniforms, a.positions = positions, a.pos_stride_vec4 = pos_stride_vec4, a.scales = scales,                    \
    a.scale_stride_vec4 = scale_stride_vec4, a.rotations = rotations, a.rot_stride_vec4 = rot_stride_vec4, a.n = n,            \
    a.grad_records = grad_records, a.grad_positions = grad_positions, a.grad_scales = grad_scales, a.grad_rotations = grad_rotations

extern "C" int splat_project_ellipsoid_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                                uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales, void *grad_rotations) {
    ProjectBackwardArgs a{};
    PROJECT_BACKWARD_COMMON(a);
    a.what = "launch k_project_ellipsoid_backward";
    return a.launch(ctx);
}

extern "C" int splat_project_ellipsoid_backward_depth(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                      const void *scales, uint32_t scale_stride_vec4, const void *rotations,
                                                      uint32_t rot_stride_vec4, uint32_t n, const void *grad_records, void *grad_positions,
                                                      void *grad_scales, void *grad_rotations, const void *grad_depth) {
    ProjectBackwardArgs a{};
    PROJECT_BACKWARD_COMMON(a);
    a.grad_depth = grad_depth, a.need_depth = true;
    a.what = "launch k_project_ellipsoid_backward<DEPTH>";
    return a.launch(ctx);
}

extern "C" int splat_project_ellipsoid_backward_camera(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                       const void *scales, uint32_t scale_stride_vec4, const void *rotations,
                                                       uint32_t rot_stride_vec4, uint32_t n, const void *grad_records, void *grad_positions,
                                                       void *grad_scales, void *grad_rotations, const void *grad_depth, void *grad_uniforms) {
    ProjectBackwardArgs a{};
    PROJECT_BACKWARD_COMMON(a);
    a.grad_depth = grad_depth, a.grad_uniforms = grad_uniforms, a.cam = true;
    a.what = "launch k_project_ellipsoid_backward<CAM>";
    return a.launch(ctx);
}

extern "C" int splat_project_ellipsoid_backward_aa(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                   const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                                   uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales,
                                                   void *grad_rotations, const void *grad_depth, void *grad_uniforms, const void *grad_rho) {
    ProjectBackwardArgs a{};
    PROJECT_BACKWARD_COMMON(a);
    a.grad_depth = grad_depth, a.grad_uniforms = grad_uniforms, a.cam = grad_uniforms != nullptr;
    a.grad_rho = grad_rho, a.aa = true;
    a.what = "launch k_project_ellipsoid_backward<AA>";
    return a.launch(ctx);
}

namespace {

// What the two SH backwards hand to their one launch, named as above.  cam: also dL/deye into grad_eye, summed from per-wave
// partials.
struct ShBackwardArgs {
    const float *eye3;
    const void *positions, *sh, *opacity_f32, *grad_color_opacity;
    uint32_t pos_stride_vec4, sh_stride_floats, degree, n;
    void *grad_sh, *grad_positions, *grad_opacity, *grad_eye;
    bool cam;

    int launch(splat_ctx *ctx) const {
        if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
        ARG_CHECK(ctx, eye3 && (!cam || grad_eye) && degree <= 3 && pos_stride_vec4 >= 1);
        ARG_CHECK(ctx, n == 0 || (positions && sh && grad_color_opacity && grad_sh && grad_positions && grad_opacity));
        ARG_CHECK(ctx, sh_stride_floats >= 3 * (degree + 1) * (degree + 1));
        ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)grad_color_opacity | (uintptr_t)grad_positions | (uintptr_t)grad_eye) & 15) == 0 &&
                           (((uintptr_t)sh | (uintptr_t)grad_sh | (uintptr_t)grad_opacity | (uintptr_t)opacity_f32) & 3) == 0);
        ShOpacityCam gop = {(float *)grad_opacity, nullptr};
        uint32_t nparts = 0;
        if (cam) {
            const int rc = camera_partials(ctx, n, nparts, gop.part);
            if (rc != SPLAT_OK) return rc;
        }
        if (n) {
            variant_dispatch(
                [&](auto deg, auto cam_) {
                    const auto last = [&] { if constexpr (cam_.value) return gop; else return gop.gop; }(); // (<CAM>: with the partials)
                    launch_kernel(ctx, NO_STAGE, k_sh_colors_backward<deg.value, cam_.value>, dim3(div_up(n, 256)), dim3(256), eye3[0], eye3[1],
                                  eye3[2], (const float4 *)positions, pos_stride_vec4, (const float *)sh, sh_stride_floats,
                                  (const float4 *)grad_color_opacity, n, (float *)grad_sh, (float4 *)grad_positions, last);
                },
                OneOf<0, 1, 2, 3>{(int)degree}, cam);
            const int rc = launch_check(ctx, cam ? "launch k_sh_colors_backward<CAM>" : "launch k_sh_colors_backward");
            if (rc != SPLAT_OK) return rc;
        }
        if (!cam) return SPLAT_OK;
        camera_sum_launch<2>(ctx, gop.part, nparts, (float *)grad_eye);
        LAUNCH_CHECK(ctx, "k_camera_sum");
        return SPLAT_OK;
    }
};

} // namespace

#define SH_BACKWARD_COMMON(a)                                                                                                  \
    a.eye3 = eye3, a.positions = positions, a.pos_stride_vec4 = pos_stride_vec4, a.sh = sh, a.sh_stride_floats = sh_stride_floats, \
    a.degree = degree, a.opacity_f32 = opacity_f32, a.grad_color_opacity = grad_color_opacity, a.n = n, a.grad_sh = grad_sh,   \
    a.grad_positions = grad_positions, a.grad_opacity = grad_opacity

extern "C" int splat_sh_colors_backward(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                                        uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, const void *grad_color_opacity,
                                        uint32_t n, void *grad_sh, void *grad_positions, void *grad_opacity) {
    ShBackwardArgs a{};
    SH_BACKWARD_COMMON(a);
    return a.launch(ctx);
}

extern "C" int splat_sh_colors_backward_camera(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                                               uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32,
                                               const void *grad_color_opacity, uint32_t n, void *grad_sh, void *grad_positions,
                                               void *grad_opacity, void *grad_eye) {
    ShBackwardArgs a{};
    SH_BACKWARD_COMMON(a);
    a.grad_eye = grad_eye, a.cam = true;
    return a.launch(ctx);
}

