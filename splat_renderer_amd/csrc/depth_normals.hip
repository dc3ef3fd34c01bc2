// depth_normals.hip — the normal of the surface a depth map describes, and 2DGS's normal-consistency loss between it and a
// blended normal map (an extension, no reference counterpart; include/splat.h, "Normals of a depth map", states the contract).
//
// The camera's rays are affine in the pixel index, d(x, y) = D0 + x Dx + y Dy (splat_camera_rays makes D0, Dx, Dy and the
// handedness sign in float64 on the host), and the point a pixel sees is eye + s d with s the ray parameter: s = depth for planar
// depth, depth / |d| for the distance from the eye.  With D = s_r - s_l, S = s_r + s_l across a pixel and likewise down it, the
// contract's n = sigma (a_y x a_x), a_x = Dx_s d + Sx_s Dx, a_y = Dy_s d + Sy_s Dy, is evaluated as
//     n = sigma [Dy_s Sx_s P + Sy_s Dx_s Q + Sy_s Sx_s C],   P = d x Dx = A + y C,  Q = Dy x d = B + x C,  C = Dy x Dx,
// A = D0 x Dx, B = Dy x D0: the d x d term, which is zero, is not formed and cancelled, and what is left is linear in each of the
// four ray parameters, so the backward is three dot products: dn/ds_r = sigma [Dy_s P + Sy_s (Q + C)] and so on.  P and Q are
// made per pixel in float64 from the host's float64 A, B, C and rounded once.
//
// One __device__ function, pixel_normal, evaluates a pixel; k_depth_normals (the map, or the loss's sums) and
// k_depth_normals_backward (the map's backward, or the loss's two gradients in one launch) call it on tiles of 32 x 16 pixels,
// 256 threads, as loss.hip tiles the screen.  The ray parameters of the tile and its halo are staged in LDS by coalesced row
// loads: halo 1 forward; halo 2 backward, where a depth pixel q gathers from the normals of its four neighbours, which read
// q +- 2 and the diagonals.  The backward evaluates each pixel of the tile and its halo 1 once, leaves the four derivatives
// dL/ds_l, dL/ds_r, dL/ds_u, dL/ds_d of each in LDS, and q adds the four that name it in a fixed order: no atomics, no
// workspace, the same bits on every run.  1 / |d| is formed in float64 per staged pixel (one square root and one divide, beside
// 4 bytes of HBM traffic), so that s is the correctly rounded quotient and s_r - s_l loses nothing to a rounded 1 / |d|.
//
// Roofline: all four are bound by HBM ("Normal consistency", has the measured times beside the floors).
#include "common.h"
#include "image.h"

#include <math.h>

namespace {

constexpr int NTW = 32, NTH = 16;    // a workgroup's tile
constexpr int NPX = NTW * NTH / 256; // pixels per thread
constexpr uint32_t NORMALS_MAX_SIDE = 65535;

struct RayCam {
    double d0[3], dx[3], dy[3]; // d(x, y) = d0 + x dx + y dy
    double a[3], b[3], c[3];    // d0 x dx, dy x d0, dy x dx
    float sigma;
    int distance; // depth is |P - eye| (else clip w)
};
struct DepthMap {
    const float *z;
    int w, h;
};
// the loss's other inputs: the blended normal map F (pointer, pixel stride), the optional weight, -upstream / (W H) read on the device
struct NormalTerm {
    const float *map;
    uint32_t ms;
    const float *weight;
};

struct PxNormal {
    float n[3];           // the unit normal; 0 when !valid
    float rn;             // 1 / |n|
    float dx, sx, dy, sy; // s_r - s_l, s_r + s_l, s_d - s_u, s_d + s_u
    float p[3], q[3], c[3];
    bool valid;
};

__device__ __forceinline__ bool ray_ok(float s) { return s > 0.0f && s <= 3.402823466e38f; }

// The normal at pixel (x, y) of a w x h screen from the ray parameters of its left, right, upper and lower neighbours.
__device__ __forceinline__ PxNormal pixel_normal(const RayCam &cam, int x, int y, int w, int h, float sl, float sr, float su, float sd) {
    PxNormal r;
    r.valid = x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2 && ray_ok(sl) && ray_ok(sr) && ray_ok(su) && ray_ok(sd);
    r.dx = sr - sl; r.sx = sr + sl; r.dy = sd - su; r.sy = sd + su;
    const float kp = r.dy * r.sx, kq = r.sy * r.dx, kc = r.sy * r.sx;
    float n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r.p[i] = (float)fma((double)y, cam.c[i], cam.a[i]);
        r.q[i] = (float)fma((double)x, cam.c[i], cam.b[i]);
        r.c[i] = (float)cam.c[i];
        n[i] = cam.sigma * fmaf(kp, r.p[i], fmaf(kq, r.q[i], kc * r.c[i]));
    }
    const float nn = fmaf(n[0], n[0], fmaf(n[1], n[1], n[2] * n[2]));
    r.valid = r.valid && nn > 0.0f && nn <= 3.402823466e38f;
    r.rn = 1.0f / sqrtf(nn);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.n[i] = r.valid ? n[i] * r.rn : 0.0f;
    return r;
}

// dL/d(s_l, s_r, s_u, s_d) of a VALID pixel from dL/dN
__device__ __forceinline__ void pixel_normal_backward(const RayCam &cam, const PxNormal &r, const float gN[3], float out[4]) {
    const float t = fmaf(r.n[0], gN[0], fmaf(r.n[1], gN[1], r.n[2] * gN[2]));
    float gp = 0.0f, gq = 0.0f, gc = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float gn = fmaf(-r.n[i], t, gN[i]) * r.rn; // dL/dn: the part of gN across N, over |n|
        gp = fmaf(gn, r.p[i], gp);
        gq = fmaf(gn, r.q[i], gq);
        gc = fmaf(gn, r.c[i], gc);
    }
    const float across = fmaf(r.dy, gp, r.sy * gc), along = r.sy * gq; // d/ds_r = across + along, d/ds_l = across - along
    const float down = fmaf(r.dx, gq, r.sx * gc), side = r.sx * gp;    // d/ds_d = down + side,    d/ds_u = down - side
    out[0] = cam.sigma * (across - along);
    out[1] = cam.sigma * (across + along);
    out[2] = cam.sigma * (down - side);
    out[3] = cam.sigma * (down + side);
}

// The ray parameters (and, when s_inv is given, ds/ddepth) of the tile at (tx0, ty0) with its halo, by rows; 0 outside the screen
template <int HALO>
__device__ __forceinline__ void stage_rays(const RayCam &cam, const DepthMap &dm, int tx0, int ty0, float *__restrict__ s_s, float *__restrict__ s_inv) {
    constexpr int SW = NTW + 2 * HALO, SH = NTH + 2 * HALO;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const int gx = tx0 - HALO + c, gy = ty0 - HALO + r;
        float s = 0.0f, inv = 0.0f;
        if (gx >= 0 && gx < dm.w && gy >= 0 && gy < dm.h) {
            const float z = dm.z[(size_t)gy * dm.w + gx];
            if (cam.distance) {
                double dd = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double d = fma((double)gy, cam.dy[k], fma((double)gx, cam.dx[k], cam.d0[k]));
                    dd = fma(d, d, dd);
                }
                const double iv = 1.0 / sqrt(dd);
                s = (float)((double)z * iv);
                inv = (float)iv;
            } else {
                s = z;
                inv = 1.0f;
            }
        }
        s_s[i] = s;
        if (s_inv) s_inv[i] = inv;
    }
}

// LOSS = false: the map, N to the first three floats of every pixel of (normals, ns).
// LOSS = true: per workgroup the float64 partials {sum over valid pixels of w F . N, number of valid pixels} to part.
template <bool LOSS>
__global__ __launch_bounds__(256) void k_depth_normals(RayCam cam, DepthMap dm, float *__restrict__ normals, uint32_t ns, NormalTerm in,
                                                       double *__restrict__ part) {
    __shared__ float s_s[NTH + 2][NTW + 2];
    __shared__ double s_red[4][2];
    const int tid = threadIdx.x, tx0 = blockIdx.x * NTW, ty0 = blockIdx.y * NTH;
    const int px = tid & (NTW - 1), py0 = tid / NTW;
    stage_rays<1>(cam, dm, tx0, ty0, &s_s[0][0], nullptr);
    __syncthreads();
    const bool mv = LOSS && is_vec4(in.map, in.ms);
    double dot = 0.0, cnt = 0.0;
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
        const int py = py0 + j * (256 / NTW), gx = tx0 + px, gy = ty0 + py;
        if (gx < dm.w && gy < dm.h) {
            const PxNormal r = pixel_normal(cam, gx, gy, dm.w, dm.h, s_s[py + 1][px], s_s[py + 1][px + 2], s_s[py][px + 1], s_s[py + 2][px + 1]);
            const size_t p = (size_t)gy * dm.w + gx;
            if constexpr (LOSS) {
                if (r.valid) { // (an invalid pixel's F and w are not read: NaN there is harmless)
                    const Px3 f = load_px(in.map, in.ms, mv, p);
                    const float wv = in.weight ? in.weight[p] : 1.0f;
                    dot += (double)(wv * fmaf(f.c[0], r.n[0], fmaf(f.c[1], r.n[1], f.c[2] * r.n[2])));
                    cnt += 1.0;
                }
            } else {
                float *o = normals + p * ns;
                o[0] = r.n[0]; o[1] = r.n[1]; o[2] = r.n[2];
            }
        }
    }
    if constexpr (LOSS) {
        dot = wave_sum_f64(dot);
        cnt = wave_sum_f64(cnt);
        if ((tid & 63) == 0) {
            s_red[tid >> 6][0] = dot;
            s_red[tid >> 6][1] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            double *dst = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
            dst[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
            dst[1] = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
        }
    }
}

// The workgroups' partials, added in index order (thread t its contiguous share, then the 256 shares in order) and rounded once:
// out = {1 - sum / (W H), valid / (W H), 0, 0}
__global__ __launch_bounds__(256) void k_normal_loss_sum(const double *__restrict__ part, uint32_t nparts, double inv_n, float *__restrict__ out) {
    __shared__ double s_sum[256][2];
    const uint32_t t = threadIdx.x, per = (nparts + 255u) / 256u;
    const uint32_t b0 = min(t * per, nparts), b1 = min(b0 + per, nparts);
    double d = 0.0, v = 0.0;
    for (uint32_t b = b0; b < b1; ++b) {
        d += part[2 * (size_t)b];
        v += part[2 * (size_t)b + 1];
    }
    s_sum[t][0] = d;
    s_sum[t][1] = v;
    __syncthreads();
    if (t == 0) {
        d = 0.0;
        v = 0.0;
        for (int q = 0; q < 256; ++q) {
            d += s_sum[q][0];
            v += s_sum[q][1];
        }
        out[0] = (float)(1.0 - d * inv_n);
        out[1] = (float)(v * inv_n);
        out[2] = 0.0f;
        out[3] = 0.0f;
    }
}

// dL/ddepth of every pixel of the tile (overwritten), gathered from the normals of its four neighbours.
// LOSS = false: dL/dN is (gN, gs).  LOSS = true: dL/dN_p = k w_p F_p with k = -upstream[0] inv_n, and the first three floats of
// every pixel of (grad_map, gms) receive dL/dF_p = k w_p N_p (0 at an invalid pixel).
template <bool LOSS>
__global__ __launch_bounds__(256) void k_depth_normals_backward(RayCam cam, DepthMap dm, const float *__restrict__ gN, uint32_t gs, NormalTerm in,
                                                                const float *__restrict__ upstream, float inv_n, float *__restrict__ grad_map,
                                                                uint32_t gms, float *__restrict__ grad_depth) {
    __shared__ float s_s[NTH + 4][NTW + 4], s_inv[NTH + 4][NTW + 4];
    __shared__ float s_g[4][NTH + 2][NTW + 2];
    const int tid = threadIdx.x, tx0 = blockIdx.x * NTW, ty0 = blockIdx.y * NTH;
    stage_rays<2>(cam, dm, tx0, ty0, &s_s[0][0], &s_inv[0][0]);
    __syncthreads();
    const bool mv = LOSS && is_vec4(in.map, in.ms), gv = !LOSS && is_vec4(gN, gs);
    float k = 0.0f;
    if constexpr (LOSS) k = -upstream[0] * inv_n;

    // every pixel of the tile and its halo 1: the derivatives with respect to its four neighbours' ray parameters
    for (int i = tid; i < (NTH + 2) * (NTW + 2); i += 256) {
        const int r = i / (NTW + 2), c = i - r * (NTW + 2);
        const int gx = tx0 - 1 + c, gy = ty0 - 1 + r;
        float g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (gx >= 0 && gx < dm.w && gy >= 0 && gy < dm.h) {
            const PxNormal pn = pixel_normal(cam, gx, gy, dm.w, dm.h, s_s[r + 1][c], s_s[r + 1][c + 2], s_s[r][c + 1], s_s[r + 2][c + 1]);
            const size_t p = (size_t)gy * dm.w + gx;
            float kw = 0.0f;
            if (pn.valid) { // (an invalid pixel's upstream, F and w are not read: it is selected away, not multiplied by zero)
                float g[3];
                if constexpr (LOSS) {
                    const Px3 f = load_px(in.map, in.ms, mv, p);
                    kw = in.weight ? k * in.weight[p] : k;
                    g[0] = kw * f.c[0]; g[1] = kw * f.c[1]; g[2] = kw * f.c[2];
                } else {
                    const Px3 u = load_px(gN, gs, gv, p);
                    g[0] = u.c[0]; g[1] = u.c[1]; g[2] = u.c[2];
                }
                pixel_normal_backward(cam, pn, g, g4);
            }
            if constexpr (LOSS) {
                if (r >= 1 && r <= NTH && c >= 1 && c <= NTW) { // the tile's own pixel: dL/dF
                    float *o = grad_map + p * gms;
                    o[0] = pn.valid ? kw * pn.n[0] : 0.0f;
                    o[1] = pn.valid ? kw * pn.n[1] : 0.0f;
                    o[2] = pn.valid ? kw * pn.n[2] : 0.0f;
                }
            }
        }
        s_g[0][r][c] = g4[0]; s_g[1][r][c] = g4[1]; s_g[2][r][c] = g4[2]; s_g[3][r][c] = g4[3];
    }
    __syncthreads();

    // q is the left neighbour of q + (1, 0), the right one of q - (1, 0), the upper one of q + (0, 1), the lower one of q - (0, 1):
    // added in that order
    const int px = tid & (NTW - 1), py0 = tid / NTW;
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
        const int py = py0 + j * (256 / NTW), gx = tx0 + px, gy = ty0 + py;
        if (gx < dm.w && gy < dm.h) {
            const float sum = ((s_g[0][py + 1][px + 2] + s_g[1][py + 1][px]) + s_g[2][py + 2][px + 1]) + s_g[3][py][px + 1];
            const float sq = s_s[py + 2][px + 2];
            grad_depth[(size_t)gy * dm.w + gx] = fabsf(sq) <= 3.402823466e38f ? sum * s_inv[py + 2][px + 2] : 0.0f; // (false for a NaN)
        }
    }
}

void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// {D0, Dx, Dy, sigma} of the uniform block's VP on a width x height screen, or why there are none
int camera_rays(splat_ctx *ctx, const float *uniforms, uint32_t width, uint32_t height, double out10[10]) {
    // the block stores VP by columns: VP[r][c] = uniforms[4 c + r]; M = rows 0, 1, 3 of VP on xyz
    const int rows[3] = {0, 1, 3};
    double m[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = (double)uniforms[4 * j + rows[i]];
    double cof[3][3]; // cof[i] = m[i+1] x m[i+2]: the columns of det(M) M^-1
    cross3(m[1], m[2], cof[0]);
    cross3(m[2], m[0], cof[1]);
    cross3(m[0], m[1], cof[2]);
    const double det = dot3(m[0], cof[0]);
    const double scale = sqrt(dot3(m[0], m[0]) * dot3(m[1], m[1]) * dot3(m[2], m[2]));
    if (!(fabs(det) > 1e-14 * scale) || !(scale <= 1.7976931348623157e308))
        return ctx_fail(ctx, SPLAT_ERR_INVALID,
                        "camera rays: rows 0, 1, 3 of VP are singular on xyz (an orthographic VP has no eye that every ray leaves: only "
                        "perspective cameras have depth-map normals here)");
    const double W = (double)width, H = (double)height;
    // d(x, y) = M^-1 (2 (x + 1/2) / W - 1, 1 - 2 (y + 1/2) / H, 1)
    const double v0[3] = {1.0 / W - 1.0, 1.0 - 1.0 / H, 1.0}, vx[3] = {2.0 / W, 0.0, 0.0}, vy[3] = {0.0, -2.0 / H, 0.0};
    double *d0 = out10, *dx = out10 + 3, *dy = out10 + 6, dc[3], yx[3];
    for (int k = 0; k < 3; ++k) {
        d0[k] = (cof[0][k] * v0[0] + cof[1][k] * v0[1] + cof[2][k] * v0[2]) / det;
        dx[k] = cof[0][k] * vx[0] / det;
        dy[k] = cof[1][k] * vy[1] / det;
        dc[k] = cof[2][k] / det; // the ray of the screen's centre, M^-1 (0, 0, 1)
    }
    cross3(dy, dx, yx);
    const double hand = dot3(yx, dc);
    out10[9] = hand < 0.0 ? 1.0 : hand > 0.0 ? -1.0 : 0.0;
    if (out10[9] == 0.0 || !(fabs(hand) <= 1.7976931348623157e308))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "camera rays: (Dy x Dx) . d_centre is 0 or not finite: the screen's axes and the central ray span no volume");
    return SPLAT_OK;
}

int ray_cam(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, uint32_t width, uint32_t height, RayCam *cam) {
    ARG_CHECK(ctx, uniforms != nullptr);
    ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= NORMALS_MAX_SIDE && height <= NORMALS_MAX_SIDE);
    ARG_CHECK(ctx, depth_kind == SPLAT_DEPTH_DISTANCE || depth_kind == SPLAT_DEPTH_Z);
    double r[10];
    const int rc = camera_rays(ctx, uniforms, width, height, r);
    if (rc != SPLAT_OK) return rc;
    for (int k = 0; k < 3; ++k) cam->d0[k] = r[k], cam->dx[k] = r[3 + k], cam->dy[k] = r[6 + k];
    cross3(cam->d0, cam->dx, cam->a);
    cross3(cam->dy, cam->d0, cam->b);
    cross3(cam->dy, cam->dx, cam->c);
    cam->sigma = (float)r[9];
    cam->distance = depth_kind == SPLAT_DEPTH_DISTANCE;
    return SPLAT_OK;
}

bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

} // namespace

extern "C" int splat_camera_rays(const float *uniforms, double *out10) {
    if (!uniforms || !out10) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "splat_camera_rays: uniforms or out10 is NULL");
    const float w = uniforms[20], h = uniforms[21];
    if (!(w >= 1.0f && h >= 1.0f && w <= (float)NORMALS_MAX_SIDE && h <= (float)NORMALS_MAX_SIDE && w == floorf(w) && h == floorf(h)))
        return ctx_fail(nullptr, SPLAT_ERR_INVALID, "splat_camera_rays: uniforms[20], uniforms[21] must hold a screen of 1 to 65535 pixels a side");
    return camera_rays(nullptr, uniforms, (uint32_t)w, (uint32_t)h, out10);
}

extern "C" int splat_depth_normals(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, uint32_t width, uint32_t height,
                                   void *normals, uint32_t normal_stride) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    RayCam cam;
    const int rc = ray_cam(ctx, uniforms, depth_kind, width, height, &cam);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, depth && normals && normal_stride >= 3 && aligned4(depth) && aligned4(normals));
    const DepthMap dm{(const float *)depth, (int)width, (int)height};
    hipLaunchKernelGGL(k_depth_normals<false>, dim3(div_up(width, NTW), div_up(height, NTH)), dim3(256), 0, ctx->stream, cam, dm, (float *)normals,
                       normal_stride, NormalTerm{nullptr, 0, nullptr}, (double *)nullptr);
    LAUNCH_CHECK(ctx, "k_depth_normals");
    return SPLAT_OK;
}

extern "C" int splat_depth_normals_backward(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, uint32_t width,
                                            uint32_t height, const void *grad_normals, uint32_t grad_stride, void *grad_depth) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    RayCam cam;
    const int rc = ray_cam(ctx, uniforms, depth_kind, width, height, &cam);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, depth && grad_normals && grad_depth && grad_stride >= 3 && aligned4(depth) && aligned4(grad_normals) && aligned4(grad_depth));
    const DepthMap dm{(const float *)depth, (int)width, (int)height};
    hipLaunchKernelGGL(k_depth_normals_backward<false>, dim3(div_up(width, NTW), div_up(height, NTH)), dim3(256), 0, ctx->stream, cam, dm,
                       (const float *)grad_normals, grad_stride, NormalTerm{nullptr, 0, nullptr}, (const float *)nullptr, 0.0f, (float *)nullptr, 0u,
                       (float *)grad_depth);
    LAUNCH_CHECK(ctx, "k_depth_normals_backward");
    return SPLAT_OK;
}

extern "C" int splat_normal_consistency(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, const void *normal_map,
                                        uint32_t map_stride, const void *weight, uint32_t width, uint32_t height, void *out4) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    RayCam cam;
    int rc = ray_cam(ctx, uniforms, depth_kind, width, height, &cam);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, depth && normal_map && out4 && map_stride >= 3);
    ARG_CHECK(ctx, aligned4(depth) && aligned4(normal_map) && aligned4(weight) && aligned4(out4));
    const dim3 grid(div_up(width, NTW), div_up(height, NTH));
    const uint32_t nparts = grid.x * grid.y;
    rc = ctx_ensure_scan_ws(ctx, (size_t)nparts * 2 * sizeof(double));
    if (rc != SPLAT_OK) return rc;
    double *part = (double *)ctx->scan_ws;
    const DepthMap dm{(const float *)depth, (int)width, (int)height};
    hipLaunchKernelGGL(k_depth_normals<true>, grid, dim3(256), 0, ctx->stream, cam, dm, (float *)nullptr, 0u,
                       NormalTerm{(const float *)normal_map, map_stride, (const float *)weight}, part);
    LAUNCH_CHECK(ctx, "k_depth_normals");
    hipLaunchKernelGGL(k_normal_loss_sum, dim3(1), dim3(256), 0, ctx->stream, part, nparts, 1.0 / ((double)width * (double)height), (float *)out4);
    LAUNCH_CHECK(ctx, "k_normal_loss_sum");
    return SPLAT_OK;
}

extern "C" int splat_normal_consistency_backward(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth,
                                                 const void *normal_map, uint32_t map_stride, const void *weight, uint32_t width, uint32_t height,
                                                 const void *upstream, void *grad_map, uint32_t grad_map_stride, void *grad_depth) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    RayCam cam;
    const int rc = ray_cam(ctx, uniforms, depth_kind, width, height, &cam);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, depth && normal_map && upstream && grad_map && grad_depth && map_stride >= 3 && grad_map_stride >= 3);
    ARG_CHECK(ctx, aligned4(depth) && aligned4(normal_map) && aligned4(weight) && aligned4(upstream) && aligned4(grad_map) && aligned4(grad_depth));
    const DepthMap dm{(const float *)depth, (int)width, (int)height};
    hipLaunchKernelGGL(k_depth_normals_backward<true>, dim3(div_up(width, NTW), div_up(height, NTH)), dim3(256), 0, ctx->stream, cam, dm,
                       (const float *)nullptr, 0u, NormalTerm{(const float *)normal_map, map_stride, (const float *)weight}, (const float *)upstream,
                       (float)(1.0 / ((double)width * (double)height)), (float *)grad_map, grad_map_stride, (float *)grad_depth);
    LAUNCH_CHECK(ctx, "k_depth_normals_backward");
    return SPLAT_OK;
}
