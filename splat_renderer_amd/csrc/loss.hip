// loss.hip — the photometric loss of 3D Gaussian splatting between a rendered image x and a target y (an extension, no
// reference counterpart): loss = (1 - lambda) mean|x - y| + lambda (1 - mean SSIM), SSIM over an 11 x 11 Gaussian window of
// sigma 1.5 with zero padding, per channel (include/splat.h, "Image loss", states the formulas).
//
// Images are (pointer, pixel stride in floats), channels in the first three words of a pixel; a fourth word may be loaded
// (one float4 load where stride and base allow it) but never enters a result and is never written.
//
// k_image_loss, one launch over tiles of 32 x 16 pixels (256 threads, two pixels each): the tile and its 5-pixel halo of x and
// y go to LDS, then per channel the horizontal pass makes the five window sums (x, y, xx, yy, xy) of every staged row and the
// vertical pass finishes them for the thread's two pixels, which evaluate the SSIM map m and its three derivative maps
// (dm/dmu_x, dm/dsigma_x, dm/dsigma_xy: 9 floats per pixel, stored as planes in the caller's workspace for the backward).
// In a tile whose halo lies inside the image the window sums are taken of x - cx and y - cy, cx and cy the tile's centre
// pixel: the window's weights sum to 1, so the variances conv(x^2) - mu^2 are the same numbers, formed without the
// cancellation of two values near cx^2 where the image is locally flat (the end of a fit; a frame that is still all
// background).  Tiles that see the zero padding sum x and y as they are.
// sum m and sum |x - y| leave each workgroup as two float64 partials in a slot of its own; k_image_loss_sum adds the slots
// in index order and rounds once: no atomics, the same bits for the same inputs.
//
// k_image_loss_backward is a gather over the same tiles: per channel it convolves the three stored maps (zero outside the
// image: the window is its own adjoint) and adds the L1 term, scaled by the upstream gradient it reads from device memory.
// No atomics either.
//
// Roofline: both kernels are bound by their LDS passes, not by HBM ("Loss", has the measured times beside
// the traffic floors).
#include "common.h"
#include "image.h"

namespace {

constexpr int LR = 5, LK = 2 * LR + 1;               // the window: radius, taps
constexpr int LTW = 32, LTH = 16;                      // a workgroup's tile
constexpr int LSW = LTW + 2 * LR, LSH = LTH + 2 * LR;  // the tile with its halo
constexpr int LPX = LTW * LTH / 256;                   // pixels per thread
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct LossWindow {
    float g[LK];
};
struct LossImages {
    const float *x, *y;
    uint32_t xs, ys, w, h;
};
template <bool SSIM>
__global__ __launch_bounds__(256) void k_image_loss(LossImages im, LossWindow win, float *__restrict__ ws, double *__restrict__ part) {
    __shared__ float s_x[SSIM ? 3 : 1][SSIM ? LSH : 1][SSIM ? LSW : 1], s_y[SSIM ? 3 : 1][SSIM ? LSH : 1][SSIM ? LSW : 1];
    __shared__ float s_h[SSIM ? 5 : 1][SSIM ? LSH : 1][SSIM ? LTW : 1];
    __shared__ double s_red[4][2];
    const int tid = threadIdx.x, w = (int)im.w, h = (int)im.h;
    const int tx0 = blockIdx.x * LTW, ty0 = blockIdx.y * LTH;
    const bool xv = is_vec4(im.x, im.xs), yv = is_vec4(im.y, im.ys);
    const size_t plane = (size_t)im.w * im.h;
    const int px = tid & (LTW - 1), py0 = tid / LTW;

    // the thread's own pixels, as given: the L1 term and the derivative maps' home
    Px3 ox[LPX], oy[LPX];
    bool in[LPX];
    double l1 = 0.0, msum = 0.0;
#pragma unroll
    for (int j = 0; j < LPX; ++j) {
        const int gx = tx0 + px, gy = ty0 + py0 + j * (256 / LTW);
        in[j] = gx < w && gy < h;
        if (in[j]) {
            const size_t p = (size_t)gy * im.w + gx;
            ox[j] = load_px(im.x, im.xs, xv, p);
            oy[j] = load_px(im.y, im.ys, yv, p);
            float a = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) a += fabsf(ox[j].c[c] - oy[j].c[c]);
            l1 += (double)a;
        }
    }

    if constexpr (SSIM) {
        // (a tile whose halo leaves the image keeps cx = cy = 0: there the padding would turn from exact zeros into -cx, and
        // mu_x = conv(x - cx) + cx would lose bits where the padding outweighs the image, at most on images below the window)
        const bool inner = tx0 >= LR && ty0 >= LR && tx0 + LTW + LR <= w && ty0 + LTH + LR <= h;
        Px3 cx = {{0.0f, 0.0f, 0.0f}}, cy = {{0.0f, 0.0f, 0.0f}};
        if (inner) {
            const size_t pc = (size_t)(ty0 + LTH / 2) * im.w + (tx0 + LTW / 2);
            cx = load_px(im.x, im.xs, xv, pc);
            cy = load_px(im.y, im.ys, yv, pc);
        }
        for (int i = tid; i < LSH * LSW; i += 256) {
            const int r = i / LSW, c = i - r * LSW;
            const int gy = ty0 - LR + r, gx = tx0 - LR + c;
            Px3 vx = {{0.0f, 0.0f, 0.0f}}, vy = {{0.0f, 0.0f, 0.0f}};
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const size_t p = (size_t)gy * im.w + gx;
                vx = load_px(im.x, im.xs, xv, p);
                vy = load_px(im.y, im.ys, yv, p);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                s_x[ch][r][c] = vx.c[ch] - cx.c[ch];
                s_y[ch][r][c] = vy.c[ch] - cy.c[ch];
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            for (int i = tid; i < LSH * LTW; i += 256) {
                const int r = i / LTW, c = i & (LTW - 1);
                float a = 0.0f, b = 0.0f, aa = 0.0f, bb = 0.0f, ab = 0.0f;
#pragma unroll
                for (int k = 0; k < LK; ++k) {
                    const float u = s_x[ch][r][c + k], v = s_y[ch][r][c + k];
                    const float gu = win.g[k] * u, gv = win.g[k] * v;
                    a += gu;
                    b += gv;
                    aa = fmaf(gu, u, aa);
                    bb = fmaf(gv, v, bb);
                    ab = fmaf(gu, v, ab);
                }
                s_h[0][r][c] = a; s_h[1][r][c] = b; s_h[2][r][c] = aa; s_h[3][r][c] = bb; s_h[4][r][c] = ab;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LPX; ++j) {
                const int py = py0 + j * (256 / LTW);
                float a = 0.0f, b = 0.0f, aa = 0.0f, bb = 0.0f, ab = 0.0f;
#pragma unroll
                for (int k = 0; k < LK; ++k) {
                    const float g = win.g[k];
                    a = fmaf(g, s_h[0][py + k][px], a);
                    b = fmaf(g, s_h[1][py + k][px], b);
                    aa = fmaf(g, s_h[2][py + k][px], aa);
                    bb = fmaf(g, s_h[3][py + k][px], bb);
                    ab = fmaf(g, s_h[4][py + k][px], ab);
                }
                if (in[j]) {
                    const float sx = fmaf(-a, a, aa), sy = fmaf(-b, b, bb), sxy = fmaf(-a, b, ab);
                    const float mx = a + cx.c[ch], my = b + cy.c[ch];
                    const float A = fmaf(2.0f * mx, my, SSIM_C1), B = fmaf(2.0f, sxy, SSIM_C2);
                    const float Cc = fmaf(mx, mx, fmaf(my, my, SSIM_C1)), D = sx + sy + SSIM_C2;
                    const float rcd = 1.0f / (Cc * D);
                    const float m = A * B * rcd;
                    msum += (double)m;
                    const size_t p = (size_t)(ty0 + py) * im.w + (tx0 + px);
                    // dm/dmu_x = 2 mu_y (B - A) / (C D) + 2 mu_x m (1 / D - 1 / C), on the common denominator
                    ws[(size_t)(0 + ch) * plane + p] = 2.0f * rcd * fmaf(my, B - A, mx * m * (Cc - D));
                    ws[(size_t)(3 + ch) * plane + p] = -m / D;
                    ws[(size_t)(6 + ch) * plane + p] = 2.0f * A * rcd;
                }
            }
            __syncthreads();
        }
    }

    l1 = wave_sum_f64(l1);
    msum = wave_sum_f64(msum);
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = l1;
        s_red[tid >> 6][1] = msum;
    }
    __syncthreads();
    if (tid == 0) {
        double *dst = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        dst[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
        dst[1] = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
    }
}

// The workgroups' partials {sum |x - y|, sum m}, added in index order (thread t its contiguous share, then the 256 shares in
// order) and rounded once: out = {loss, l1, ssim, 0}; ssim NaN when the SSIM part did not run (lambda = 0 without a workspace).
__global__ __launch_bounds__(256) void k_image_loss_sum(const double *__restrict__ part, uint32_t nparts, double inv_n, float lambda, int ssim,
                                                        float *__restrict__ out) {
    __shared__ double s_sum[256][2];
    const uint32_t t = threadIdx.x, per = (nparts + 255u) / 256u;
    const uint32_t b0 = min(t * per, nparts), b1 = min(b0 + per, nparts);
    double l = 0.0, m = 0.0;
    for (uint32_t b = b0; b < b1; ++b) {
        l += part[2 * (size_t)b];
        m += part[2 * (size_t)b + 1];
    }
    s_sum[t][0] = l;
    s_sum[t][1] = m;
    __syncthreads();
    if (t == 0) {
        l = 0.0;
        m = 0.0;
        for (int q = 0; q < 256; ++q) {
            l += s_sum[q][0];
            m += s_sum[q][1];
        }
        const double l1 = l * inv_n, ss = m * inv_n, lam = (double)lambda;
        out[0] = (float)(ssim ? (1.0 - lam) * l1 + lam * (1.0 - ss) : (1.0 - lam) * l1);
        out[1] = (float)l1;
        out[2] = ssim ? (float)ss : __builtin_nanf("");
        out[3] = 0.0f;
    }
}

template <bool SSIM>
__global__ __launch_bounds__(256) void k_image_loss_backward(LossImages im, LossWindow win, const float *__restrict__ ws,
                                                             const float *__restrict__ upstream, float lambda, float inv_n,
                                                             float *__restrict__ grad, uint32_t gs) {
    __shared__ float s_d[SSIM ? 3 : 1][SSIM ? LSH : 1][SSIM ? LSW : 1];
    __shared__ float s_h[SSIM ? 3 : 1][SSIM ? LSH : 1][SSIM ? LTW : 1];
    const int tid = threadIdx.x, w = (int)im.w, h = (int)im.h;
    const int tx0 = blockIdx.x * LTW, ty0 = blockIdx.y * LTH;
    const bool xv = is_vec4(im.x, im.xs), yv = is_vec4(im.y, im.ys);
    const size_t plane = (size_t)im.w * im.h;
    const int px = tid & (LTW - 1), py0 = tid / LTW;
    const float up = upstream[0];
    const float kl = up * (1.0f - lambda) * inv_n, ks = up * lambda * inv_n;

    Px3 ox[LPX], oy[LPX], g[LPX];
    bool in[LPX];
#pragma unroll
    for (int j = 0; j < LPX; ++j) {
        const int gx = tx0 + px, gy = ty0 + py0 + j * (256 / LTW);
        in[j] = gx < w && gy < h;
        if (in[j]) {
            const size_t p = (size_t)gy * im.w + gx;
            ox[j] = load_px(im.x, im.xs, xv, p);
            oy[j] = load_px(im.y, im.ys, yv, p);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = ox[j].c[c] - oy[j].c[c];
                g[j].c[c] = d > 0.0f ? kl : d < 0.0f ? -kl : 0.0f * d; // (sign(0) = 0; a NaN stays one)
            }
        }
    }

    if constexpr (SSIM) {
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
            for (int i = tid; i < LSH * LSW; i += 256) {
                const int r = i / LSW, c = i - r * LSW;
                const int gy = ty0 - LR + r, gx = tx0 - LR + c;
                float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
                if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                    const size_t p = (size_t)gy * im.w + gx;
                    d0 = ws[(size_t)(0 + ch) * plane + p];
                    d1 = ws[(size_t)(3 + ch) * plane + p];
                    d2 = ws[(size_t)(6 + ch) * plane + p];
                }
                s_d[0][r][c] = d0; s_d[1][r][c] = d1; s_d[2][r][c] = d2;
            }
            __syncthreads();
            for (int i = tid; i < LSH * LTW; i += 256) {
                const int r = i / LTW, c = i & (LTW - 1);
                float a = 0.0f, b = 0.0f, e = 0.0f;
#pragma unroll
                for (int k = 0; k < LK; ++k) {
                    const float gk = win.g[k];
                    a = fmaf(gk, s_d[0][r][c + k], a);
                    b = fmaf(gk, s_d[1][r][c + k], b);
                    e = fmaf(gk, s_d[2][r][c + k], e);
                }
                s_h[0][r][c] = a; s_h[1][r][c] = b; s_h[2][r][c] = e;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LPX; ++j) {
                const int py = py0 + j * (256 / LTW);
                float a = 0.0f, b = 0.0f, e = 0.0f;
#pragma unroll
                for (int k = 0; k < LK; ++k) {
                    const float gk = win.g[k];
                    a = fmaf(gk, s_h[0][py + k][px], a);
                    b = fmaf(gk, s_h[1][py + k][px], b);
                    e = fmaf(gk, s_h[2][py + k][px], e);
                }
                if (in[j]) {
                    // (ch is a loop counter, not a constant: select, so that g stays in registers)
                    const float xc = ch == 0 ? ox[j].c[0] : ch == 1 ? ox[j].c[1] : ox[j].c[2];
                    const float yc = ch == 0 ? oy[j].c[0] : ch == 1 ? oy[j].c[1] : oy[j].c[2];
                    const float s = ks * fmaf(2.0f * xc, b, fmaf(yc, e, a));
                    if (ch == 0) g[j].c[0] -= s;
                    else if (ch == 1) g[j].c[1] -= s;
                    else g[j].c[2] -= s;
                }
            }
            // (the next channel's staging writes s_d, which no thread reads after the second barrier above; its horizontal
            // pass writes s_h only after its own first barrier, which every thread reaches after this vertical pass)
        }
    }

#pragma unroll
    for (int j = 0; j < LPX; ++j) {
        if (in[j]) {
            float *q = grad + ((size_t)(ty0 + py0 + j * (256 / LTW)) * im.w + (tx0 + px)) * gs;
            q[0] = g[j].c[0]; q[1] = g[j].c[1]; q[2] = g[j].c[2];
        }
    }
}

LossWindow loss_window() {
    double g[LK], s = 0.0;
    for (int k = 0; k < LK; ++k) s += g[k] = exp(-(double)((k - LR) * (k - LR)) / (2.0 * 1.5 * 1.5));
    LossWindow win;
    for (int k = 0; k < LK; ++k) win.g[k] = (float)(g[k] / s);
    return win;
}

constexpr uint32_t LOSS_MAX_SIDE = 65535;

int loss_args(splat_ctx *ctx, const void *image, uint32_t image_stride, const void *target, uint32_t target_stride, uint32_t width,
              uint32_t height, float lambda) {
    ARG_CHECK(ctx, image && target && image_stride >= 3 && target_stride >= 3);
    ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= LOSS_MAX_SIDE && height <= LOSS_MAX_SIDE);
    ARG_CHECK(ctx, lambda >= 0.0f && lambda <= 1.0f); // (false for a NaN)
    ARG_CHECK(ctx, (((uintptr_t)image | (uintptr_t)target) & 3) == 0);
    return SPLAT_OK;
}

} // namespace

extern "C" uint64_t splat_image_loss_workspace_bytes(uint32_t width, uint32_t height) {
    return ((uint64_t)width * height * 9u * sizeof(float) + 15u) & ~(uint64_t)15u;
}

extern "C" int splat_image_loss(splat_ctx *ctx, const void *image, uint32_t image_stride, const void *target, uint32_t target_stride,
                                uint32_t width, uint32_t height, float lambda, void *workspace, uint64_t workspace_bytes, void *out4) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    int rc = loss_args(ctx, image, image_stride, target, target_stride, width, height, lambda);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, out4 && ((uintptr_t)out4 & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
    const bool ssim = workspace != nullptr || lambda > 0.0f;
    if (ssim && (!workspace || workspace_bytes < splat_image_loss_workspace_bytes(width, height)))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_image_loss: the workspace is smaller than splat_image_loss_workspace_bytes(width, height)");
    const dim3 grid(div_up(width, LTW), div_up(height, LTH));
    const uint32_t nparts = grid.x * grid.y;
    rc = ctx_ensure_scan_ws(ctx, (size_t)nparts * 2 * sizeof(double));
    if (rc != SPLAT_OK) return rc;
    double *part = (double *)ctx->scan_ws;
    const LossImages im{(const float *)image, (const float *)target, image_stride, target_stride, width, height};
    if (ssim) hipLaunchKernelGGL(k_image_loss<true>, grid, dim3(256), 0, ctx->stream, im, loss_window(), (float *)workspace, part);
    else hipLaunchKernelGGL(k_image_loss<false>, grid, dim3(256), 0, ctx->stream, im, loss_window(), (float *)nullptr, part);
    LAUNCH_CHECK(ctx, "k_image_loss");
    hipLaunchKernelGGL(k_image_loss_sum, dim3(1), dim3(256), 0, ctx->stream, part, nparts, 1.0 / (3.0 * (double)width * (double)height), lambda,
                       ssim ? 1 : 0, (float *)out4);
    LAUNCH_CHECK(ctx, "k_image_loss_sum");
    return SPLAT_OK;
}

extern "C" int splat_image_loss_backward(splat_ctx *ctx, const void *image, uint32_t image_stride, const void *target, uint32_t target_stride,
                                         uint32_t width, uint32_t height, float lambda, const void *workspace, uint64_t workspace_bytes,
                                         const void *upstream, void *grad_image, uint32_t grad_stride) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    const int rc = loss_args(ctx, image, image_stride, target, target_stride, width, height, lambda);
    if (rc != SPLAT_OK) return rc;
    ARG_CHECK(ctx, upstream && grad_image && grad_stride >= 3);
    ARG_CHECK(ctx, (((uintptr_t)upstream | (uintptr_t)grad_image) & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
    const bool ssim = lambda > 0.0f;
    if (ssim && (!workspace || workspace_bytes < splat_image_loss_workspace_bytes(width, height)))
        return ctx_fail(ctx, SPLAT_ERR_INVALID,
                        "splat_image_loss_backward: the workspace is smaller than splat_image_loss_workspace_bytes(width, height)");
    const dim3 grid(div_up(width, LTW), div_up(height, LTH));
    const LossImages im{(const float *)image, (const float *)target, image_stride, target_stride, width, height};
    const float inv_n = (float)(1.0 / (3.0 * (double)width * (double)height));
    if (ssim)
        hipLaunchKernelGGL(k_image_loss_backward<true>, grid, dim3(256), 0, ctx->stream, im, loss_window(), (const float *)workspace,
                           (const float *)upstream, lambda, inv_n, (float *)grad_image, grad_stride);
    else
        hipLaunchKernelGGL(k_image_loss_backward<false>, grid, dim3(256), 0, ctx->stream, im, loss_window(), (const float *)nullptr,
                           (const float *)upstream, lambda, inv_n, (float *)grad_image, grad_stride);
    LAUNCH_CHECK(ctx, "k_image_loss_backward");
    return SPLAT_OK;
}
