// points.hip — the reference app's own renderer: one opaque quad per point through a depth test.
//
// Reference: src/Renderer.ts:68-72 (computeTangent), :84-125 (the quad in the tangent plane of the SDF
// gradient, 0.025 * scale a side, two triangles), :128-143 (lit colour from the normal), :196-201 (depth24plus, "less"),
// :262-270 (clear colour, depth cleared to 1), drawn by src/main.ts:183-190.  The hardware pipeline becomes three steps:
//   - k_point_setup, one thread per point: the four clip-space corners in f32 in the vertex stage's order (the same
//     construction as disc.h's disc_record), then in f64 the screen corners, per triangle the three edge functions and
//     the depth plane, stored in f32 relative to an integer origin near the quad (so that a pixel's edge and depth values
//     lose nothing to the size of its screen coordinates); a ProjectedSplat whose bounds hold the quad, for the binner;
//     the lit colour; the point's own index (the binner's `sorted` array: index order);
//   - splat_bin_run's binner, unchanged: every tile's list in index order;
//   - k_point_resolve, one workgroup per 16 x 16 tile, PT_SLICES lanes per pixel: the tile's records are staged through
//     LDS in batches, every lane keeps the nearest (depth, index) of its share of them in registers, and the slices are
//     merged through LDS at the end.  "Nearest" is the total order (depth, then index): on equal depth the lower index
//     wins — what "less" does with draws in instance order — whatever order the records are visited in.  No atomics, and
//     the result does not depend on any scheduling.
//
// Conventions the reference leaves to the implementation, as fixed here: pixel centres at +0.5, the
// top-left fill rule (oracle.c: raster_tri), stored depth z/w (WebGPU keeps 0 <= z <= w), a fragment passes when
// 0 <= depth < the buffer's value.  There is no clipper: a quad with a corner at w <= 0 is dropped (orc_sequential's
// convention), and a point whose normal, scale or corners are not finite covers nothing.
//
// Compiled with contraction off (the Makefile's default rule): the corners are the same binary32 values as
// tests/point_raster.py computes.
#include "common.h"

#include <math.h>

constexpr uint32_t PT_TILE = 16;    // the reference's Renderer has no tile; 16 x 16 = one pixel per lane of a workgroup
constexpr uint32_t PT_BATCH = 256;  // records staged per round (one per thread)
constexpr uint32_t PT_REC_F4 = 7;   // float4s per raster record
// k_point_resolve's workgroup: PT_SLICES lanes per pixel, each slice walking every PT_SLICES-th record of the tile's list.
// A tile's records are visited one after another by its lanes, so the frame's longest list sets its time (the demo scene
// at 1080p: lists of up to ~2 800 records along the silhouette, mean ~480): four slices cut that chain four ways and give
// each SIMD four waves to interleave instead of one (measured: DESIGN.md §7).
constexpr uint32_t PT_SLICES = 4;
constexpr uint32_t PT_THREADS = PT_SLICES * PT_TILE * PT_TILE;

// Raster record (7 float4 = 112 bytes):
//   [0]    origin x, origin y (integers), top-left bits of the six edges (u32), -
//   [1..4] edges e0..e5 as (A, B, C) triples, packed: e(q) = A qx + B qy + C, q = pixel centre - origin; e0..e2 are the
//          first triangle's, e3..e5 the second's, each triangle oriented so that its inside is e >= 0
//   [5]    first triangle's depth plane: dz/dx, dz/dy, depth at the origin, -
//   [6]    second triangle's
// A triangle of zero area (or of a culled point) has edges (0, 0, -1): no pixel passes them.
struct PointVP {
    float m[16];
};

static constexpr size_t kPointBytes = 32 + PT_REC_F4 * 16 + 16 + 4; // ProjectedSplat, raster record, colour, index

// One triangle's edges (A, B, C) relative to the origin, its top-left bits and its depth plane.  Same
// orientation handling and fill rule as oracle.c's raster_tri (area from the vertex order; a negative
// area swaps the last two vertices).  Returns false for a triangle of zero area, which covers nothing.
__device__ static bool point_triangle(const double *X, const double *Y, const double *Z, int a, int b, int c, double ox, double oy,
                                      float *e, uint32_t &tl, float *zp) {
    double area = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a]);
    if (!(area != 0.0) || !isfinite(area)) {
        for (int k = 0; k < 3; ++k) { e[3 * k] = 0.0f; e[3 * k + 1] = 0.0f; e[3 * k + 2] = -1.0f; }
        zp[0] = zp[1] = zp[2] = 0.0f;
        tl = 0;
        return false;
    }
    if (area < 0.0) { const int t = b; b = c; c = t; area = -area; }
    const int v[3] = {a, b, c};
    tl = 0;
    for (int k = 0; k < 3; ++k) { // edge k runs from v[k+1] to v[k+2] (raster_tri's w0, w1, w2)
        const int p = v[(k + 1) % 3], q = v[(k + 2) % 3];
        const double dx = X[q] - X[p], dy = Y[q] - Y[p];
        // w = dx (py - Yp) - dy (px - Xp), with px = ox + qx, py = oy + qy
        e[3 * k] = (float)(-dy);
        e[3 * k + 1] = (float)dx;
        e[3 * k + 2] = (float)(dx * (oy - Y[p]) - dy * (ox - X[p]));
        if (dy < 0.0 || (dy == 0.0 && dx > 0.0)) tl |= 1u << k;
    }
    const double x1 = X[b] - X[a], y1 = Y[b] - Y[a], z1 = Z[b] - Z[a];
    const double x2 = X[c] - X[a], y2 = Y[c] - Y[a], z2 = Z[c] - Z[a];
    const double dzdx = (z1 * y2 - z2 * y1) / area, dzdy = (z2 * x1 - z1 * x2) / area;
    zp[0] = (float)dzdx;
    zp[1] = (float)dzdy;
    zp[2] = (float)(Z[a] + dzdx * (ox - X[a]) + dzdy * (oy - Y[a]));
    return true;
}

__global__ __launch_bounds__(256) void k_point_setup(PointVP vp, uint32_t width, uint32_t height, const float4 *__restrict__ positions,
                                                     uint32_t ps, const float4 *__restrict__ gradients, uint32_t gs,
                                                     const float *__restrict__ scales, uint32_t ss, uint32_t n, float4 *__restrict__ projected,
                                                     float4 *__restrict__ recs, float4 *__restrict__ colors, uint32_t *__restrict__ sorted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *m = vp.m;
    const float4 p = positions[(size_t)i * ps];
    const float4 g = gradients[(size_t)i * gs];
    const float sf = scales[(size_t)i * ss];
    // normal = normalize(gradient.yzw) (Renderer.ts:84-88): one reciprocal, three products
    const float gl = sqrtf((g.y * g.y + g.z * g.z) + g.w * g.w);
    const float ig = 1.0f / gl;
    const float nx = g.y * ig, ny = g.z * ig, nz = g.w * ig;
    // computeTangent (:68-72) and the bitangent (:91), as disc.h's disc_record
    const bool steep = fabsf(ny) > 0.9f;
    const float ux = steep ? 1.0f : 0.0f, uy = steep ? 0.0f : 1.0f, uz = 0.0f;
    float tx = uy * nz - uz * ny, ty = uz * nx - ux * nz, tz = ux * ny - uy * nx;
    const float itl = 1.0f / sqrtf((tx * tx + ty * ty) + tz * tz);
    tx *= itl; ty *= itl; tz *= itl;
    const float bx = ny * tz - nz * ty, by = nz * tx - nx * tz, bz = nx * ty - ny * tx;
    const float s = 0.025f * sf; // :101-103
    // corners in the order (-1,-1), (1,-1), (-1,1), (1,1); worldPos + (t ox s + b oy s) (:105-114), then VP * corner
    float cx[4], cy[4], cz[4], cw[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ox = (k & 1) ? 1.0f : -1.0f, oy = (k & 2) ? 1.0f : -1.0f;
        const float wx = p.x + ((tx * ox) * s + (bx * oy) * s);
        const float wy = p.y + ((ty * ox) * s + (by * oy) * s);
        const float wz = p.z + ((tz * ox) * s + (bz * oy) * s);
        cx[k] = ((m[0] * wx + m[4] * wy) + m[8] * wz) + m[12];
        cy[k] = ((m[1] * wx + m[5] * wy) + m[9] * wz) + m[13];
        cz[k] = ((m[2] * wx + m[6] * wy) + m[10] * wz) + m[14];
        cw[k] = ((m[3] * wx + m[7] * wy) + m[11] * wz) + m[15];
        ok = ok && cw[k] > 0.0f && isfinite(cx[k]) && isfinite(cy[k]) && isfinite(cz[k]) && isfinite(cw[k]);
    }
    float4 rec[PT_REC_F4];
    float4 bounds = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // bins nowhere (tile_range: min >= max)
    for (int k = 0; k < (int)PT_REC_F4; ++k) rec[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float e[18] = {0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1};
    float zp[6] = {0, 0, 0, 0, 0, 0};
    uint32_t tl0 = 0, tl1 = 0;
    if (ok) {
        double X[4], Y[4], Z[4];
        const double W = (double)width, H = (double)height;
        double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        for (int k = 0; k < 4; ++k) {
            const double w = (double)cw[k];
            X[k] = ((double)cx[k] / w + 1.0) * 0.5 * W;
            Y[k] = (1.0 - (double)cy[k] / w) * 0.5 * H;
            Z[k] = (double)cz[k] / w;
            x0 = fmin(x0, X[k]); x1 = fmax(x1, X[k]); y0 = fmin(y0, Y[k]); y1 = fmax(y1, Y[k]);
        }
        // origin: the box's corner clamped to the screen (the pixels evaluated are on it)
        const double ox = floor(fmin(fmax(x0, 0.0), W)), oy = floor(fmin(fmax(y0, 0.0), H));
        const bool t0 = point_triangle(X, Y, Z, 0, 1, 2, ox, oy, e, tl0, zp);         // (-1,-1), (1,-1), (-1,1)  (:99-102)
        const bool t1 = point_triangle(X, Y, Z, 2, 1, 3, ox, oy, e + 9, tl1, zp + 3); // (-1,1), (1,-1), (1,1)
        // the box, widened by 2^-6 px so that the rounding of its corners to f32 never loses a pixel centre
        const double pad = 1.0 / 64.0;
        if (t0 || t1) bounds = make_float4((float)(x0 - pad), (float)(y0 - pad), (float)(x1 + pad), (float)(y1 + pad));
        rec[0] = make_float4((float)ox, (float)oy, __uint_as_float(tl0 | (tl1 << 3)), 0.0f);
    }
    rec[1] = make_float4(e[0], e[1], e[2], e[3]);
    rec[2] = make_float4(e[4], e[5], e[6], e[7]);
    rec[3] = make_float4(e[8], e[9], e[10], e[11]);
    rec[4] = make_float4(e[12], e[13], e[14], e[15]);
    rec[5] = make_float4(e[16], e[17], zp[0], zp[1]);
    rec[6] = make_float4(zp[2], zp[3], zp[4], zp[5]);
    for (int k = 0; k < (int)PT_REC_F4; ++k) recs[(size_t)i * PT_REC_F4 + k] = rec[k];
    projected[(size_t)i * 2] = bounds;
    projected[(size_t)i * 2 + 1] = make_float4(0.0f, 0.0f, __uint_as_float(i), 0.0f); // (depth, radius unused; originalIndex)
    // colour (:121-124, :128-143): c = n * 0.5 + 0.5, lit = c * (0.3 + 0.7 max(dot(n, normalize(1,1,1)), 0)), alpha 1
    const float l = 1.0f / sqrtf(3.0f);
    const float kd = 0.3f + 0.7f * fmaxf((nx * l + ny * l) + nz * l, 0.0f);
    colors[i] = make_float4((nx * 0.5f + 0.5f) * kd, (ny * 0.5f + 0.5f) * kd, (nz * 0.5f + 0.5f) * kd, 1.0f);
    sorted[i] = i;
}

// orc_unorm8: clamp to [0, 1] (NaN -> 0), then v * 255 + 0.5 truncated
__device__ __forceinline__ uint32_t point_unorm8(float v) {
    if (!(v > 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    return (uint32_t)(v * 255.0f + 0.5f);
}

__device__ __forceinline__ bool point_inside(float qx, float qy, const float *e, uint32_t tl) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float w = fmaf(e[3 * k], qx, fmaf(e[3 * k + 1], qy, e[3 * k + 2]));
        in = in && (w > 0.0f || (w == 0.0f && ((tl >> k) & 1u)));
    }
    return in;
}

// (depth, index) nearer in the depth test's sense: smaller depth, and on equal depth the lower index (the earlier draw,
// which "less" keeps).  A total order, so the nearest fragment does not depend on the order records are visited in.
__device__ __forceinline__ bool point_nearer(float z, uint32_t i, float bz, uint32_t bi) { return z < bz || (z == bz && i < bi); }

__global__ __launch_bounds__(PT_THREADS) void k_point_resolve(const float4 *__restrict__ recs, const float4 *__restrict__ colors,
                                                              const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ indices, uint32_t ntx, uint32_t width,
                                                              uint32_t height, uint8_t *__restrict__ out8, float4 *__restrict__ out32,
                                                              float *__restrict__ out_depth, uint32_t *__restrict__ out_ids) {
    __shared__ float4 s_rec[PT_REC_F4][PT_BATCH];
    __shared__ uint32_t s_idx[PT_BATCH];
    __shared__ float s_best[PT_SLICES][PT_TILE * PT_TILE];
    __shared__ uint32_t s_best_i[PT_SLICES][PT_TILE * PT_TILE];
    const uint32_t tid = threadIdx.x, pix = tid & 255u, slice = tid >> 8;
    const uint32_t tile = blockIdx.y * ntx + blockIdx.x;
    const uint32_t count = counts[tile], off = offsets[tile];
    const uint32_t x = blockIdx.x * PT_TILE + (pix & 15u), y = blockIdx.y * PT_TILE + (pix >> 4);
    const float xf = (float)x, yf = (float)y;
    float best = 1.0f; // the cleared depth: a fragment must be nearer ("less")
    uint32_t best_i = 0xffffffffu;
    for (uint32_t base = 0; base < count; base += PT_BATCH) {
        __syncthreads(); // the previous batch has been read by every lane
        if (tid < PT_BATCH && base + tid < count) {
            const uint32_t idx = indices[off + base + tid];
            s_idx[tid] = idx;
#pragma unroll
            for (uint32_t k = 0; k < PT_REC_F4; ++k) s_rec[k][tid] = recs[(size_t)idx * PT_REC_F4 + k];
        }
        __syncthreads();
        const uint32_t m = min(PT_BATCH, count - base);
        // slice s of the workgroup's PT_SLICES x 256 lanes takes records s, s + PT_SLICES, ... of the batch for its pixel
        for (uint32_t j = slice; j < m; j += PT_SLICES) {
            const float4 r0 = s_rec[0][j];
            const float4 r1 = s_rec[1][j], r2 = s_rec[2][j], r3 = s_rec[3][j], r4 = s_rec[4][j], r5 = s_rec[5][j], r6 = s_rec[6][j];
            const float e[18] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x, r5.y};
            const uint32_t tl = __float_as_uint(r0.z);
            const float qx = (xf - r0.x) + 0.5f, qy = (yf - r0.y) + 0.5f; // exact: integers below 2^24, then + 0.5
            const uint32_t idx = s_idx[j];
            if (point_inside(qx, qy, e, tl)) {
                const float z = fmaf(r5.z, qx, fmaf(r5.w, qy, r6.x));
                if (z >= 0.0f && point_nearer(z, idx, best, best_i)) { best = z; best_i = idx; }
            }
            if (point_inside(qx, qy, e + 9, tl >> 3)) {
                const float z = fmaf(r6.y, qx, fmaf(r6.z, qy, r6.w));
                if (z >= 0.0f && point_nearer(z, idx, best, best_i)) { best = z; best_i = idx; }
            }
        }
    }
    // the slices' nearest fragments of each pixel, merged in the same order
    s_best[slice][pix] = best;
    s_best_i[slice][pix] = best_i;
    __syncthreads();
    if (slice != 0) return;
    for (uint32_t s = 1; s < PT_SLICES; ++s)
        if (point_nearer(s_best[s][pix], s_best_i[s][pix], best, best_i)) { best = s_best[s][pix]; best_i = s_best_i[s][pix]; }
    if (x >= width || y >= height) return;
    const size_t o = (size_t)y * width + x;
    const float4 c = best_i != 0xffffffffu ? colors[best_i] : make_float4(0.05f, 0.05f, 0.1f, 1.0f); // Renderer.ts:267
    if (out8)
        ((uint32_t *)out8)[o] = point_unorm8(c.x) | (point_unorm8(c.y) << 8) | (point_unorm8(c.z) << 16) | (point_unorm8(c.w) << 24);
    if (out32) out32[o] = c;
    if (out_depth) out_depth[o] = best;
    if (out_ids) out_ids[o] = best_i;
}

extern "C" int splat_point_frame(splat_ctx *ctx, splat_binner *binner, const float *uniforms, const void *positions,
                                 uint32_t pos_stride_vec4, const void *gradients, uint32_t grad_stride_vec4, const void *scales,
                                 uint32_t scale_stride_f32, uint32_t n, uint32_t width, uint32_t height, void *out_rgba8,
                                 void *out_rgba32f, void *out_depth_f32, void *out_ids) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, binner != nullptr && binner->ctx == ctx && uniforms != nullptr);
    ARG_CHECK(ctx, binner->tile == PT_TILE);
    ARG_CHECK(ctx, n == 0 || (positions && gradients && scales));
    ARG_CHECK(ctx, pos_stride_vec4 >= 1 && grad_stride_vec4 >= 1 && scale_stride_f32 >= 1);
    ARG_CHECK(ctx, width >= 1 && height >= 1);
    const uint32_t ntx = div_up(width, PT_TILE), nty = div_up(height, PT_TILE);
    ARG_CHECK(ctx, ntx <= 65535 && nty <= 65535 && (uint64_t)ntx * nty <= (1u << 24)); // (the binner's limits)
    splat_binner *b = binner;
    if (n > b->points_cap) { // (with a quarter's headroom, unless that overflows)
        const uint32_t grown = n + n / 4 > n ? n + n / 4 : n;
        const int rc = device_reserve(ctx, &b->points, &b->points_cap, grown, (size_t)grown * kPointBytes, "point frame hipMalloc");
        if (rc != SPLAT_OK) return rc;
    }
    const size_t cap = b->points_cap;
    float4 *projected = (float4 *)b->points;
    float4 *recs = projected + cap * 2;
    float4 *colors = recs + cap * PT_REC_F4;
    uint32_t *sorted = (uint32_t *)(colors + cap);
    if (n > 0) {
        PointVP vp;
        for (int k = 0; k < 16; ++k) vp.m[k] = uniforms[k];
        hipLaunchKernelGGL(k_point_setup, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, vp, width, height, (const float4 *)positions,
                           pos_stride_vec4, (const float4 *)gradients, grad_stride_vec4, (const float *)scales, scale_stride_f32, n,
                           projected, recs, colors, sorted);
        LAUNCH_CHECK(ctx, "k_point_setup");
    }
    // bin in index order; the frame reads its pair total back (one host round trip) instead of running sync-free, so its
    // lists are complete when the resolve runs and there is never a frame to render again
    const bool allow_async = b->allow_async;
    b->allow_async = false;
    BinRunArgs run;
    run.projected = projected, run.n_splats = n, run.sorted = sorted, run.n_sorted = n, run.width = width, run.height = height;
    int rc = binner_run(b, run);
    b->allow_async = allow_async;
    if (rc != SPLAT_OK) return rc;
    const uint32_t *indices = b->pairs.result_in_primary ? b->pairs.payload : b->pairs.payload_b;
    hipLaunchKernelGGL(k_point_resolve, dim3(ntx, nty), dim3(PT_THREADS), 0, ctx->stream, recs, colors, b->counts, b->offsets, indices, ntx,
                       width, height, (uint8_t *)out_rgba8, (float4 *)out_rgba32f, (float *)out_depth_f32, (uint32_t *)out_ids);
    LAUNCH_CHECK(ctx, "k_point_resolve");
    return SPLAT_OK;
}
