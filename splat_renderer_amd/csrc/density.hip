// density.hip — what a 3D Gaussian splatting fit needs beside the frame, its loss and their gradients (an extension, no
// reference counterpart): the optimiser step and adaptive density control (include/splat.h, "Density control and optimiser",
// states the rules).
//
// k_adam<MASKED, VEC>     one Adam update of one parameter plane of rows x floats_per_row floats.  VEC: one float4 of the
//                         flattened plane per thread (all four planes 16-byte aligned; the up to three floats past the last
//                         whole float4 take the scalar form in the same launch); else one float per thread.  MASKED: a row
//                         whose visibility byte is 0 is left alone: a thread none of whose floats is visible loads nothing but
//                         the mask, and a float4 that straddles a visible and an invisible row stores the invisible floats back
//                         with the bits it loaded (one thread owns a float4: no race).  Every element goes through adam_one(),
//                         whose roundings are written out (explicit fmaf, no contraction), so the four instantiations give one
//                         element the same bits.
// k_density_accumulate    one thread per splat: visibility of the record's 3-sigma box, the three running statistics, the mask.
//                         <PLANE2>: the gradient read from an n x 2 plane (splat_density_accumulate_abs) instead of columns 0, 1
//                         of the n x 8 plane; everything else the same code.  <SURFEL>: the visibility and the radius from
//                         disc_bounds() of the record itself (splat_density_accumulate_surfel: a surfel's B10 and q are not 0).
// k_densify_classify ..   splat_densify_plan: classify -> scan(alive), scan(wants) -> grant under the cap -> scan(rows per
// k_densify_fill          splat), scan(granted clones) -> one thread per splat writes its rows.  The scans are scan.hip's.
// k_densify_geometry      one thread per OUTPUT row: means and log-scales, the split children drawn with Philox4x32-10 (philox.h).
// k_densify_classify and k_densify_geometry are templates on NS, the log-scales per row: 3 for an ellipsoid, 2 for a 2D Gaussian
// surfel (the _surfel entry points), whose split children stay in its plane: 2DGS's stds = (sx, sy, 0).
// k_densify_rows<VEC>     one thread per float (float4) of the OUTPUT plane: a gather, contiguous writes.
// No atomics anywhere: the same inputs give the same bits.
//
// Roofline: all of them are HBM streams.  Adam moves 28 B per parameter (p, g, m, v read; p, m, v written): 8.3 GB for 5 M splats
// with SH of degree 3, 1.6 ms at the 5.1 TB/s copy rate ("Density control and optimiser";
// tools/grad_bench.py --optimizer measures the step against that floor).
#include "common.h"
#include "disc.h"
#include "philox.h"

namespace {

constexpr uint32_t DT = 256; // threads per workgroup, every kernel here

struct AdamArgs {
    float *p, *m, *v;
    const float *g;
    const uint8_t *vis;
    uint32_t total, fpr, head; // floats in the plane, per row, of a row's head
    float step_head, step_tail, b1, omb1, b2, omb2, isbc2, eps;
};

__device__ __forceinline__ void adam_one(const AdamArgs &a, float step, float g, float &p, float &m, float &v) {
#pragma clang fp contract(off)
    m = fmaf(a.b1, m, a.omb1 * g);
    v = fmaf(a.b2, v, (a.omb2 * g) * g);
    const float d = fmaf(sqrtf(v), a.isbc2, a.eps);
    p = fmaf(-step, m / d, p);
}

template <bool MASKED, bool VEC>
__global__ __launch_bounds__(DT) void k_adam(AdamArgs a) {
    const uint32_t t = blockIdx.x * DT + threadIdx.x;
    const bool one_rate = a.head >= a.fpr;
    if constexpr (VEC) {
        const uint32_t units = a.total >> 2;
        if (t < units) {
            const uint32_t e0 = t << 2;
            uint32_t row = 0, col = e0;
            if (MASKED || !one_rate) {
                row = e0 / a.fpr;
                col = e0 - row * a.fpr;
            }
            float st[4];
            bool on[4];
            bool any = !MASKED;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                st[j] = (one_rate || col < a.head) ? a.step_head : a.step_tail;
                on[j] = true;
                if constexpr (MASKED) {
                    on[j] = a.vis[row] != 0;
                    any |= on[j];
                }
                if (++col == a.fpr) {
                    col = 0;
                    ++row;
                }
            }
            if (!any) return;
            float4 p = reinterpret_cast<float4 *>(a.p)[t], m = reinterpret_cast<float4 *>(a.m)[t], v = reinterpret_cast<float4 *>(a.v)[t];
            const float4 g = reinterpret_cast<const float4 *>(a.g)[t];
            if (on[0]) adam_one(a, st[0], g.x, p.x, m.x, v.x);
            if (on[1]) adam_one(a, st[1], g.y, p.y, m.y, v.y);
            if (on[2]) adam_one(a, st[2], g.z, p.z, m.z, v.z);
            if (on[3]) adam_one(a, st[3], g.w, p.w, m.w, v.w);
            reinterpret_cast<float4 *>(a.p)[t] = p;
            reinterpret_cast<float4 *>(a.m)[t] = m;
            reinterpret_cast<float4 *>(a.v)[t] = v;
            return;
        }
    }
    // one float: the whole plane (scalar form), or the floats past the last whole float4
    uint32_t e;
    if constexpr (VEC) {
        e = (a.total & ~3u) + (t - (a.total >> 2));
    } else {
        e = t;
    }
    if (e >= a.total) return;
    uint32_t row = 0, col = e;
    if (MASKED || !one_rate) {
        row = e / a.fpr;
        col = e - row * a.fpr;
    }
    if constexpr (MASKED) {
        if (a.vis[row] == 0) return;
    }
    float p = a.p[e], m = a.m[e], v = a.v[e];
    adam_one(a, (one_rate || col < a.head) ? a.step_head : a.step_tail, a.g[e], p, m, v);
    a.p[e] = p;
    a.m[e] = m;
    a.v[e] = v;
}

// The visibility rule in binary32, one rounding per operation in the order written (tests/density_ref.py restates it bit for
// bit); hx, hy are disc_bounds()'s half-widths of a record with q = 0 and B10 = 0.
__device__ __forceinline__ bool density_visible(float4 ra, float4 rb, float w, float h, float &radius) {
#pragma clang fp contract(off)
    const bool culled = ra.x == 0.0f && ra.y == 0.0f && ra.z == 0.0f && ra.w == 0.0f && rb.x == 0.0f && rb.y == 0.0f && rb.z == 0.0f &&
                        rb.w == 0.0f;
    const float b00 = ra.z, b01 = ra.w, b11 = rb.y;
    const float hx = sqrtf(b01 * b01 + b11 * b11) / (b00 * b11), hy = 1.0f / b11;
    radius = fmaxf(hx, hy);
    return !culled && ra.x + hx > 0.0f && ra.x - hx < w && ra.y + hy > 0.0f && ra.y - hy < h; // (false for a NaN)
}

// A surfel record's own rule: disc_bounds() (disc.h; binary32, bit for bit the box splat_project_surfel wrote to `projected`),
// visible when the box overlaps the screen, radius half its larger side: projected[i].screenRadius.
__device__ __forceinline__ bool density_visible_surfel(float4 ra, float4 rb, float w, float h, float &radius) {
#pragma clang fp contract(off)
    const DiscRecord rec = {ra, rb};
    float4 b;
    const bool ok = disc_bounds(rec, b);
    radius = 0.5f * fmaxf(b.z - b.x, b.w - b.y);
    return ok && b.z > 0.0f && b.x < w && b.w > 0.0f && b.y < h;
}

template <bool PLANE2, bool SURFEL>
__global__ __launch_bounds__(DT) void k_density_accumulate(const float4 *__restrict__ rec, const void *__restrict__ grad, uint32_t n, float w,
                                                           float h, float *__restrict__ grad_accum, float *__restrict__ denom,
                                                           float *__restrict__ max_radius, uint8_t *__restrict__ vis) {
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    const float4 ra = rec[2 * (size_t)i], rb = rec[2 * (size_t)i + 1];
    float radius;
    bool on;
    if constexpr (SURFEL) on = density_visible_surfel(ra, rb, w, h, radius);
    else on = density_visible(ra, rb, w, h, radius);
    vis[i] = on ? 1 : 0;
    if (!on) return;
    float gx, gy;
    if constexpr (PLANE2) {
        const float2 g = static_cast<const float2 *>(grad)[i];
        gx = g.x;
        gy = g.y;
    } else {
        const float4 g = static_cast<const float4 *>(grad)[2 * (size_t)i];
        gx = g.x;
        gy = g.y;
    }
    grad_accum[i] += hypotf(gx * (0.5f * w), gy * (0.5f * h));
    denom[i] += 1.0f;
    max_radius[i] = fmaxf(max_radius[i], radius);
}

enum : uint32_t { CLS_DEAD = 0, CLS_KEPT = 1, CLS_CLONE = 2, CLS_SPLIT = 3 };
constexpr uint32_t ROW_PARENT_MASK = 0x3fffffffu;

template <int NS>
__global__ __launch_bounds__(DT) void k_densify_classify(const float *__restrict__ log_scales, const float *__restrict__ logits,
                                                         const float *__restrict__ grad_accum, const float *__restrict__ denom,
                                                         const float *__restrict__ max_radius, uint32_t n, splat_densify_cfg cfg,
                                                         uint32_t *__restrict__ cls, uint32_t *__restrict__ alive, uint32_t *__restrict__ wants) {
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    const float l0 = log_scales[NS * (size_t)i], l1 = log_scales[NS * (size_t)i + 1];
    float lmax = fmaxf(l0, l1);
    bool nan = l0 != l0 || l1 != l1;
    if constexpr (NS == 3) {
        const float l2 = log_scales[NS * (size_t)i + 2];
        lmax = fmaxf(lmax, l2);
        nan = nan || l2 != l2;
    }
    if (nan) lmax = __builtin_nanf(""); // (fmaxf drops a NaN; the rule's max keeps it)
    const float s = expf(lmax), o = 1.0f / (1.0f + expf(-logits[i])), r = max_radius[i];
    const float d = denom[i], g = d > 0.0f ? grad_accum[i] / d : 0.0f;
    const bool dead = !(o >= cfg.min_opacity) || (cfg.max_screen_radius > 0.0f && r > cfg.max_screen_radius) ||
                      (cfg.max_world_scale > 0.0f && !(s <= cfg.max_world_scale));
    const bool more = !dead && g >= cfg.grad_threshold;
    cls[i] = dead ? CLS_DEAD : !more ? CLS_KEPT : s > cfg.scale_threshold ? CLS_SPLIT : CLS_CLONE;
    alive[i] = dead ? 0u : 1u;
    wants[i] = more ? 1u : 0u;
}

// tot[0] = survivors, before[i] = the splats of lower index that want more: extras are granted in index order while
// survivors + extras granted so far < max_splats (a refused splat is kept as it is)
__global__ __launch_bounds__(DT) void k_densify_grant(uint32_t *__restrict__ cls, const uint32_t *__restrict__ before, const uint32_t *__restrict__ tot,
                                                      uint32_t n, uint32_t max_splats, uint32_t *__restrict__ count, uint32_t *__restrict__ clones) {
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    uint32_t c = cls[i];
    if (c >= CLS_CLONE && max_splats != 0u && !((uint64_t)tot[0] + before[i] < (uint64_t)max_splats)) cls[i] = c = CLS_KEPT;
    count[i] = c == CLS_DEAD ? 0u : c == CLS_KEPT ? 1u : 2u;
    clones[i] = c == CLS_CLONE ? 1u : 0u;
}

__global__ __launch_bounds__(DT) void k_densify_fill(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ offset, uint32_t n,
                                                     uint32_t *__restrict__ rows) {
    const uint32_t i = blockIdx.x * DT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cls[i], o = offset[i];
    if (c == CLS_KEPT) {
        rows[o] = i;
    } else if (c == CLS_CLONE) {
        rows[o] = i;
        rows[o + 1] = i | (1u << 30);
    } else if (c == CLS_SPLIT) {
        rows[o] = i | (2u << 30);
        rows[o + 1] = i | (3u << 30);
    }
}

constexpr double LOG_SPLIT_SHRINK = 0.47000362924573555; // log 1.6

template <int NS>
__global__ __launch_bounds__(DT) void k_densify_geometry(const uint32_t *__restrict__ rows, uint32_t n_out, const float *__restrict__ means,
                                                         const float *__restrict__ log_scales, const float4 *__restrict__ rotations, uint2 key,
                                                         float *__restrict__ means_out, float *__restrict__ log_scales_out) {
    const uint32_t r = blockIdx.x * DT + threadIdx.x;
    if (r >= n_out) return;
    const uint32_t code = rows[r], parent = code & ROW_PARENT_MASK, kind = code >> 30;
    const size_t src = 3 * (size_t)parent, dst = 3 * (size_t)r, lsrc = NS * (size_t)parent, ldst = NS * (size_t)r;
    float px = means[src], py = means[src + 1], pz = means[src + 2];
    float lx = log_scales[lsrc], ly = log_scales[lsrc + 1], lz = 0.0f;
    if constexpr (NS == 3) lz = log_scales[lsrc + 2];
    if (kind >= 2u) {
        const uint4 x = philox4x32_10(make_uint4(parent, kind - 2u, 0u, 0u), key);
        const float3 xi = philox_normals3(x);
        const float ex = expf(lx) * xi.x, ey = expf(ly) * xi.y, ez = NS == 3 ? expf(lz) * xi.z : 0.0f;
        const float4 q = rotations[parent]; // (w, x, y, z), normalised as ellipsoid_record() does
        const float k = 1.0f / sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
        const float qr = q.x * k, qx = q.y * k, qy = q.z * k, qz = q.w * k;
        const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r01 = 2.0f * (qx * qy - qr * qz), r02 = 2.0f * (qx * qz + qr * qy);
        const float r10 = 2.0f * (qx * qy + qr * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r12 = 2.0f * (qy * qz - qr * qx);
        const float r20 = 2.0f * (qx * qz - qr * qy), r21 = 2.0f * (qy * qz + qr * qx), r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
        if constexpr (NS == 3) {
            px += (r00 * ex + r01 * ey) + r02 * ez;
            py += (r10 * ex + r11 * ey) + r12 * ez;
            pz += (r20 * ex + r21 * ey) + r22 * ez;
        } else { // a surfel: the tangent axes only (csrc/surfel.h's R[:,0], R[:,1]); the third normal is not used
            px += r00 * ex + r01 * ey;
            py += r10 * ex + r11 * ey;
            pz += r20 * ex + r21 * ey;
        }
        lx = (float)((double)lx - LOG_SPLIT_SHRINK); // (in float64: rounded once, also where log sigma is near log 1.6)
        ly = (float)((double)ly - LOG_SPLIT_SHRINK);
        lz = (float)((double)lz - LOG_SPLIT_SHRINK);
    }
    means_out[dst] = px; means_out[dst + 1] = py; means_out[dst + 2] = pz;
    log_scales_out[ldst] = lx; log_scales_out[ldst + 1] = ly;
    if constexpr (NS == 3) log_scales_out[ldst + 2] = lz;
}

// `per` = floats (VEC: float4s) per row
template <bool VEC>
__global__ __launch_bounds__(DT) void k_densify_rows(const uint32_t *__restrict__ rows, uint32_t total, uint32_t per, const void *__restrict__ in,
                                                     void *__restrict__ out, bool zero_new) {
    const uint32_t e = blockIdx.x * DT + threadIdx.x;
    if (e >= total) return;
    const uint32_t r = e / per, c = e - r * per;
    const uint32_t code = rows[r];
    const bool zero = zero_new && (code >> 30) != 0u;
    const size_t src = (size_t)(code & ROW_PARENT_MASK) * per + c;
    if constexpr (VEC) {
        static_cast<float4 *>(out)[e] = zero ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : static_cast<const float4 *>(in)[src];
    } else {
        static_cast<float *>(out)[e] = zero ? 0.0f : static_cast<const float *>(in)[src];
    }
}

constexpr uint32_t DENSIFY_MAX_SPLATS = 1u << 30;
constexpr uint64_t DENSITY_MAX_FLOATS = 0xffffffffull - DT; // one thread per float at most, and div_up() adds DT - 1 in 32 bits
size_t plan_plane_bytes(uint32_t n) { return ((size_t)n * 4 + 255) & ~(size_t)255; }

} // namespace

extern "C" int splat_adam_step(splat_ctx *ctx, void *param, const void *grad, void *m, void *v, uint32_t rows, uint32_t floats_per_row,
                               uint32_t head_floats, double step_head, double step_tail, double beta1, double beta2, double inv_sqrt_bc2,
                               double eps, const void *visible_u8) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    if (rows == 0) return SPLAT_OK;
    ARG_CHECK(ctx, param && grad && m && v && floats_per_row >= 1 && head_floats <= floats_per_row);
    ARG_CHECK(ctx, (uint64_t)rows * floats_per_row <= DENSITY_MAX_FLOATS);
    ARG_CHECK(ctx, (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 3) == 0);
    ARG_CHECK(ctx, beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0); // (false for a NaN)
    AdamArgs a;
    a.p = (float *)param; a.m = (float *)m; a.v = (float *)v; a.g = (const float *)grad; a.vis = (const uint8_t *)visible_u8;
    a.total = rows * floats_per_row; a.fpr = floats_per_row; a.head = head_floats;
    a.step_head = (float)step_head; a.step_tail = (float)step_tail;
    a.b1 = (float)beta1; a.omb1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.omb2 = (float)(1.0 - beta2);
    a.isbc2 = (float)inv_sqrt_bc2; a.eps = (float)eps;
    const bool vec = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && a.total >= 4;
    const uint32_t threads = vec ? (a.total >> 2) + (a.total & 3u) : a.total;
    const dim3 grid(div_up(threads, DT));
    if (vec && a.vis) hipLaunchKernelGGL((k_adam<true, true>), grid, dim3(DT), 0, ctx->stream, a);
    else if (vec) hipLaunchKernelGGL((k_adam<false, true>), grid, dim3(DT), 0, ctx->stream, a);
    else if (a.vis) hipLaunchKernelGGL((k_adam<true, false>), grid, dim3(DT), 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_adam<false, false>), grid, dim3(DT), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx, "k_adam");
    return SPLAT_OK;
}

// splat_density_accumulate (grad: the n x 8 plane, 16-byte aligned) and splat_density_accumulate_abs (plane2: the n x 2 plane,
// 8-byte aligned): one kernel, the gradient's layout its template argument
static int density_accumulate(splat_ctx *ctx, const void *records, const void *grad, bool plane2, bool surfel, uint32_t n, uint32_t width, uint32_t height,
                              void *grad_accum, void *denom, void *max_radius, void *visible_u8) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    if (n == 0) return SPLAT_OK;
    ARG_CHECK(ctx, records && grad && grad_accum && denom && max_radius && visible_u8 && width >= 1 && height >= 1);
    ARG_CHECK(ctx, ((uintptr_t)records & 15) == 0 && ((uintptr_t)grad & (plane2 ? 7 : 15)) == 0);
    ARG_CHECK(ctx, (((uintptr_t)grad_accum | (uintptr_t)denom | (uintptr_t)max_radius) & 3) == 0);
    if (surfel)
        hipLaunchKernelGGL((k_density_accumulate<false, true>), dim3(div_up(n, DT)), dim3(DT), 0, ctx->stream, (const float4 *)records, grad, n,
                           (float)width, (float)height, (float *)grad_accum, (float *)denom, (float *)max_radius, (uint8_t *)visible_u8);
    else if (plane2)
        hipLaunchKernelGGL((k_density_accumulate<true, false>), dim3(div_up(n, DT)), dim3(DT), 0, ctx->stream, (const float4 *)records, grad, n, (float)width,
                           (float)height, (float *)grad_accum, (float *)denom, (float *)max_radius, (uint8_t *)visible_u8);
    else
        hipLaunchKernelGGL((k_density_accumulate<false, false>), dim3(div_up(n, DT)), dim3(DT), 0, ctx->stream, (const float4 *)records, grad, n, (float)width,
                           (float)height, (float *)grad_accum, (float *)denom, (float *)max_radius, (uint8_t *)visible_u8);
    LAUNCH_CHECK(ctx, "k_density_accumulate");
    return SPLAT_OK;
}

extern "C" int splat_density_accumulate(splat_ctx *ctx, const void *records, const void *grad_records, uint32_t n, uint32_t width,
                                        uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8) {
    return density_accumulate(ctx, records, grad_records, false, false, n, width, height, grad_accum, denom, max_radius, visible_u8);
}

extern "C" int splat_density_accumulate_abs(splat_ctx *ctx, const void *records, const void *grad_center_abs, uint32_t n, uint32_t width,
                                            uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8) {
    return density_accumulate(ctx, records, grad_center_abs, true, false, n, width, height, grad_accum, denom, max_radius, visible_u8);
}

extern "C" int splat_density_accumulate_surfel(splat_ctx *ctx, const void *records, const void *grad_records, uint32_t n, uint32_t width,
                                               uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8) {
    if (n >= DENSIFY_MAX_SPLATS) return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_density_accumulate_surfel: n must be below 2^30");
    return density_accumulate(ctx, records, grad_records, false, true, n, width, height, grad_accum, denom, max_radius, visible_u8);
}

extern "C" uint64_t splat_densify_plan_workspace_bytes(uint32_t n) { return 4 * (uint64_t)plan_plane_bytes(n) + 256; }

// splat_densify_plan (ns = 3) and splat_densify_plan_surfel (ns = 2): one plan, the log-scales per row the classify kernel's
// template argument
static int densify_plan(splat_ctx *ctx, int ns, const void *log_scales, const void *opacity_logits, const void *grad_accum, const void *denom,
                        const void *max_radius, uint32_t n, const splat_densify_cfg *cfg, void *workspace, uint64_t workspace_bytes, void *rows,
                        uint32_t *n_out_host, uint32_t *counts4_host) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, cfg && n_out_host && counts4_host);
    if (n >= DENSIFY_MAX_SPLATS) return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_densify_plan: n must be below 2^30 (a row keeps its parent in 30 bits)");
    *n_out_host = 0;
    counts4_host[0] = counts4_host[1] = counts4_host[2] = counts4_host[3] = 0;
    if (n == 0) return SPLAT_OK;
    ARG_CHECK(ctx, log_scales && opacity_logits && grad_accum && denom && max_radius && rows && workspace);
    ARG_CHECK(ctx, (((uintptr_t)log_scales | (uintptr_t)opacity_logits | (uintptr_t)grad_accum | (uintptr_t)denom | (uintptr_t)max_radius |
                     (uintptr_t)rows) & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
    if (workspace_bytes < splat_densify_plan_workspace_bytes(n))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_densify_plan: the workspace is smaller than splat_densify_plan_workspace_bytes(n)");
    const size_t plane = plan_plane_bytes(n);
    char *w = (char *)workspace;
    uint32_t *cls = (uint32_t *)w, *a = (uint32_t *)(w + plane), *b = (uint32_t *)(w + 2 * plane), *c = (uint32_t *)(w + 3 * plane);
    uint32_t *tot = (uint32_t *)(w + 4 * plane); // {survivors, splats that want more, output rows, clones}
    int rc = ctx_ensure_pinned(ctx, 4 * sizeof(uint32_t));
    if (rc != SPLAT_OK) return rc;
    const dim3 grid(div_up(n, DT)), block(DT);
    if (ns == 2)
        hipLaunchKernelGGL(k_densify_classify<2>, grid, block, 0, ctx->stream, (const float *)log_scales, (const float *)opacity_logits,
                           (const float *)grad_accum, (const float *)denom, (const float *)max_radius, n, *cfg, cls, a, c);
    else
        hipLaunchKernelGGL(k_densify_classify<3>, grid, block, 0, ctx->stream, (const float *)log_scales, (const float *)opacity_logits,
                           (const float *)grad_accum, (const float *)denom, (const float *)max_radius, n, *cfg, cls, a, c);
    LAUNCH_CHECK(ctx, "k_densify_classify");
    if ((rc = scan_exclusive_u32(ctx, a, a, n, tot + 0)) != SPLAT_OK) return rc;
    if ((rc = scan_exclusive_u32(ctx, c, b, n, tot + 1)) != SPLAT_OK) return rc;
    hipLaunchKernelGGL(k_densify_grant, grid, block, 0, ctx->stream, cls, b, tot, n, cfg->max_splats, a, c);
    LAUNCH_CHECK(ctx, "k_densify_grant");
    if ((rc = scan_exclusive_u32(ctx, a, b, n, tot + 2)) != SPLAT_OK) return rc;
    if ((rc = scan_exclusive_u32(ctx, c, c, n, tot + 3)) != SPLAT_OK) return rc;
    hipLaunchKernelGGL(k_densify_fill, grid, block, 0, ctx->stream, cls, b, n, (uint32_t *)rows);
    LAUNCH_CHECK(ctx, "k_densify_fill");
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, tot, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t *t = (const uint32_t *)ctx->pinned;
    const uint32_t survivors = t[0], out = t[2], clones = t[3], splits = out - survivors - clones;
    *n_out_host = out;
    counts4_host[0] = n - survivors;
    counts4_host[1] = survivors - clones - splits;
    counts4_host[2] = clones;
    counts4_host[3] = splits;
    return SPLAT_OK;
}

extern "C" int splat_densify_plan(splat_ctx *ctx, const void *log_scales, const void *opacity_logits, const void *grad_accum, const void *denom,
                                  const void *max_radius, uint32_t n, const splat_densify_cfg *cfg, void *workspace, uint64_t workspace_bytes,
                                  void *rows, uint32_t *n_out_host, uint32_t *counts4_host) {
    return densify_plan(ctx, 3, log_scales, opacity_logits, grad_accum, denom, max_radius, n, cfg, workspace, workspace_bytes, rows, n_out_host,
                        counts4_host);
}

extern "C" int splat_densify_plan_surfel(splat_ctx *ctx, const void *log_scales, const void *opacity_logits, const void *grad_accum,
                                         const void *denom, const void *max_radius, uint32_t n, const splat_densify_cfg *cfg, void *workspace,
                                         uint64_t workspace_bytes, void *rows, uint32_t *n_out_host, uint32_t *counts4_host) {
    return densify_plan(ctx, 2, log_scales, opacity_logits, grad_accum, denom, max_radius, n, cfg, workspace, workspace_bytes, rows, n_out_host,
                        counts4_host);
}

static int densify_geometry(splat_ctx *ctx, int ns, const void *rows, uint32_t n_out, const void *means, const void *log_scales,
                            const void *rotations, const splat_densify_cfg *cfg, void *means_out, void *log_scales_out) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, cfg);
    if (n_out == 0) return SPLAT_OK;
    ARG_CHECK(ctx, rows && means && log_scales && rotations && means_out && log_scales_out && n_out <= 0x7fffffffu);
    ARG_CHECK(ctx, (((uintptr_t)rows | (uintptr_t)means | (uintptr_t)log_scales | (uintptr_t)means_out | (uintptr_t)log_scales_out) & 3) == 0 &&
                       ((uintptr_t)rotations & 15) == 0);
    ARG_CHECK(ctx, means_out != means && log_scales_out != log_scales);
    const uint2 key = make_uint2((uint32_t)cfg->seed, (uint32_t)(cfg->seed >> 32));
    if (ns == 2)
        hipLaunchKernelGGL(k_densify_geometry<2>, dim3(div_up(n_out, DT)), dim3(DT), 0, ctx->stream, (const uint32_t *)rows, n_out,
                           (const float *)means, (const float *)log_scales, (const float4 *)rotations, key, (float *)means_out,
                           (float *)log_scales_out);
    else
        hipLaunchKernelGGL(k_densify_geometry<3>, dim3(div_up(n_out, DT)), dim3(DT), 0, ctx->stream, (const uint32_t *)rows, n_out,
                           (const float *)means, (const float *)log_scales, (const float4 *)rotations, key, (float *)means_out,
                           (float *)log_scales_out);
    LAUNCH_CHECK(ctx, "k_densify_geometry");
    return SPLAT_OK;
}

extern "C" int splat_densify_geometry(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *means, const void *log_scales,
                                      const void *rotations, const splat_densify_cfg *cfg, void *means_out, void *log_scales_out) {
    return densify_geometry(ctx, 3, rows, n_out, means, log_scales, rotations, cfg, means_out, log_scales_out);
}

extern "C" int splat_densify_geometry_surfel(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *means, const void *log_scales,
                                             const void *rotations, const splat_densify_cfg *cfg, void *means_out, void *log_scales_out) {
    return densify_geometry(ctx, 2, rows, n_out, means, log_scales, rotations, cfg, means_out, log_scales_out);
}

extern "C" int splat_densify_rows(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *in, void *out, uint32_t floats_per_row,
                                  uint32_t mode) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, mode == SPLAT_DENSIFY_COPY || mode == SPLAT_DENSIFY_ZERO_NEW);
    if (n_out == 0) return SPLAT_OK;
    ARG_CHECK(ctx, rows && in && out && in != out && floats_per_row >= 1 && (uint64_t)n_out * floats_per_row <= DENSITY_MAX_FLOATS);
    ARG_CHECK(ctx, (((uintptr_t)rows | (uintptr_t)in | (uintptr_t)out) & 3) == 0);
    const bool vec = (floats_per_row & 3u) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const uint32_t per = vec ? floats_per_row / 4 : floats_per_row, total = n_out * per;
    if (vec)
        hipLaunchKernelGGL(k_densify_rows<true>, dim3(div_up(total, DT)), dim3(DT), 0, ctx->stream, (const uint32_t *)rows, total, per, in, out,
                           mode == SPLAT_DENSIFY_ZERO_NEW);
    else
        hipLaunchKernelGGL(k_densify_rows<false>, dim3(div_up(total, DT)), dim3(DT), 0, ctx->stream, (const uint32_t *)rows, total, per, in, out,
                           mode == SPLAT_DENSIFY_ZERO_NEW);
    LAUNCH_CHECK(ctx, "k_densify_rows");
    return SPLAT_OK;
}
