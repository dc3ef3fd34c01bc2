// grad.hip — gradients of a frame of anisotropic 3D Gaussians (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference
// counterpart): the backward passes of the composite, of the ellipsoid projector and of the SH colour.
//
// k_composite_backward   one 256-thread workgroup per 16x16 tile, one pixel per lane (k_composite's pixel mapping).
//   Walk 1, front to back over the tile's list in chunks of GCH entries staged in LDS, recomputes each pixel's forward in the
//   operation order of the kernel that drew the frame (composite_uses_px; this file is compiled with contraction on, as
//   composite.hip is): L, the number of entries the pixel consumed (up to and including the one its early-out stopped at),
//   T_{L-1} and T_L.  <PX = false> k_composite's T -= T (g o); <PX = true> k_composite_px's T = fma(-o, T g, T).  The two
//   round differently, and where T lands within an ulp or two of T_STOP they stop a pixel at different entries.
//   Walk 2 goes back to front from the tile's largest L, chunk by chunk.  Per entry i < L a pixel recovers
//   T_i = T_{i+1} / (1 - alpha_i) (except at its last entry, whose T_{L-1} it kept: only there may 1 - alpha be <= 0.01) and
//   forms dL/dalpha_i = T_i (G.c_i - S_i), S the blend of everything behind the entry, with alpha as a fourth channel
//   (colour 1, background 0).  Each wave sums its 64 lanes' nine numbers per entry with DPP (skipped when the ballot says no
//   lane of the wave is inside the entry); the four waves' sums meet in LDS, and after the chunk one float atomic add per
//   (entry, number) goes to grad_records (8 floats per splat: c.x, c.y, B00, B01, -, B11, -, -) and grad_color_opacity
//   (4 per splat: r, g, b, opacity).  The sums depend on the atomics' arrival order: reproducible to rounding only.
//   <DEPTH = true> (splat_composite_backward_depth) also differentiates the AOV depth D = sum w z / sum w: walk 1 sums
//   ws = sum w and zw = sum w z beside T, walk 2 carries D as a fifth channel of colour z_i - D, background 0 and upstream
//   G_D / ws, and each entry sums a tenth number, w_i G_D / ws, into grad_depth (1 float per splat).  z_i is staged in the
//   entry's unused c.y.
//   <DET = true> (splat_composite_backward_det) hands the same per-(entry, number) sums to no atomic: it stores them to slots
//   of the caller's workspace, splat-major (k_det_rect_count and the scan give every splat the first slot of its tile
//   rectangle; a tile's slot is its row-major position in it), and writes per tile {largest L, depth key and index of its last
//   consumed entry}.  k_det_gather then adds, per splat, the slots of the tiles that consumed it - lists ascend in (key,
//   index), so one compare with the tile's row decides - each tile row left to right, the rows top to bottom, and the total
//   once into the splat's row: the order include/splat.h states, the same bits on every run.  The instantiations without DET
//   are the kernel as it was, instruction for instruction.
//   <ABS = true> (splat_composite_backward_abs, splat_composite_backward_det_abs) sums two more numbers per entry, |term c.x| and
//   |term c.y|: the absolute values of the very terms numbers 0 and 1 add (AbsGS's homodirectional gradient: a splat whose
//   pixels pull its centre in opposite directions keeps a large statistic where the signed sum cancels).  They take the path
//   of the others - a DPP sum per wave under the same ballot, the partials in LDS, (w0 + w1) + (w2 + w3), then a float atomic
//   add or a slot store - into grad_center_abs (2 floats per splat).  The order of an entry's numbers: c.x, c.y, B00, B01,
//   B11, r, g, b, opacity, (DEPTH: z,) (ABS: |c.x|, |c.y|): the two new ones last, so that k < GNV means what it meant; a det
//   slot then holds 11 (12) floats.  The instantiations without ABS are the kernel as it was, instruction for instruction.
// k_composite_contribution   (splat_composite_contribution) walk 1 alone, with every lane kept in the loop: per consumed entry
//   inside the cut a pixel's blend weight w = T alpha, in the drawing kernel's operation order as above (<PX>), times the
//   pixel's mask.  Per entry and wave a ballot counts the hits and two integer DPP trees give the largest weight (non-negative
//   floats order as their bit patterns) and the sum of the weights in fixed point; the four waves' partials meet in LDS, and
//   after the chunk at most one integer atomic per (entry, output) goes to global memory.  Integer max, sum and count do not
//   depend on the order of arrival: the same bits on every run.
// k_project_ellipsoid_backward   one thread per splat: the record's gradient through B = U / 3, U(a, b, c), Sigma2 = T T^T + 0.3 I,
//   T = J M, M = R S, the quaternion's normalisation and J's and the centre's dependence on the position, in float64.  The
//   cull decisions are ellipsoid_record's own (binary32); a culled splat gets exact zeros.  <DEPTH = true> adds the ProjectedSplat
//   depth's term, dL/dz (p - eye) / |p - eye|, to dL/dposition.
// k_sh_colors_backward   one thread per splat: sh.hip's basis and constants, dir = normalize(p - eye), zero where the
//   forward's max(., 0) clamped.
// <CAM = true> of both, with k_camera_sum_slices and k_camera_sum: the camera's gradient, dL/d(VP, eye) — each splat's share
//   formed in float64 beside its other gradients and summed over all splats in a fixed order (the lanes of a wave by DPP,
//   per-wave partials in the context's scratch, the partials slice by slice in index order), so that the same inputs give the
//   same bits on every run.  The instantiations without CAM are the kernels above,
//   instruction for instruction.
#include "common.h"
#include "variant.h"
#include "tile_range.h"
#include "disc.h"
#include "ellipsoid.h"

namespace {

constexpr int GT = 16;          // tile edge
constexpr int GCH = 64;         // list entries per staged chunk
constexpr int GNV = 9;          // numbers summed per entry: c.x, c.y, B00, B01, B11, r, g, b, opacity (DEPTH: and z)
constexpr int GNABS = 2;        // (ABS) and, after all of those, |term c.x|, |term c.y|
// numbers per entry of a variant, and of it without the absolute sums (the index of |term c.x| where it has them)
constexpr int grad_nv_base(bool depth) { return depth ? GNV + 1 : GNV; }
constexpr int grad_nv(bool depth, bool abs) { return grad_nv_base(depth) + (abs ? GNABS : 0); }
constexpr float G_T_STOP = 0x1.47ae4p-7f; // composite.h's T_STOP: the last transmittance that stops a pixel
constexpr float G_EXP2_SCALE = -6.492127684000335f; // composite.h's ELLIPSOID_EXP2_SCALE: exp(-4.5 d2) = exp2(d2 * this)

struct GradEntry {
    float4 a;   // c.x, c.y, B00, B01
    float4 b;   // B11, opacity, r, g
    float4 c;   // b, z (DEPTH; else 0), -, -
    float4 bnd; // the record's exact 3-sigma box (all zeros: covers no pixel)
};

// The sum of v over the wave's 64 lanes, valid in lane 63 (quad swaps, rotations by 4 and 8 in each row of 16, then the
// row broadcasts 15 and 31 into rows 1, 3 and 2, 3)
__device__ __forceinline__ float wave_sum63(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false)); // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false)); // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false)); // row_ror:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false)); // row_ror:8
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false)); // row_bcast:15
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false)); // row_bcast:31
    return v;
}

// wave_sum63 and its unsigned maximum on 32-bit integers (lanes a row mask leaves out read 0: neutral for both)
__device__ __forceinline__ uint32_t wave_add63_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false); // row_ror:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false); // row_ror:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31
    return v;
}
__device__ __forceinline__ uint32_t wave_max63_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return v;
}

struct BackParams {
    const float4 *color; uint32_t color_stride;
    const float4 *records;
    const uint32_t *indices, *counts, *offsets;
    uint32_t width, height, ntx;
    const float4 *grad_img;
    float *grad_records;
    float *grad_color;
};

// the depth variant's further arguments: z_i = z[i * z_stride], dL/dD per pixel (W*H), dL/dz_i added into grad_depth[i]
struct BackDepthParams : BackParams {
    const float *z; uint32_t z_stride;
    const float *grad_depth_img;
    float *grad_depth;
};

// the fixed-order variant's further arguments (splat_composite_backward_det): the ProjectedSplats the lists were binned from
// and the three parts of the caller's workspace.  It does not write grad_records / grad_color / grad_depth: k_det_gather does.
struct BackDetParams : BackDepthParams {
    const float4 *projected;    // 2 float4 per splat: bounds, then depth in .x
    const uint32_t *slot_base;  // per splat: its first slot (the exclusive scan of the rectangles' tile counts)
    float *slots;               // slot_cap slots of NV floats, splat-major
    uint4 *tile_table;          // per tile {largest L, depth key and splat index of the last consumed entry, 0}
    uint32_t slot_cap, nty;
};

// the absolute-sum variants' further argument (splat_composite_backward_abs, _det_abs): 2 floats per splat, ADDED into
struct BackAbsParams : BackDetParams {
    float *grad_abs;
};

constexpr uint32_t DET_NO_SLOT = 0xffffffffu;

// splat_composite_contribution's arguments: the frame's (the gradient pointers of BackParams are not read), the pixel mask (NULL:
// 1 everywhere) and the three per-splat outputs (each NULL: not wanted)
struct ContribParams : BackParams {
    const float *pixel_weight;
    float min_weight;
    uint32_t *hits;
    uint32_t *weight_max;          // binary32 bit patterns
    unsigned long long *weight_sum; // units of 2^-24
};

// extract-depth-keys' key of a ProjectedSplat depth (project.hip's depth_key): the lists ascend in (key, index)
__device__ __forceinline__ uint32_t det_depth_key(float depth) {
    const uint32_t bits = __float_as_uint(depth);
    return bits ^ (((bits >> 31) == 1u) ? 0xffffffffu : 0x80000000u);
}

// Splat idx's slot for tile (tx, ty): slot_base[idx] + the tile's row-major position in the splat's tile rectangle (the
// binner's tile_range of its bounds over the whole screen).  DET_NO_SLOT for a tile outside the rectangle (lists that were
// not binned from this `projected`) or a slot at or past slot_cap: nothing is stored then.
__device__ __forceinline__ uint32_t det_slot(const BackDetParams &p, uint32_t idx, uint32_t tx, uint32_t ty) {
    uint32_t tx0, tx1, ty0, ty1;
    if (!tile_range(p.projected[(size_t)idx * 2], p.width, p.height, GT, p.ntx, p.nty, 0u, p.nty, tx0, tx1, ty0, ty1)) return DET_NO_SLOT;
    if (tx < tx0 || tx > tx1 || ty < ty0 || ty > ty1) return DET_NO_SLOT;
    const uint64_t slot = (uint64_t)p.slot_base[idx] + (uint64_t)(ty - ty0) * (tx1 - tx0 + 1u) + (tx - tx0);
    return slot < p.slot_cap ? (uint32_t)slot : DET_NO_SLOT;
}

// stages entries [c0, c0 + m) of the tile's list (threads 0 .. m-1)
template <bool DEPTH, typename P>
__device__ __forceinline__ void stage_chunk(const P &p, uint32_t off, uint32_t c0, uint32_t m, GradEntry *s_ent, uint32_t *s_idx) {
    const uint32_t t = threadIdx.x;
    if (t < m) {
        const uint32_t idx = p.indices[off + c0 + t];
        const DiscRecord rec = {p.records[(size_t)idx * 2], p.records[(size_t)idx * 2 + 1]};
        float4 bnd;
        const bool ok = disc_bounds(rec, bnd); // all zeros when not: no pixel centre (>= 0.5) is inside
        const float4 col = p.color[(size_t)idx * p.color_stride];
        GradEntry e;
        e.a = rec.a;
        e.b = make_float4(rec.b.y, col.w, col.x, col.y);
        if constexpr (DEPTH) e.c = make_float4(col.z, p.z[(size_t)idx * p.z_stride], 0.0f, 0.0f);
        else e.c = make_float4(col.z, 0.0f, 0.0f, 0.0f);
        e.bnd = ok ? bnd : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_ent[t] = e;
        s_idx[t] = idx;
    }
}

// alpha of entry e at pixel centre (pxf, pyf) in k_composite's operation order (ELL, q = 0: rd = 1); ge = the exponential,
// d2, u, v and the pixel offset returned for the backward.  Outside the box or the cut: false.
__device__ __forceinline__ bool entry_alpha(const GradEntry &e, float pxf, float pyf, float &alpha, float &ge, float &u, float &v, float &dx,
                                            float &dy) {
    const bool in_box = !(pxf < e.bnd.x || pxf > e.bnd.z || pyf < e.bnd.y || pyf > e.bnd.w);
    dx = pxf - e.a.x;
    dy = pyf - e.a.y;
    u = e.a.z * dx + e.a.w * dy;
    v = e.b.x * dy; // (B10 = 0: the forward's 0 dx + B11 dy, the same value for a finite dx)
    const float d2 = u * u + v * v;
    ge = (d2 <= 1.0f) ? __builtin_amdgcn_exp2f(d2 * G_EXP2_SCALE) : 0.0f;
    alpha = ge;
    alpha *= e.b.y;
    return in_box && d2 <= 1.0f;
}

} // namespace

// (DET) per staged entry its slot; no LDS in the instantiations without
template <bool DET>
__device__ __forceinline__ uint32_t *det_slot_lds() {
    if constexpr (DET) {
        __shared__ uint32_t s_slot[GCH];
        return s_slot;
    } else {
        return nullptr;
    }
}

// <DET = true> (splat_composite_backward_det): the same sums, stored to the splat-major slots of BackDetParams for k_det_gather
// to add in a fixed order, where <DET = false> hands them to float atomic adds into the splats' rows.
// <ABS = true>: two more sums per entry, |term c.x| and |term c.y|, after the others (file header); the argument is then
// BackAbsParams, with or without DET.
template <bool DEPTH, bool PX, bool DET = false, bool ABS = false>
__global__ __launch_bounds__(256) void k_composite_backward(
    std::conditional_t<ABS, BackAbsParams, std::conditional_t<DET, BackDetParams, std::conditional_t<DEPTH, BackDepthParams, BackParams>>> p) {
    constexpr int NV = grad_nv(DEPTH, ABS); // (the tenth: dL/dz; ABS: the last two)
    constexpr int NVB = grad_nv_base(DEPTH);
    __shared__ GradEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ float s_part[4][GCH][NV];
    __shared__ uint32_t s_touch[GCH];
    __shared__ uint32_t s_maxL;
    uint32_t *const s_slot = det_slot_lds<DET>();

    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t tx = blockIdx.x, ty = blockIdx.y;
    const uint32_t tile_idx = ty * p.ntx + tx;
    const uint32_t count = p.counts[tile_idx], off = p.offsets[tile_idx];
    const uint32_t px = tx * GT + (w & 1) * 8 + (lane & 7), py = ty * GT + (w >> 1) * 8 + (lane >> 3);
    const bool pixel_ok = px < p.width && py < p.height;
    const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f;

    // ---- walk 1: front to back, the forward's stop rule ----
    bool live = pixel_ok;
    uint32_t L = 0;
    float T = 1.0f, T_last = 1.0f; // T_L, T_{L-1}
    float zw = 0.0f, ws = 0.0f;    // (DEPTH) sum w z, sum w over the consumed entries, as AovPixel sums them
    if (tid == 0) s_maxL = 0;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads();
        stage_chunk<DEPTH>(p, off, c0, m, s_ent, s_idx);
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < m; ++j) {
                float alpha, ge, u, v, dx, dy;
                const bool in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
                float wgt;
                T_last = T;
                if constexpr (PX) { // k_composite_px: the colour premultiplied by the opacity, w = T g, T = fma(-opacity, w, T)
                    const float w = T * (in ? ge : 0.0f);
                    wgt = w * s_ent[j].b.y; // (its AOV's weight)
                    T = __builtin_fmaf(-s_ent[j].b.y, w, T);
                } else { // k_composite: alpha = g opacity, w = T alpha, T -= w
                    const float g = in ? alpha : 0.0f;
                    wgt = T * g;
                    T -= wgt;
                }
                if constexpr (DEPTH) {
                    zw += s_ent[j].c.y * wgt;
                    ws += wgt;
                }
                if (T <= G_T_STOP) {
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
    // (DEPTH) D and G_D / ws; no gradient, and G_D not read, where nothing contributed
    float D = 0.0f, GDn = 0.0f;
    if constexpr (DEPTH) {
        if (pixel_ok && ws > 0.0f) {
            D = zw / ws;
            GDn = p.grad_depth_img[(size_t)py * p.width + px] / ws;
        }
    }
    float Tn = T;                                          // T_{i+1} on the way back
    __syncthreads();
    const uint32_t maxL = s_maxL;
    if constexpr (DET) { // the tile's row of the table: which of its entries have a slot that walk 2 stores
        if (tid == 0) {
            uint4 row = make_uint4(maxL, 0u, 0u, 0u);
            if (maxL) {
                row.z = p.indices[off + maxL - 1];
                row.y = det_depth_key(p.projected[(size_t)row.z * 2 + 1].x);
            }
            p.tile_table[tile_idx] = row;
        }
    }

    // ---- walk 2: back to front from the tile's largest L ----
    for (uint32_t cend = maxL; cend > 0;) {
        const uint32_t c0 = cend > GCH ? cend - GCH : 0, m = cend - c0;
        __syncthreads(); // the previous chunk's sums are added
        stage_chunk<DEPTH>(p, off, c0, m, s_ent, s_idx);
        if constexpr (DET) {
            if (tid < m) s_slot[tid] = det_slot(p, s_idx[tid], tx, ty); // (s_idx[tid]: this thread's own store)
        }
        if (tid < GCH) s_touch[tid] = 0;
        __syncthreads();
        for (int j = (int)m - 1; j >= 0; --j) {
            const uint32_t i = c0 + (uint32_t)j;
            float alpha = 0.0f, ge = 0.0f, u = 0.0f, v = 0.0f, dx = 0.0f, dy = 0.0f;
            bool in = false;
            if (i < L) in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
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
                const GradEntry &e = s_ent[j];
                const float Ti = (i + 1 == L) ? T_last : Tn / (1.0f - alpha);
                float cg = ((G.x * e.b.z + G.y * e.b.w) + G.z * e.c.x) + G.w; // G . (c, 1)
                if constexpr (DEPTH) cg += GDn * (e.c.y - D);                   // the centred depth channel
                const float dA = Ti * (cg - S);
                const float wgt = Ti * alpha;
                vals[5] = wgt * G.x;
                vals[6] = wgt * G.y;
                vals[7] = wgt * G.z;
                vals[8] = ge * dA;
                if constexpr (DEPTH) vals[9] = wgt * GDn;
                const float dd2 = -4.5f * alpha * dA;
                const float du = 2.0f * u * dd2, dv = 2.0f * v * dd2;
                vals[0] = -du * e.a.z;              // d2 / c.x
                vals[1] = -(du * e.a.w + dv * e.b.x); // d2 / c.y
                vals[2] = du * dx;                   // d2 / B00
                vals[3] = du * dy;                   // d2 / B01
                vals[4] = dv * dy;                   // d2 / B11
                if constexpr (ABS) {
                    vals[NVB] = fabsf(vals[0]);
                    vals[NVB + 1] = fabsf(vals[1]);
                }
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
        if constexpr (DET) {
            // one store per (entry, number), touched or not (an untouched entry's four partials are zeros): every slot below
            // the tile's largest L is written, NV contiguous floats each
            for (uint32_t q = tid; q < m * NV; q += 256) {
                const uint32_t e = q / NV, k = q - e * NV;
                const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
                const uint32_t slot = s_slot[e];
                if (slot != DET_NO_SLOT) p.slots[(size_t)slot * NV + k] = sum;
            }
        } else {
            // one atomic add per touched (entry, number): the nine sums of an entry are its records row (20 of 32 bytes) and
            // its colour row (16 bytes), the depth variant's tenth its grad_depth word
            for (uint32_t q = tid; q < m * NV; q += 256) {
                const uint32_t e = q / NV, k = q - e * NV;
                if (!s_touch[e]) continue;
                const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
                const size_t idx = s_idx[e];
                float *dst = k < 5 ? p.grad_records + idx * 8 + (k < 4 ? k : 5u) : p.grad_color + idx * 4 + (k - 5);
                if constexpr (DEPTH) dst = k == GNV ? p.grad_depth + idx : dst;
                if constexpr (ABS) dst = k >= (uint32_t)NVB ? p.grad_abs + idx * 2 + (k - NVB) : dst;
                atomicAdd(dst, sum);
            }
        }
        cend = c0;
    }
}

// k_composite_contribution   (file header) the blend weight of every (pixel, consumed entry inside the cut) pair, reduced per splat
//   to a hit count, a maximum and a fixed-point sum, all ACCUMULATED into the caller's buffers.  Walk 1's arithmetic, but its
//   per-lane break at the stop would take lanes out of the wave-wide reductions: here the loop over a chunk is uniform and a
//   stopped pixel is a predicate, as walk 2's i < L is.  A wave with no live pixel skips the chunk (its partials were zeroed
//   with the staging); the workgroup leaves after the chunk in which its last pixel stopped.
//   wm = clamp(m T alpha, 0, 1) (the clamp acts only on an opacity outside [0, 1] or not finite: NaN -> 0), q = rint(wm 2^24) <=
//   2^24: a wave's 64 fit 32 bits (2^30), the tile's four waves are added in 64.
template <bool PX>
__global__ __launch_bounds__(256) void k_composite_contribution(ContribParams p) {
    __shared__ GradEntry s_ent[GCH];
    __shared__ uint32_t s_idx[GCH];
    __shared__ uint32_t s_part[3][4][GCH]; // hits, largest weight's bits, sum of q: per wave and entry

    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t tx = blockIdx.x, ty = blockIdx.y;
    const uint32_t tile_idx = ty * p.ntx + tx;
    const uint32_t count = p.counts[tile_idx], off = p.offsets[tile_idx];
    const uint32_t px = tx * GT + (w & 1) * 8 + (lane & 7), py = ty * GT + (w >> 1) * 8 + (lane >> 3);
    const bool pixel_ok = px < p.width && py < p.height;
    const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f;
    float msk = pixel_ok ? 1.0f : 0.0f;
    if (pixel_ok && p.pixel_weight) msk = __builtin_fminf(__builtin_fmaxf(p.pixel_weight[(size_t)py * p.width + px], 0.0f), 1.0f); // (NaN -> 0)

    bool live = pixel_ok;
    float T = 1.0f;
    for (uint32_t c0 = 0; c0 < count; c0 += GCH) {
        const uint32_t m = min((uint32_t)GCH, count - c0);
        __syncthreads(); // the previous chunk's partials are added
        stage_chunk<false>(p, off, c0, m, s_ent, s_idx);
        (&s_part[0][0][0])[tid] = 0u;
        (&s_part[0][0][0])[tid + 256] = 0u;
        (&s_part[0][0][0])[tid + 512] = 0u;
        __syncthreads();
        if (__ballot(live) != 0ull) {
            for (uint32_t j = 0; j < m; ++j) {
                bool has = false, hit = false;
                float wm = 0.0f;
                if (live) {
                    float alpha, ge, u, v, dx, dy;
                    const bool in = entry_alpha(s_ent[j], pxf, pyf, alpha, ge, u, v, dx, dy);
                    float wgt;
                    if constexpr (PX) { // k_composite_px: w = T g, T = fma(-opacity, w, T); its AOV's weight w opacity
                        const float wg = T * (in ? ge : 0.0f);
                        wgt = wg * s_ent[j].b.y;
                        T = __builtin_fmaf(-s_ent[j].b.y, wg, T);
                    } else { // k_composite: alpha = g opacity, w = T alpha, T -= w
                        const float g = in ? alpha : 0.0f;
                        wgt = T * g;
                        T -= wgt;
                    }
                    live = !(T <= G_T_STOP); // (this entry, the one the pixel stops at, is still consumed)
                    has = in && msk > 0.0f;
                    wm = has ? __builtin_fminf(__builtin_fmaxf(msk * wgt, 0.0f), 1.0f) : 0.0f;
                    hit = has && wm >= p.min_weight;
                }
                if (__ballot(has) == 0ull) continue;
                const uint32_t nhit = (uint32_t)__popcll(__ballot(hit));
                const uint32_t mx = wave_max63_u32(__float_as_uint(wm));
                const uint32_t sm = wave_add63_u32((uint32_t)__builtin_rintf(wm * 0x1p24f));
                if (lane == 63) {
                    s_part[0][w][j] = nhit;
                    s_part[1][w][j] = mx;
                    s_part[2][w][j] = sm;
                }
            }
        }
        const int any = __syncthreads_or(live);
        // wave k adds output k of the chunk's entries: at most one atomic per (entry, output), none for a zero partial
        if (tid < 3 * GCH && lane < m) {
            const uint32_t a = s_part[w][0][lane], b = s_part[w][1][lane], c = s_part[w][2][lane], d = s_part[w][3][lane];
            const size_t idx = s_idx[lane];
            if (w == 0) {
                const uint32_t hits = (a + b) + (c + d);
                if (hits && p.hits) atomicAdd(p.hits + idx, hits);
            } else if (w == 1) {
                const uint32_t mx = max(max(a, b), max(c, d));
                if (mx && p.weight_max) atomicMax(p.weight_max + idx, mx);
            } else {
                const unsigned long long sum = ((unsigned long long)a + b) + ((unsigned long long)c + d);
                if (sum && p.weight_sum) atomicAdd(p.weight_sum + idx, sum);
            }
        }
        if (!any) break;
    }
}

// The number of tiles in every splat's tile rectangle (0: it bins nowhere); their exclusive scan is slot_base.
__global__ __launch_bounds__(256) void k_det_rect_count(const float4 *__restrict__ projected, uint32_t n, uint32_t width, uint32_t height,
                                                        uint32_t ntx, uint32_t nty, uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t tx0, tx1, ty0, ty1;
    const bool ok = tile_range(projected[(size_t)i * 2], width, height, GT, ntx, nty, 0u, nty, tx0, tx1, ty0, ty1);
    count[i] = ok ? (tx1 - tx0 + 1u) * (ty1 - ty0 + 1u) : 0u; // (at most 65535^2)
}

// One tile row of a splat's rectangle: (((+0 + P(tile 0)) + P(tile 1)) + ...) over the `cols` tiles from `tile0`, whose slots
// start at slot0.  A slot holds a sum exactly when its tile consumed the splat's entry: lists ascend strictly in (depth key,
// index), so that is when (key, idx) is not past the tile's last consumed entry.  Other tiles add nothing.
template <int NV>
__device__ __forceinline__ bool det_row_sum(const BackDetParams &p, uint32_t tile0, uint32_t cols, uint64_t slot0, uint32_t key, uint32_t idx,
                                            float (&row)[NV]) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < NV; ++k) row[k] = 0.0f;
    for (uint32_t c = 0; c < cols; ++c) {
        const uint4 t = p.tile_table[tile0 + c];
        const uint64_t slot = slot0 + c;
        if (t.x == 0u || key > t.y || (key == t.y && idx > t.z) || slot >= p.slot_cap) continue;
        const float *src = p.slots + (size_t)slot * NV;
        any = true;
#pragma unroll
        for (int k = 0; k < NV; ++k) row[k] += src[k];
    }
    return any;
}

// k_det_gather   one thread per splat: the slots of its rectangle added in the contract's order (include/splat.h) — each tile
//   row left to right from +0, the rows top to bottom from +0 — and the total added once to the splat's prior row.  A
//   rectangle of more than DET_WIDE tiles in more than one row is taken by its whole wave in turn: lane r sums row r (and r +
//   64, ...), and the row sums are then added in row order, read lane by lane.  Which lanes add what changes; the order of
//   the additions does not.  A splat with no consumed entry keeps its prior bits.
constexpr uint32_t DET_WIDE = 64;

// <ABS = true>: the slots' last two numbers too, in the same order, into grad_abs.
template <bool DEPTH, bool ABS = false>
__global__ __launch_bounds__(256) void k_det_gather(std::conditional_t<ABS, BackAbsParams, BackDetParams> p, uint32_t n) {
    constexpr int NV = grad_nv(DEPTH, ABS);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t tx0 = 0, tx1 = 0, ty0 = 0, ty1 = 0, key = 0, base = 0;
    bool ok = false;
    if (i < n) {
        ok = tile_range(p.projected[(size_t)i * 2], p.width, p.height, GT, p.ntx, p.nty, 0u, p.nty, tx0, tx1, ty0, ty1);
        key = det_depth_key(p.projected[(size_t)i * 2 + 1].x);
        base = p.slot_base[i];
    }
    const uint32_t cols = ok ? tx1 - tx0 + 1u : 0u, rows = ok ? ty1 - ty0 + 1u : 0u;
    const bool wide = rows > 1u && cols * rows > DET_WIDE;
    float total[NV];
    bool any = false;
#pragma unroll
    for (int k = 0; k < NV; ++k) total[k] = 0.0f;
    if (ok && !wide) {
        for (uint32_t r = 0; r < rows; ++r) {
            float row[NV];
            any |= det_row_sum<NV>(p, (ty0 + r) * p.ntx + tx0, cols, (uint64_t)base + (uint64_t)r * cols, key, i, row);
#pragma unroll
            for (int k = 0; k < NV; ++k) total[k] += row[k];
        }
    }
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = __ffsll((long long)todo) - 1;
        const uint32_t s_tx0 = __shfl(tx0, src), s_ty0 = __shfl(ty0, src), s_cols = __shfl(cols, src), s_rows = __shfl(rows, src);
        const uint32_t s_key = __shfl(key, src), s_base = __shfl(base, src), s_idx = (i - lane) + (uint32_t)src;
        float tot[NV];
        bool mine = false;
#pragma unroll
        for (int k = 0; k < NV; ++k) tot[k] = 0.0f;
        for (uint32_t r0 = 0; r0 < s_rows; r0 += 64u) {
            const uint32_t r = r0 + lane, cnt = min(64u, s_rows - r0);
            float row[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) row[k] = 0.0f;
            if (r < s_rows)
                mine |= det_row_sum<NV>(p, (s_ty0 + r) * p.ntx + s_tx0, s_cols, (uint64_t)s_base + (uint64_t)r * s_cols, s_key, s_idx, row);
            for (uint32_t q = 0; q < cnt; ++q) {
#pragma unroll
                for (int k = 0; k < NV; ++k) tot[k] += __shfl(row[k], (int)q);
            }
        }
        const bool hit = __ballot(mine) != 0ull;
        if ((int)lane == src) {
            any = hit;
#pragma unroll
            for (int k = 0; k < NV; ++k) total[k] = tot[k];
        }
    }
    if (!any) return;
    float *grec = p.grad_records + (size_t)i * 8, *gcol = p.grad_color + (size_t)i * 4;
#pragma unroll
    for (int k = 0; k < 5; ++k) grec[k < 4 ? k : 5] += total[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) gcol[k] += total[5 + k];
    if constexpr (DEPTH) p.grad_depth[i] += total[GNV];
    if constexpr (ABS) {
        float *gabs = p.grad_abs + (size_t)i * 2;
#pragma unroll
        for (int k = 0; k < GNABS; ++k) gabs[k] += total[grad_nv_base(DEPTH) + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
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

// v's sum over the wave's 64 lanes, valid in lane 63: wave_sum63's six steps on a double (two 32-bit DPP moves each)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum63_f64(double v) {
    v = dpp_add_f64<0xb1, 0xf>(v);  // quad_perm [1,0,3,2]
    v = dpp_add_f64<0x4e, 0xf>(v);  // quad_perm [2,3,0,1]
    v = dpp_add_f64<0x124, 0xf>(v); // row_ror:4
    v = dpp_add_f64<0x128, 0xf>(v); // row_ror:8
    v = dpp_add_f64<0x142, 0xa>(v); // row_bcast:15
    v = dpp_add_f64<0x143, 0xc>(v); // row_bcast:31
    return v;
}

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
        float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            r += Y[k] * row[3 * k];
            g += Y[k] * row[3 * k + 1];
            b += Y[k] * row[3 * k + 2];
        }
        // the clamp: no gradient where the forward's max(., 0) took the 0
        const float gr = (r + 0.5f > 0.0f) ? gc.x : 0.0f, gg = (g + 0.5f > 0.0f) ? gc.y : 0.0f, gb = (b + 0.5f > 0.0f) ? gc.z : 0.0f;
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
// The two composite backwards: their checks, the kernel's parameters and the launch.  depth: splat_composite_backward_depth,
// with its four further arguments.
// det: splat_composite_backward_det's further arguments, or NULL for the two atomic entry points.
// abs: the _abs entry points, with grad_center_abs (n x 2 floats, 8-byte aligned, ADDED into).
struct DetArgs {
    const void *projected;
    uint64_t total_pairs;
    void *workspace;
    uint64_t workspace_bytes;
};

// The workspace of splat_composite_backward_det: the tile table (16 bytes per tile), slot_base (4 bytes per splat, rounded up
// to 16) and the slots (4 NV bytes per pair, NV = 9, or 10 with depth; the _abs entry points: 11, or 12).  0 where it would
// not fit 64 bits (judged by the largest slot of the family: 40 bytes, 48 with the absolute sums).
static uint64_t det_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, bool depth, uint64_t *slot_base_off = nullptr,
                                    uint64_t *slots_off = nullptr, bool abs = false) {
    const uint64_t table = (uint64_t)num_tiles * 16u, base = ((uint64_t)n * 4u + 15u) & ~15ull;
    if (slot_base_off) *slot_base_off = table;
    if (slots_off) *slots_off = table + base;
    if (total_pairs > (~0ull - table - base) / (4u * (uint64_t)grad_nv(true, abs))) return 0;
    return table + base + total_pairs * 4u * (uint64_t)grad_nv(depth, abs);
}

extern "C" uint64_t splat_composite_backward_det_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth) {
    return det_workspace_bytes(total_pairs, num_tiles, n, with_depth != 0);
}

extern "C" uint64_t splat_composite_backward_det_abs_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth) {
    return det_workspace_bytes(total_pairs, num_tiles, n, with_depth != 0, nullptr, nullptr, true);
}

static int composite_backward_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                     const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                     uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                     void *grad_color_opacity, bool depth, const void *depth_f32, uint32_t depth_stride_floats,
                                     const void *grad_depth_f32, void *grad_depth, const DetArgs *det = nullptr, bool abs = false,
                                     void *grad_center_abs = nullptr) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, cfg != nullptr);
    if (cfg->footprint != SPLAT_FOOTPRINT_ELLIPSOID || cfg->mode != SPLAT_COMPOSITE_FRONT_TO_BACK || cfg->early_out != 1 ||
        cfg->tile_size != GT || cfg->record_format != SPLAT_RECORDS_PROJECTED)
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_composite_backward: footprint ELLIPSOID, FRONT_TO_BACK, early_out = 1, tile_size = 16 "
                                                "and PROJECTED records only");
    ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= 65535u * GT && height <= 65535u * GT);
    const uint32_t ntx = div_up(width, GT), nty = div_up(height, GT);
    ARG_CHECK(ctx, cfg->tile_row0 == 0 && cfg->tile_row1 >= nty); // the whole screen: no strict band
    ARG_CHECK(ctx, color_stride_vec4 >= 1);
    ARG_CHECK(ctx, color_opacity && records && tile_indices && tile_counts && tile_offsets && grad_rgba32f);
    ARG_CHECK(ctx, n == 0 || (grad_records && grad_color_opacity));
    ARG_CHECK(ctx, (((uintptr_t)color_opacity | (uintptr_t)records | (uintptr_t)grad_rgba32f | (uintptr_t)grad_records |
                     (uintptr_t)grad_color_opacity) & 15) == 0);
    ARG_CHECK(ctx, (((uintptr_t)tile_indices | (uintptr_t)tile_counts | (uintptr_t)tile_offsets) & 3) == 0);
    if (depth) {
        ARG_CHECK(ctx, depth_f32 && grad_depth_f32 && (n == 0 || grad_depth) && depth_stride_floats >= 1);
        ARG_CHECK(ctx, (((uintptr_t)depth_f32 | (uintptr_t)grad_depth_f32 | (uintptr_t)grad_depth) & 3) == 0);
    }
    if (abs) ARG_CHECK(ctx, (n == 0 || grad_center_abs) && ((uintptr_t)grad_center_abs & 7) == 0);
    uint64_t slot_base_off = 0, slots_off = 0;
    if (det) {
        // (a slot index is a u32, as a list offset is)
        ARG_CHECK(ctx, det->projected && ((uintptr_t)det->projected & 15) == 0 && det->total_pairs <= 0xffffffffull);
        const uint64_t need = det_workspace_bytes(det->total_pairs, ntx * nty, n, depth, &slot_base_off, &slots_off, abs);
        ARG_CHECK(ctx, det->workspace && ((uintptr_t)det->workspace & 15) == 0 && need != 0 && det->workspace_bytes >= need);
    }
    if (n == 0) return SPLAT_OK; // (no splat: every list is empty)
    BackAbsParams p{}; // (every kernel takes the base of it that it reads; what a launch does not set is zero)
    p.grad_abs = (float *)grad_center_abs;
    p.color = (const float4 *)color_opacity;
    p.color_stride = color_stride_vec4;
    p.records = (const float4 *)records;
    p.indices = (const uint32_t *)tile_indices;
    p.counts = (const uint32_t *)tile_counts;
    p.offsets = (const uint32_t *)tile_offsets;
    p.width = width;
    p.height = height;
    p.ntx = ntx;
    p.grad_img = (const float4 *)grad_rgba32f;
    p.grad_records = (float *)grad_records;
    p.grad_color = (float *)grad_color_opacity;
    p.z = (const float *)depth_f32;
    p.z_stride = depth_stride_floats;
    p.grad_depth_img = (const float *)grad_depth_f32;
    p.grad_depth = (float *)grad_depth;
    if (det) {
        // slot_base (the scan of the rectangles' tile counts), the tile kernel storing its sums to the slots, the gather
        p.projected = (const float4 *)det->projected;
        p.tile_table = (uint4 *)det->workspace;
        uint32_t *slot_base = (uint32_t *)((char *)det->workspace + slot_base_off);
        p.slot_base = slot_base;
        p.slots = (float *)((char *)det->workspace + slots_off);
        p.slot_cap = (uint32_t)det->total_pairs;
        p.nty = nty;
        launch_kernel(ctx, NO_STAGE, k_det_rect_count, dim3(div_up(n, 256)), dim3(256), p.projected, n, width, height, ntx, nty, slot_base);
        LAUNCH_CHECK(ctx, "launch k_det_rect_count");
        const int rc = splat_scan_u32(ctx, slot_base, slot_base, n, nullptr);
        if (rc != SPLAT_OK) return rc;
        variant_dispatch([&](auto d, auto px, auto ab) {
            launch_kernel(ctx, NO_STAGE, k_composite_backward<d.value, px.value, true, ab.value>, dim3(ntx, nty), dim3(256), p);
        }, depth, composite_uses_px(ctx, ntx, nty), abs);
        LAUNCH_CHECK(ctx, "launch k_composite_backward<DET>");
        variant_dispatch([&](auto d, auto ab) { launch_kernel(ctx, NO_STAGE, k_det_gather<d.value, ab.value>, dim3(div_up(n, 256)), dim3(256), p, n); },
                         depth, abs);
        return launch_check(ctx, "launch k_det_gather");
    }
    // (<DEPTH, PX, ABS>: the kernel without DEPTH or ABS takes the BackParams part of p)
    variant_dispatch([&](auto d, auto px, auto ab) {
        launch_kernel(ctx, NO_STAGE, k_composite_backward<d.value, px.value, false, ab.value>, dim3(ntx, nty), dim3(256), p);
    }, depth, composite_uses_px(ctx, ntx, nty), abs);
    return launch_check(ctx, depth ? "launch k_composite_backward<DEPTH>" : "launch k_composite_backward");
}

extern "C" int splat_composite_backward(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                        const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                        uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                        void *grad_color_opacity) {
    return composite_backward_launch(ctx, cfg, color_opacity, color_stride_vec4, records, tile_indices, tile_counts, tile_offsets, width, height,
                                     grad_rgba32f, n, grad_records, grad_color_opacity, false, nullptr, 0, nullptr, nullptr);
}

extern "C" int splat_composite_backward_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                              uint32_t color_stride_vec4, const void *records, const void *tile_indices, const void *tile_counts,
                                              const void *tile_offsets, uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n,
                                              void *grad_records, void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                              const void *grad_depth_f32, void *grad_depth) {
    return composite_backward_launch(ctx, cfg, color_opacity, color_stride_vec4, records, tile_indices, tile_counts, tile_offsets, width, height,
                                     grad_rgba32f, n, grad_records, grad_color_opacity, true, depth_f32, depth_stride_floats, grad_depth_f32,
                                     grad_depth);
}

extern "C" int splat_composite_backward_det(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                            uint32_t color_stride_vec4, const void *records, const void *projected, const void *tile_indices,
                                            const void *tile_counts, const void *tile_offsets, uint64_t total_pairs, uint32_t width,
                                            uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records, void *grad_color_opacity,
                                            const void *depth_f32, uint32_t depth_stride_floats, const void *grad_depth_f32, void *grad_depth,
                                            void *workspace, uint64_t workspace_bytes) {
    // (colour only: the four depth arguments all NULL / 0; any of them given asks for the depth variant, with its checks)
    const bool depth = depth_f32 || depth_stride_floats || grad_depth_f32 || grad_depth;
    const DetArgs det = {projected, total_pairs, workspace, workspace_bytes};
    return composite_backward_launch(ctx, cfg, color_opacity, color_stride_vec4, records, tile_indices, tile_counts, tile_offsets, width, height,
                                     grad_rgba32f, n, grad_records, grad_color_opacity, depth, depth_f32, depth_stride_floats, grad_depth_f32,
                                     grad_depth, &det);
}

extern "C" int splat_composite_backward_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                            const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                            uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                            void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                            const void *grad_depth_f32, void *grad_depth, void *grad_center_abs) {
    // (the det convention: colour only when the four depth arguments are all NULL / 0)
    const bool depth = depth_f32 || depth_stride_floats || grad_depth_f32 || grad_depth;
    return composite_backward_launch(ctx, cfg, color_opacity, color_stride_vec4, records, tile_indices, tile_counts, tile_offsets, width, height,
                                     grad_rgba32f, n, grad_records, grad_color_opacity, depth, depth_f32, depth_stride_floats, grad_depth_f32,
                                     grad_depth, nullptr, true, grad_center_abs);
}

extern "C" int splat_composite_backward_det_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                                uint32_t color_stride_vec4, const void *records, const void *projected, const void *tile_indices,
                                                const void *tile_counts, const void *tile_offsets, uint64_t total_pairs, uint32_t width,
                                                uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                                void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                                const void *grad_depth_f32, void *grad_depth, void *workspace, uint64_t workspace_bytes,
                                                void *grad_center_abs) {
    const bool depth = depth_f32 || depth_stride_floats || grad_depth_f32 || grad_depth;
    const DetArgs det = {projected, total_pairs, workspace, workspace_bytes};
    return composite_backward_launch(ctx, cfg, color_opacity, color_stride_vec4, records, tile_indices, tile_counts, tile_offsets, width, height,
                                     grad_rgba32f, n, grad_records, grad_color_opacity, depth, depth_f32, depth_stride_floats, grad_depth_f32,
                                     grad_depth, &det, true, grad_center_abs);
}

extern "C" int splat_composite_contribution(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                            const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                            uint32_t width, uint32_t height, const void *pixel_weight_f32, float min_weight, uint32_t n,
                                            void *hits_u32, void *weight_max_f32, void *weight_sum_u64) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, cfg != nullptr);
    if (cfg->footprint != SPLAT_FOOTPRINT_ELLIPSOID || cfg->mode != SPLAT_COMPOSITE_FRONT_TO_BACK || cfg->early_out != 1 ||
        cfg->tile_size != GT || cfg->record_format != SPLAT_RECORDS_PROJECTED)
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_composite_contribution: footprint ELLIPSOID, FRONT_TO_BACK, early_out = 1, tile_size = 16 "
                                                "and PROJECTED records only");
    ARG_CHECK(ctx, width >= 1 && height >= 1 && width <= 65535u * GT && height <= 65535u * GT);
    const uint32_t ntx = div_up(width, GT), nty = div_up(height, GT);
    ARG_CHECK(ctx, cfg->tile_row0 == 0 && cfg->tile_row1 >= nty); // the whole screen: no strict band
    ARG_CHECK(ctx, color_stride_vec4 >= 1);
    ARG_CHECK(ctx, min_weight >= 0.0f); // (NaN fails it)
    ARG_CHECK(ctx, color_opacity && records && tile_indices && tile_counts && tile_offsets);
    ARG_CHECK(ctx, hits_u32 || weight_max_f32 || weight_sum_u64);
    ARG_CHECK(ctx, (((uintptr_t)color_opacity | (uintptr_t)records) & 15) == 0 && ((uintptr_t)weight_sum_u64 & 7) == 0);
    ARG_CHECK(ctx, (((uintptr_t)tile_indices | (uintptr_t)tile_counts | (uintptr_t)tile_offsets | (uintptr_t)pixel_weight_f32 |
                     (uintptr_t)hits_u32 | (uintptr_t)weight_max_f32) & 3) == 0);
    if (n == 0) return SPLAT_OK; // (no splat: every list is empty)
    ContribParams p;
    p.color = (const float4 *)color_opacity;
    p.color_stride = color_stride_vec4;
    p.records = (const float4 *)records;
    p.indices = (const uint32_t *)tile_indices;
    p.counts = (const uint32_t *)tile_counts;
    p.offsets = (const uint32_t *)tile_offsets;
    p.width = width;
    p.height = height;
    p.ntx = ntx;
    p.grad_img = nullptr;
    p.grad_records = nullptr;
    p.grad_color = nullptr;
    p.pixel_weight = (const float *)pixel_weight_f32;
    p.min_weight = min_weight;
    p.hits = (uint32_t *)hits_u32;
    p.weight_max = (uint32_t *)weight_max_f32;
    p.weight_sum = (unsigned long long *)weight_sum_u64;
    variant_dispatch([&](auto px) { launch_kernel(ctx, NO_STAGE, k_composite_contribution<px.value>, dim3(ntx, nty), dim3(256), p); },
                     composite_uses_px(ctx, ntx, nty));
    return launch_check(ctx, "launch k_composite_contribution");
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

// The three ellipsoid projector backwards.  need_depth: grad_depth is required (else optional: NULL = none); cam: also
// dL/duniforms into grad_uniforms, summed from per-wave partials.  what: the launch's name in an error.
static int project_ellipsoid_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                      const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4, uint32_t n,
                                      const void *grad_records, void *grad_positions, void *grad_scales, void *grad_rotations,
                                      const void *grad_depth, bool need_depth, void *grad_uniforms, bool cam, const char *what,
                                      const void *grad_rho = nullptr, bool aa = false) {
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
                launch_kernel(ctx, NO_STAGE, k_project_ellipsoid_backward<depth.value, cam_.value, aa_.value>, dim3(div_up(n, 256)), dim3(256), u,
                              (const float4 *)positions, pos_stride_vec4, (const float4 *)scales, scale_stride_vec4, (const float4 *)rotations,
                              rot_stride_vec4, n, (const float4 *)grad_records, (float4 *)grad_positions, (float4 *)grad_scales,
                              (float4 *)grad_rotations, (const float *)grad_depth);
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

extern "C" int splat_project_ellipsoid_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                                uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales, void *grad_rotations) {
    return project_ellipsoid_backward(ctx, uniforms, positions, pos_stride_vec4, scales, scale_stride_vec4, rotations, rot_stride_vec4, n,
                                      grad_records, grad_positions, grad_scales, grad_rotations, nullptr, false, nullptr, false,
                                      "launch k_project_ellipsoid_backward");
}

extern "C" int splat_project_ellipsoid_backward_depth(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                      const void *scales, uint32_t scale_stride_vec4, const void *rotations,
                                                      uint32_t rot_stride_vec4, uint32_t n, const void *grad_records, void *grad_positions,
                                                      void *grad_scales, void *grad_rotations, const void *grad_depth) {
    return project_ellipsoid_backward(ctx, uniforms, positions, pos_stride_vec4, scales, scale_stride_vec4, rotations, rot_stride_vec4, n,
                                      grad_records, grad_positions, grad_scales, grad_rotations, grad_depth, true, nullptr, false,
                                      "launch k_project_ellipsoid_backward<DEPTH>");
}

extern "C" int splat_project_ellipsoid_backward_camera(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                       const void *scales, uint32_t scale_stride_vec4, const void *rotations,
                                                       uint32_t rot_stride_vec4, uint32_t n, const void *grad_records, void *grad_positions,
                                                       void *grad_scales, void *grad_rotations, const void *grad_depth, void *grad_uniforms) {
    return project_ellipsoid_backward(ctx, uniforms, positions, pos_stride_vec4, scales, scale_stride_vec4, rotations, rot_stride_vec4, n,
                                      grad_records, grad_positions, grad_scales, grad_rotations, grad_depth, false, grad_uniforms, true,
                                      "launch k_project_ellipsoid_backward<CAM>");
}

extern "C" int splat_project_ellipsoid_backward_aa(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                                   const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                                   uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales,
                                                   void *grad_rotations, const void *grad_depth, void *grad_uniforms, const void *grad_rho) {
    return project_ellipsoid_backward(ctx, uniforms, positions, pos_stride_vec4, scales, scale_stride_vec4, rotations, rot_stride_vec4, n,
                                      grad_records, grad_positions, grad_scales, grad_rotations, grad_depth, false, grad_uniforms,
                                      grad_uniforms != nullptr, "launch k_project_ellipsoid_backward<AA>", grad_rho, true);
}

// The two SH backwards.  cam: also dL/deye into grad_eye, summed from per-wave partials.
static int sh_colors_backward(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                              uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, const void *grad_color_opacity, uint32_t n,
                              void *grad_sh, void *grad_positions, void *grad_opacity, void *grad_eye, bool cam) {
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
                launch_kernel(ctx, NO_STAGE, k_sh_colors_backward<deg.value, cam_.value>, dim3(div_up(n, 256)), dim3(256), eye3[0], eye3[1], eye3[2],
                              (const float4 *)positions, pos_stride_vec4, (const float *)sh, sh_stride_floats, (const float4 *)grad_color_opacity,
                              n, (float *)grad_sh, (float4 *)grad_positions, last);
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

extern "C" int splat_sh_colors_backward(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                                        uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, const void *grad_color_opacity,
                                        uint32_t n, void *grad_sh, void *grad_positions, void *grad_opacity) {
    return sh_colors_backward(ctx, eye3, positions, pos_stride_vec4, sh, sh_stride_floats, degree, opacity_f32, grad_color_opacity, n, grad_sh,
                              grad_positions, grad_opacity, nullptr, false);
}

extern "C" int splat_sh_colors_backward_camera(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                                               uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32,
                                               const void *grad_color_opacity, uint32_t n, void *grad_sh, void *grad_positions,
                                               void *grad_opacity, void *grad_eye) {
    return sh_colors_backward(ctx, eye3, positions, pos_stride_vec4, sh, sh_stride_floats, degree, opacity_f32, grad_color_opacity, n, grad_sh,
                              grad_positions, grad_opacity, grad_eye, true);
}
