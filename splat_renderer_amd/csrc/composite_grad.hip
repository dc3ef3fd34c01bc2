// composite_grad.hip — the per-tile kernels behind the gradients of a frame of anisotropic 3D Gaussians
// (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference counterpart): the composite's backward and the contribution scores.
// Both recompute each pixel's forward in binary32 in the operation order of the kernel that drew the frame
// (composite_uses_px: k_composite's, composite_quadrant.h, or k_composite_px's, composite_px.hip; this file is compiled with
// contraction on, as they are).  The per-splat kernels that take the record and colour gradients on to the parameters are
// splat_grad.hip.
//
// Shared by the two tile kernels, and with composite_features.hip's (composite_walk.h): the pixel mapping
// (TILE_PIXEL_PROLOGUE), the staged list (stage_chunk), an entry's alpha at a pixel (entry_alpha), the transmittance update
// and the weight w = T alpha (blend_step<PX>), and the entry points' frame arguments (FrameArgs).
//
// k_composite_backward<DEPTH, PX, DET, ABS>
//   Walk 1, front to back: L, the number of entries the pixel consumed (up to and including the one its early-out stopped
//   at), T_{L-1} and T_L.  Walk 2, back to front from the tile's largest L: per entry i < L a pixel recovers
//   T_i = T_{i+1} / (1 - alpha_i) (except at its last entry, whose T_{L-1} it kept: only there may 1 - alpha be <= 0.01) and
//   forms dL/dalpha_i = T_i (G.c_i - S_i), S the blend of everything behind the entry, with alpha as a fourth channel
//   (colour 1, background 0).  Each wave sums its 64 lanes' numbers per entry with DPP (skipped when the ballot says no lane
//   of the wave is inside the entry); the four waves' sums meet in LDS as (w0 + w1) + (w2 + w3), and after the chunk each
//   (entry, number) sum goes to its word of the outputs (the SUM_* constants).
//     flag   entry points                     adds                                                   argument struct
//     DEPTH  _depth, and _det / _abs /        the AOV depth D = sum w z / sum w: walk 1 sums ws and  BackDepthParams
//            _det_abs given depth arguments   zw, walk 2 carries D as a fifth channel of colour
//                                             z_i - D and upstream G_D / ws; number SUM_Z =
//                                             w_i G_D / ws.  z_i is staged in the entry's spare c.y
//     PX     (composite_uses_px)              the drawing kernel's update order, above               -
//     DET    _det, _det_abs                   no float atomics: the sums are stored to splat-major    BackDetParams
//                                             slots of the caller's workspace and a tile table row
//                                             {largest L, key and index of the last consumed entry};
//                                             k_det_rect_count, a scan and k_det_gather do the rest
//     ABS    _abs, _det_abs                   two more numbers after the others, |term c.x| and       BackAbsParams
//                                             |term c.y| (AbsGS's homodirectional gradient), on the
//                                             same path into grad_center_abs
//   Without DET the sums are float atomic adds: reproducible to rounding only.  With it they are the same bits on every run.
// k_det_rect_count, k_det_gather<DEPTH, ABS>
//   k_det_rect_count and the scan give every splat the first slot of its tile rectangle; a tile's slot is its row-major
//   position in it.  k_det_gather adds, per splat, the slots of the tiles that consumed it - lists ascend in (key, index), so
//   one compare with the tile's table row decides - each tile row left to right, the rows top to bottom, and the total once
//   into the splat's words: the order include/splat.h states.
// k_composite_contribution<PX>
//   Walk 1 alone, with every lane kept in the loop: per consumed entry inside the cut a pixel's blend weight times the pixel's
//   mask.  Per entry and wave a ballot counts the hits and two integer DPP trees give the largest weight (non-negative floats
//   order as their bit patterns) and the sum of the weights in fixed point; the four waves' partials meet in LDS, and after
//   the chunk at most one integer atomic per (entry, output) goes to global memory.  Integer max, sum and count do not depend
//   on the order of arrival: the same bits on every run.
#include "common.h"
#include "variant.h"
#include "tile_range.h"
#include "disc.h"
#include "composite.h"
#include "composite_walk.h"
#include "wave_reduce.h"

namespace {

// The numbers summed per (entry, pixel), in the order of an entry's row in LDS and of a det slot.  The optional ones come last,
// so that a number below GNV is the same one in every variant.
constexpr uint32_t SUM_CX = 0, SUM_CY = 1, SUM_B00 = 2, SUM_B01 = 3, SUM_B11 = 4; // -> grad_records
constexpr uint32_t SUM_R = 5, SUM_G = 6, SUM_B = 7, SUM_OPACITY = 8;               // -> grad_color_opacity
constexpr int GNV = 9;          // the numbers every variant sums
constexpr uint32_t SUM_Z = GNV; // (DEPTH) -> grad_depth
constexpr int GNABS = 2;        // (ABS) |term c.x|, |term c.y|, from grad_nv_base(DEPTH) -> grad_center_abs
// numbers per entry of a variant, and of it without the absolute sums (the index of |term c.x| where it has them)
constexpr int grad_nv_base(bool depth) { return depth ? GNV + 1 : GNV; }
constexpr int grad_nv(bool depth, bool abs) { return grad_nv_base(depth) + (abs ? GNABS : 0); }
// floats per splat of the output planes; a record row is {c.x, c.y, B00, B01, -, B11, -, -}
constexpr uint32_t REC_ROW = 8, REC_B11 = 5, COLOR_ROW = 4, ABS_ROW = 2;

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

// (file header: the walks and the flag table.  Each instantiation takes the prefix of BackAbsParams that it reads.)
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

    TILE_PIXEL_PROLOGUE(p);

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
                T_last = T;
                [[maybe_unused]] const float wgt = blend_step<PX>(s_ent[j], in, alpha, ge, T);
                if constexpr (DEPTH) {
                    zw += s_ent[j].c.y * wgt;
                    ws += wgt;
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
                vals[SUM_R] = wgt * G.x;
                vals[SUM_G] = wgt * G.y;
                vals[SUM_B] = wgt * G.z;
                vals[SUM_OPACITY] = ge * dA;
                if constexpr (DEPTH) vals[SUM_Z] = wgt * GDn;
                const float dd2 = -4.5f * alpha * dA;
                const float du = 2.0f * u * dd2, dv = 2.0f * v * dd2;
                vals[SUM_CX] = -du * e.a.z;               // d2 / c.x
                vals[SUM_CY] = -(du * e.a.w + dv * e.b.x); // d2 / c.y
                vals[SUM_B00] = du * dx;                   // d2 / B00
                vals[SUM_B01] = du * dy;                   // d2 / B01
                vals[SUM_B11] = dv * dy;                   // d2 / B11
                if constexpr (ABS) {
                    vals[NVB] = fabsf(vals[SUM_CX]);
                    vals[NVB + 1] = fabsf(vals[SUM_CY]);
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
            // one atomic add per touched (entry, number)
            for (uint32_t q = tid; q < m * NV; q += 256) {
                const uint32_t e = q / NV, k = q - e * NV;
                if (!s_touch[e]) continue;
                const float sum = (s_part[0][e][k] + s_part[1][e][k]) + (s_part[2][e][k] + s_part[3][e][k]);
                const size_t idx = s_idx[e];
                float *dst = k < SUM_R ? p.grad_records + idx * REC_ROW + (k < SUM_B11 ? k : REC_B11) : p.grad_color + idx * COLOR_ROW + (k - SUM_R);
                if constexpr (DEPTH) dst = k == SUM_Z ? p.grad_depth + idx : dst;
                if constexpr (ABS) dst = k >= (uint32_t)NVB ? p.grad_abs + idx * ABS_ROW + (k - NVB) : dst;
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

    TILE_PIXEL_PROLOGUE(p);
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
                    const float wgt = blend_step<PX>(s_ent[j], in, alpha, ge, T);
                    live = !(T <= T_STOP); // (this entry, the one the pixel stops at, is still consumed)
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
    // (the atomic path's word of number k, with k a constant)
    float *grec = p.grad_records + (size_t)i * REC_ROW, *gcol = p.grad_color + (size_t)i * COLOR_ROW;
#pragma unroll
    for (uint32_t k = SUM_CX; k < SUM_R; ++k) grec[k < SUM_B11 ? k : REC_B11] += total[k];
#pragma unroll
    for (uint32_t k = SUM_R; k < (uint32_t)GNV; ++k) gcol[k - SUM_R] += total[k];
    if constexpr (DEPTH) p.grad_depth[i] += total[SUM_Z];
    if constexpr (ABS) {
        float *gabs = p.grad_abs + (size_t)i * ABS_ROW;
#pragma unroll
        for (int k = 0; k < GNABS; ++k) gabs[k] += total[grad_nv_base(DEPTH) + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  The argument structs carry the names of include/splat.h's arguments, because the argument checks quote them; a
// field an entry point does not have stays NULL / 0.

namespace {

// splat_composite_backward_det's further arguments
struct DetArgs {
    const void *projected;
    uint64_t total_pairs;
    void *workspace;
    uint64_t workspace_bytes;
};

// The workspace of splat_composite_backward_det: the tile table (16 bytes per tile), slot_base (4 bytes per splat, rounded up
// to 16) and the slots (4 NV bytes per pair, NV = 9, or 10 with depth; the _abs entry points: 11, or 12).  0 where it would
// not fit 64 bits (judged by the largest slot of the family: 40 bytes, 48 with the absolute sums).
static uint64_t det_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, bool depth, bool abs, uint64_t *slot_base_off = nullptr,
                                    uint64_t *slots_off = nullptr) {
    const uint64_t table = (uint64_t)num_tiles * 16u, base = ((uint64_t)n * 4u + 15u) & ~15ull;
    if (slot_base_off) *slot_base_off = table;
    if (slots_off) *slots_off = table + base;
    if (total_pairs > (~0ull - table - base) / (4u * (uint64_t)grad_nv(true, abs))) return 0;
    return table + base + total_pairs * 4u * (uint64_t)grad_nv(depth, abs);
}

// The five composite backwards: their checks, the kernel's parameters and the launches.  depth: the depth variant, with its four
// arguments; det: the fixed-order entry points' arguments, or NULL for the atomic ones; abs: the _abs entry points, with
// grad_center_abs (n x 2 floats, 8-byte aligned, ADDED into).
struct BackwardArgs : FrameArgs {
    const void *grad_rgba32f, *depth_f32, *grad_depth_f32;
    void *grad_records, *grad_color_opacity, *grad_depth, *grad_center_abs;
    uint32_t depth_stride_floats;
    const DetArgs *det;
    bool depth, abs;

    // the _det and _abs entry points' convention: colour only when the four depth arguments are all NULL / 0; any of them given
    // asks for the depth variant, with its checks
    bool any_depth_argument() const { return depth_f32 || depth_stride_floats || grad_depth_f32 || grad_depth; }

    // The fixed-order launches over det's workspace: slot_base (the scan of the rectangles' tile counts), the tile kernel
    // storing its sums to the slots, the gather
    int launch_det(splat_ctx *ctx, BackAbsParams &p, uint32_t nty, uint64_t slot_base_off, uint64_t slots_off) const {
        const uint32_t ntx = p.ntx;
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

    int launch(splat_ctx *ctx) const {
        BackAbsParams p{}; // (every kernel takes the base of it that it reads; what a launch does not set is zero)
        uint32_t nty = 0;
        const int rc_setup = setup(ctx, "splat_composite_backward", p, nty);
        if (rc_setup != SPLAT_OK) return rc_setup;
        const uint32_t ntx = p.ntx;
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
            const uint64_t need = det_workspace_bytes(det->total_pairs, ntx * nty, n, depth, abs, &slot_base_off, &slots_off);
            ARG_CHECK(ctx, det->workspace && ((uintptr_t)det->workspace & 15) == 0 && need != 0 && det->workspace_bytes >= need);
        }
        if (n == 0) return SPLAT_OK; // (no splat: every list is empty)
        p.grad_img = (const float4 *)grad_rgba32f;
        p.grad_records = (float *)grad_records;
        p.grad_color = (float *)grad_color_opacity;
        p.z = (const float *)depth_f32;
        p.z_stride = depth_stride_floats;
        p.grad_depth_img = (const float *)grad_depth_f32;
        p.grad_depth = (float *)grad_depth;
        p.grad_abs = (float *)grad_center_abs;
        if (det) return launch_det(ctx, p, nty, slot_base_off, slots_off);
        // (<DEPTH, PX, ABS>: the kernel without DEPTH or ABS takes the BackParams part of p)
        variant_dispatch([&](auto d, auto px, auto ab) {
            launch_kernel(ctx, NO_STAGE, k_composite_backward<d.value, px.value, false, ab.value>, dim3(ntx, nty), dim3(256), p);
        }, depth, composite_uses_px(ctx, ntx, nty), abs);
        return launch_check(ctx, depth ? "launch k_composite_backward<DEPTH>" : "launch k_composite_backward");
    }
};

// splat_composite_contribution: the frame, the pixel mask (NULL: 1 everywhere) and the three per-splat outputs (each NULL: not wanted)
struct ContributionArgs : FrameArgs {
    const void *pixel_weight_f32;
    float min_weight;
    void *hits_u32, *weight_max_f32, *weight_sum_u64;

    int launch(splat_ctx *ctx) const {
        ContribParams p{};
        uint32_t nty = 0;
        const int rc_setup = setup(ctx, "splat_composite_contribution", p, nty);
        if (rc_setup != SPLAT_OK) return rc_setup;
        ARG_CHECK(ctx, min_weight >= 0.0f); // (NaN fails it)
        ARG_CHECK(ctx, color_opacity && records && tile_indices && tile_counts && tile_offsets);
        ARG_CHECK(ctx, hits_u32 || weight_max_f32 || weight_sum_u64);
        ARG_CHECK(ctx, (((uintptr_t)color_opacity | (uintptr_t)records) & 15) == 0 && ((uintptr_t)weight_sum_u64 & 7) == 0);
        ARG_CHECK(ctx, (((uintptr_t)tile_indices | (uintptr_t)tile_counts | (uintptr_t)tile_offsets | (uintptr_t)pixel_weight_f32 |
                         (uintptr_t)hits_u32 | (uintptr_t)weight_max_f32) & 3) == 0);
        if (n == 0) return SPLAT_OK; // (no splat: every list is empty)
        p.pixel_weight = (const float *)pixel_weight_f32;
        p.min_weight = min_weight;
        p.hits = (uint32_t *)hits_u32;
        p.weight_max = (uint32_t *)weight_max_f32;
        p.weight_sum = (unsigned long long *)weight_sum_u64;
        variant_dispatch([&](auto px) { launch_kernel(ctx, NO_STAGE, k_composite_contribution<px.value>, dim3(p.ntx, nty), dim3(256), p); },
                         composite_uses_px(ctx, p.ntx, nty));
        return launch_check(ctx, "launch k_composite_contribution");
    }
};

} // namespace

extern "C" uint64_t splat_composite_backward_det_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth) {
    return det_workspace_bytes(total_pairs, num_tiles, n, with_depth != 0, false);
}

extern "C" uint64_t splat_composite_backward_det_abs_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth) {
    return det_workspace_bytes(total_pairs, num_tiles, n, with_depth != 0, true);
}

// ... the image's gradient and the two gradient planes of every backward, and the four depth arguments of all but the first
#define BACKWARD_ARGS(a) FRAME_ARGS(a), a.grad_rgba32f = grad_rgba32f, a.grad_records = grad_records, a.grad_color_opacity = grad_color_opacity
#define DEPTH_ARGS(a)                                                                                                          \
    a.depth_f32 = depth_f32, a.depth_stride_floats = depth_stride_floats, a.grad_depth_f32 = grad_depth_f32, a.grad_depth = grad_depth

extern "C" int splat_composite_backward(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                        const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                        uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                        void *grad_color_opacity) {
    if (ctx && cfg && cfg->footprint == SPLAT_FOOTPRINT_SURFEL) { // (surfel.hip: the whole record's alpha and gradient)
        SurfelBackwardCall a{};
        BACKWARD_ARGS(a);
        return surfel_composite_backward(ctx, a);
    }
    BackwardArgs a{};
    BACKWARD_ARGS(a);
    return a.launch(ctx);
}

extern "C" int splat_composite_backward_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                              uint32_t color_stride_vec4, const void *records, const void *tile_indices, const void *tile_counts,
                                              const void *tile_offsets, uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n,
                                              void *grad_records, void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                              const void *grad_depth_f32, void *grad_depth) {
    if (ctx && cfg && cfg->footprint == SPLAT_FOOTPRINT_SURFEL) {
        SurfelBackwardCall a{};
        BACKWARD_ARGS(a), DEPTH_ARGS(a);
        a.depth = true;
        return surfel_composite_backward(ctx, a);
    }
    BackwardArgs a{};
    BACKWARD_ARGS(a), DEPTH_ARGS(a);
    a.depth = true;
    return a.launch(ctx);
}

extern "C" int splat_composite_backward_det(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                            uint32_t color_stride_vec4, const void *records, const void *projected, const void *tile_indices,
                                            const void *tile_counts, const void *tile_offsets, uint64_t total_pairs, uint32_t width,
                                            uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records, void *grad_color_opacity,
                                            const void *depth_f32, uint32_t depth_stride_floats, const void *grad_depth_f32, void *grad_depth,
                                            void *workspace, uint64_t workspace_bytes) {
    DetArgs det{};
    det.projected = projected, det.total_pairs = total_pairs, det.workspace = workspace, det.workspace_bytes = workspace_bytes;
    BackwardArgs a{};
    BACKWARD_ARGS(a), DEPTH_ARGS(a);
    a.depth = a.any_depth_argument();
    a.det = &det;
    return a.launch(ctx);
}

extern "C" int splat_composite_backward_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                            const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                            uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                            void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                            const void *grad_depth_f32, void *grad_depth, void *grad_center_abs) {
    BackwardArgs a{};
    BACKWARD_ARGS(a), DEPTH_ARGS(a);
    a.depth = a.any_depth_argument();
    a.abs = true, a.grad_center_abs = grad_center_abs;
    return a.launch(ctx);
}

extern "C" int splat_composite_backward_det_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                                uint32_t color_stride_vec4, const void *records, const void *projected, const void *tile_indices,
                                                const void *tile_counts, const void *tile_offsets, uint64_t total_pairs, uint32_t width,
                                                uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                                void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                                const void *grad_depth_f32, void *grad_depth, void *workspace, uint64_t workspace_bytes,
                                                void *grad_center_abs) {
    DetArgs det{};
    det.projected = projected, det.total_pairs = total_pairs, det.workspace = workspace, det.workspace_bytes = workspace_bytes;
    BackwardArgs a{};
    BACKWARD_ARGS(a), DEPTH_ARGS(a);
    a.depth = a.any_depth_argument();
    a.det = &det;
    a.abs = true, a.grad_center_abs = grad_center_abs;
    return a.launch(ctx);
}

extern "C" int splat_composite_contribution(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                            const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                            uint32_t width, uint32_t height, const void *pixel_weight_f32, float min_weight, uint32_t n,
                                            void *hits_u32, void *weight_max_f32, void *weight_sum_u64) {
    ContributionArgs a{};
    FRAME_ARGS(a);
    a.pixel_weight_f32 = pixel_weight_f32, a.min_weight = min_weight;
    a.hits_u32 = hits_u32, a.weight_max_f32 = weight_max_f32, a.weight_sum_u64 = weight_sum_u64;
    return a.launch(ctx);
}

