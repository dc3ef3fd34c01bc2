// composite.h — what the composite translation units share: the launch parameters, the per-entry fetch, the exact
// coverage masks and the stop rule.  composite.hip holds the entry points, the argument checks and the choice of kernel,
// with k_composite (16x16 tiles, a wave per 8x8 quadrant); composite_px.hip holds k_composite_px (16x16 tiles, a lane per
// 2x2 pixels) and its per-band history; composite_tile.hip holds k_composite_tile, the composite for every other tile size.
// k_composite and k_composite_tile are one body: composite_quadrant.h.
#pragma once
#include "common.h"
#include "disc.h"
#include "shade.h"
#include "variant.h"

typedef float v2f __attribute__((ext_vector_type(2))); // maps onto the packed FP32 instructions (v_pk_*_f32)

constexpr int CT = 16;        // tile edge (pixels)
constexpr int CBATCH = 256;   // list entries staged per round

struct CompositeParams {
    const float4 *color;  uint32_t color_stride;   // vec4(rgb, opacity)
    const float4 *normals; uint32_t normal_stride; // vec4(normal, scaleFactor)
    const float4 *projected;                       // 2 x float4 per splat (ProjectedSplat), or 1 x float4 (compact exchange record)
    uint32_t compact;
    uint32_t lit32;                                // projected holds lit composite records (shade.h): colour and normals are not read
    uint32_t disc;                                 // projected holds disc records (disc.h): the oriented-disc footprint
    uint32_t disc_stride;                          // float4s between disc records: 2 (projector's) or 3 (48-byte exchange records, lit disc records)
    uint32_t disc_lit;                             // the third float4 of a disc record is the splat's lit colour: colour and normals are not read
    uint32_t prelit;                               // color holds lit colours (k_lit_colors): normals are not read
    const uint32_t *indices, *counts, *offsets;
    uint32_t width, height, ntx, tile_row0;
    uint32_t *out_rgba8;
    float4 *out_rgba32f;
    unsigned long long *consumed; // per tile {entries staged, entries consumed}, accumulated (or NULL)
    // the frame's report (tile-first frames; NULL otherwise): this launch is the frame's last kernel, so its first
    // workgroup tells the host {pair total, flags incl. the per-tile sort's order check, sequence number}
    const uint32_t *frame_total;
    uint32_t *report;
    uint32_t report_seq;
    const uint32_t *tile_order; // k_composite_px: workgroup b works on tile tile_order[b] of the band (NULL: b)
    uint32_t *tile_cost;        // k_composite_px: chunks each tile's consumer walked (NULL: not kept)
    const uint32_t *order_src;  // k_composite_px, workgroup 0: the costs the PREVIOUS launch over this band left (NULL: none) ...
    uint32_t *order_dst;        // ... sorted into the order the NEXT launch takes its tiles in
    const uint32_t *cost_prev;  // k_composite_px: the same costs, read by every tile: how many chunks to build and gather ahead of need (NULL: all)
#ifdef PX_PROFILE
    uint32_t debug_cap;         // (measuring build only, SPLAT_PX_CAP: every list cut after this many entries — a WRONG image: what do the long tiles cost?)
#endif
    // auxiliary outputs (splat_aov; read only by the AOV instantiations, which write each non-NULL one per rendered pixel)
    float *aov_depth;
    float *aov_alpha;
    uint32_t *aov_id;
    const float *aov_z;         // the depth of splat i is aov_z[i * aov_zstride] (NULL: the records carry none; depth not asked for)
    uint32_t aov_zstride;
};

// Per pixel of a one-pixel-per-lane composite (k_composite, k_composite_tile): what the auxiliary outputs need beside the
// colour — sum w z, sum w, and the largest w with its splat index (strictly larger: on equal weights the earlier, nearer
// entry keeps the pixel).  w is the colour's own T g, after the coverage / stop masking.
struct AovPixel {
    float zw = 0.0f, ws = 0.0f, wmax = 0.0f;
    uint32_t id = 0xffffffffu;
    __device__ __forceinline__ void add(float w, float2 zi) {
        zw += zi.x * w;
        ws += w;
        const bool top = w > wmax;
        wmax = top ? w : wmax;
        id = top ? __float_as_uint(zi.y) : id;
    }
    // alpha = 1 - T_end; depth = sum w z / sum w (+inf where nothing contributed); id 0xffffffff where nothing did
    __device__ __forceinline__ void store(const CompositeParams &p, size_t o, float T_end) const {
        if (p.aov_alpha) p.aov_alpha[o] = 1.0f - T_end;
        if (p.aov_depth) p.aov_depth[o] = ws > 0.0f ? zw / ws : __builtin_inff();
        if (p.aov_id) p.aov_id[o] = id;
    }
};

// {depth, splat index (as bits)} of a staged entry for the AOV instantiations (idx = 0xffffffff: no entry)
__device__ __forceinline__ float2 aov_entry(const CompositeParams &p, uint32_t idx) {
    if (idx == 0xffffffffu) return make_float2(0.0f, __uint_as_float(0xffffffffu));
    const float z = p.aov_z ? p.aov_z[(size_t)idx * p.aov_zstride] : 0.0f;
    return make_float2(z, __uint_as_float(idx));
}

__device__ __forceinline__ uint32_t unorm8(float v) {
    v = fminf(fmaxf(v, 0.0f), 1.0f); // fmaxf(NaN,0) = 0
    return (uint32_t)(v * 255.0f + 0.5f);
}

// 64-bit lane mask of one 8x8 quadrant from its 8-bit column mask xb and row mask yb: lane
// ly*8+lx is set iff bit lx of xb and bit ly of yb are.  (y & 15) * 0x00204081 drops bit i of y at
// bit 8i (the four shifted copies do not overlap), & 0x01010101 keeps those, * xb copies xb into
// every selected byte.
__device__ __forceinline__ uint2 quadrant_mask(uint32_t xb, uint32_t yb) {
    const uint32_t lo = (((yb & 15u) * 0x00204081u) & 0x01010101u) * xb;
    const uint32_t hi = (((yb >> 4) * 0x00204081u) & 0x01010101u) * xb;
    return make_uint2(lo, hi);
}

// Pixel columns j in [0,16) of a tile whose centres c0 + j lie inside [lo, hi]
// (ComputeShaderRenderer.ts:118-121 keeps a pixel iff !(p < min || p > max)).  c0 = tile origin +
// 0.5 >= 0.5.  For a result in [0,16) the subtraction is exact (lo >= c0 > 0 and the difference is a
// multiple of ulp(lo) no larger than lo), outside that range only its sign / being >= 16 matters
// and rounding is monotone (x - y == 0 only when x == y), so the mask is exactly the set the
// reference's comparisons select.
__device__ __forceinline__ uint32_t span_mask16(float lo, float hi, float c0) {
    const float a = fmaxf(ceilf(lo - c0), 0.0f), b = fminf(floorf(hi - c0), 15.0f);
    if (!(a <= b)) return 0u; // also NaN
    const uint32_t ia = (uint32_t)a, ib = (uint32_t)b;
    return ((2u << ib) - 1u) & ~((1u << ia) - 1u);
}

// Pins a wave-uniform 64-bit value into scalar registers (the compiler's divergence analysis gives
// up on loop-carried masks and would otherwise keep them, and every test on them, in VGPRs).
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// bounds and screen radius of splat idx.  Compact exchange records (multi-GPU frame) carry {centre x,
// y, radius, depth}: the bounds are rebuilt exactly as the projector forms them (SplatProjector.ts:
// 119-121) — with contraction switched off for this function (the file is compiled with it on).
__device__ __forceinline__ void fetch_record(const CompositeParams &p, uint32_t idx, float4 &bounds, float &radius) {
    if (p.compact) {
        const float4 c = p.projected[idx];
        bounds = lit_bounds(c); // the bounds must be the projector's: one rounding per operation
        radius = c.z;
    } else {
        bounds = p.projected[(size_t)idx * 2];
        radius = reinterpret_cast<const float *>(p.projected)[(size_t)idx * 8 + 5];
    }
}

// The stop test of the nearest-first loop is (1 - T) >= 0.99 on the transmittance T (the reference's alpha >= 0.99,
// ComputeShaderRenderer.ts:187-190).  A correctly rounded 1 - T is monotone in T, so the test is EXACTLY T <= the
// largest binary32 T that passes it — 0x1.47ae4p-7 (found by stepping ulps; NaN fails both forms) — and the
// subtraction leaves the per-pixel loop.
constexpr float T_STOP = 0x1.47ae4p-7f;
static_assert((1.0f - T_STOP) >= 0.99f && !((1.0f - 0x1.47ae42p-7f) >= 0.99f), "T_STOP is the last transmittance that stops a pixel");

// exp(-0.5 * d2 / (0.4 * 0.4)) = exp2(d2 * this)   (SequentialRenderer.ts:132-133)
constexpr float DISC_EXP2_SCALE = -4.508422002777011f;
// exp(-4.5 d2) = exp2(d2 * this), d2 = u^2 + v^2 = d^T Sigma2^-1 d / 9 of an ellipsoid record (ellipsoid.h): exp(-0.5 d^T Sigma2^-1 d)
constexpr float ELLIPSOID_EXP2_SCALE = -6.492127684000335f;
// The exponent scale is a property of the footprint; the disc-record kernels take it at compile time (ELL: the ellipsoid's)
template <bool ELL> struct FootprintExp2 { static constexpr float scale = ELL ? ELLIPSOID_EXP2_SCALE : DISC_EXP2_SCALE; };
// The footprints whose records the ELL instantiations draw: the ellipsoid's (q = 0) and the surfel's (surfel.h: full disc
// records with the ellipsoid's exponent scale and alpha = opacity g; the forward kernels evaluate B10 and q of every record)
inline bool footprint_is_ell(uint32_t footprint) { return footprint == SPLAT_FOOTPRINT_ELLIPSOID || footprint == SPLAT_FOOTPRINT_SURFEL; }

// DISC: the footprint is SequentialRenderer's oriented disc (disc.h) — per entry the 32-byte disc record and
// the lit colour are staged, a pixel is inside when u^2 + v^2 <= 1 with (u,v) = B*d / (1 - q.d); the
// coverage masks come from the disc's exact bounds, as the binner's tile ranges do.
// LIT32: `projected` holds the frame's lit composite records (shade.h) — ONE 32-byte gather per staged entry gives
// centre, radius and lit colour; colour and normal arrays are not touched.
// ELL: the ellipsoid's records — the colour's fourth word must be its opacity (lit records carry the depth there: it is read
// from the colour plane)
template <int MODE, bool EARLY_OUT, bool DISC, bool LIT32, bool ELL = false>
__device__ __forceinline__ void fetch_entry(const CompositeParams &p, uint32_t idx, float4 &f_b, float4 &f_b2, float4 &f_c, float4 &f_n,
                                            float &f_r) {
    if constexpr (DISC) {
        f_b = p.projected[(size_t)idx * p.disc_stride];
        f_b2 = p.projected[(size_t)idx * p.disc_stride + 1];
        if (p.disc_lit) {
            f_c = p.projected[(size_t)idx * p.disc_stride + 2];
            if (ELL) f_c.w = p.color[(size_t)idx * p.color_stride].w;
            return;
        }
    } else if constexpr (LIT32) {
        const float4 c = p.projected[(size_t)idx * 2];
        f_c = p.projected[(size_t)idx * 2 + 1];
        f_b = lit_bounds(c);
        f_r = c.z;
        return;
    } else {
        fetch_record(p, idx, f_b, f_r);
    }
    f_c = p.color[(size_t)idx * p.color_stride];
    if (!p.prelit) f_n = p.normals[(size_t)idx * p.normal_stride];
}

// Which instantiations of k_composite and k_composite_tile <MODE, EARLY_OUT, DISC, LIT32, AOV, ELL> exist (EARLY_OUT: both):
// the reference-literal blend is the isotropic footprint's alone and has no auxiliary outputs (aov_check and
// composite_launch's argument checks refuse the rest); a disc record's lit colour is found at run time (p.disc_lit), not
// by LIT32; the ellipsoid's records are disc records.
constexpr bool composite_variant_exists(int mode, bool disc, bool lit32, bool aov, bool ell) {
    return (mode == SPLAT_COMPOSITE_FRONT_TO_BACK || !(aov || disc)) && !(disc && lit32) && (disc || !ell);
}

// Which instantiations of k_composite_px <EARLY_OUT, LIT32, COUNT, AH, DISC, AOV, ELL> exist (EARLY_OUT, COUNT, AH, AOV: all):
// nearest on top is its only blend; a disc record's lit colour is found at run time (p.disc_lit), not by LIT32; the
// ellipsoid's records are disc records.
constexpr bool composite_px_variant_exists(bool disc, bool lit32, bool ell) { return !(disc && lit32) && (disc || !ell); }

// The two launchers composite_launch chooses between before k_composite: p is filled in by composite_launch, `band` is the
// screen's tiles of cfg->tile_size pixels and the rows of them to render.  *launched: whether the launch that carries the
// frame's report went out.
// composite_tile.hip: tile sizes other than CT.
int composite_tile_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, const CompositeParams &p, const TileBand &band, bool *launched);
// composite_px.hip: 16x16 tiles, nearest on top, where composite_uses_px says so (the launcher sets p's hints from the band's history).
int composite_px_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, CompositeParams &p, const TileBand &band, bool *launched);
