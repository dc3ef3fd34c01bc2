// composite.hip — the per-pixel alpha composite (ComputeShaderRenderer / TileRenderer front end): the public entry points,
// the argument checks and the choice of kernel.
//
// Three kernels composite a frame, one per call (composite_launch):
//   - k_composite_tile (composite_tile.hip): every tile size but 16;
//   - k_composite_px (composite_px.hip): 16x16 tiles, nearest on top, on screens of many tiles — a lane per 2x2 pixels;
//   - k_composite (here): 16x16 tiles otherwise, and every reference-literal frame — a wave per 8x8 quadrant.  Its body is
//     composite_quadrant.h's, shared with k_composite_tile; the design is described there.
//
// Compiled with -ffp-contract=on; compared with the oracle within a stated tolerance.
#include "composite_quadrant.h"

// The lit colours of all splats as a plane: when the composite is given this plane (cfg->prelit) it
// gathers two lines per staged entry (record, lit colour) instead of three (record, colour, normal) —
// the gathers, not the arithmetic, are what a staged entry costs (108 -> 93 us at C2 for one line less).
__global__ __launch_bounds__(256) void k_lit_colors(const float4 *__restrict__ color, uint32_t color_stride,
                                                    const float4 *__restrict__ normals, uint32_t normal_stride, uint32_t n,
                                                    float4 *__restrict__ lit) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) lit[i] = lit_color(color[(size_t)i * color_stride], normals[(size_t)i * normal_stride]);
}

template <int MODE, bool EARLY_OUT, bool DISC, bool LIT32, bool AOV = false, bool ELL = false>
__global__ __launch_bounds__(256) void k_composite(CompositeParams p) {
    // workgroup = tile (blockIdx.x, blockIdx.y) of the band: the window is the tile
    composite_window<false, MODE, EARLY_OUT, DISC, LIT32, AOV, ELL>(p, {blockIdx.x, blockIdx.y + p.tile_row0});
}

int aov_check(splat_ctx *ctx, const splat_composite_cfg *cfg, const splat_aov *aov, bool has_depth) {
    if (!aov) return SPLAT_OK;
    ARG_CHECK(ctx, aov->depth_f32 || aov->alpha_f32 || aov->id_u32);
    ARG_CHECK(ctx, (((uintptr_t)aov->depth_f32 | (uintptr_t)aov->alpha_f32 | (uintptr_t)aov->id_u32) & 15) == 0);
    if (cfg->mode != SPLAT_COMPOSITE_FRONT_TO_BACK)
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_aov: the reference-literal blend has no auxiliary outputs (an entry's final weight is "
                                                "not known until its list ends)");
    if (aov->depth_f32 && !has_depth)
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_aov: depth asked for, but the records composited carry no splat depth (32-byte disc "
                                                "records: composite from SPLAT_RECORDS_DISC48, or render the frame with `projected` or lit records)");
    return SPLAT_OK;
}

extern "C" int splat_lit_colors(splat_ctx *ctx, const void *color_opacity, uint32_t color_stride_vec4, const void *normals,
                                uint32_t normal_stride_vec4, uint32_t n, void *lit) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, n == 0 || (color_opacity && normals && lit));
    ARG_CHECK(ctx, color_stride_vec4 >= 1 && normal_stride_vec4 >= 1);
    ARG_CHECK(ctx, (((uintptr_t)color_opacity | (uintptr_t)normals | (uintptr_t)lit) & 15) == 0);
    if (n == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_lit_colors, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const float4 *)color_opacity, color_stride_vec4,
                       (const float4 *)normals, normal_stride_vec4, n, (float4 *)lit);
    LAUNCH_CHECK(ctx, "k_lit_colors");
    return SPLAT_OK;
}

__global__ void k_frame_report(const uint32_t *frame_total, uint32_t *report, uint32_t seq) { tile_report(frame_total, report, seq); }

extern "C" int splat_composite(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                               uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                               const void *projected, const void *tile_indices, const void *tile_counts,
                               const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8, void *out_rgba32f,
                               void *consumed_dptr) {
    return splat_composite_aov(ctx, cfg, color_opacity, color_stride_vec4, normals, normal_stride_vec4, projected, tile_indices, tile_counts,
                               tile_offsets, width, height, out_rgba8, out_rgba32f, consumed_dptr, nullptr);
}

// lit DISC records (48 bytes: the lit colour behind each disc record) exist only inside a frame's binner; a public caller's
// disc records are the projector's 32-byte ones (splat_project_disc) or 48-byte exchange records (taken at its
// word this pair would read idx * 48 out of an n * 32 allocation)
static bool lit_disc_records(const splat_composite_cfg *cfg) {
    return cfg && (cfg->footprint == SPLAT_FOOTPRINT_DISC || footprint_is_ell(cfg->footprint)) &&
           cfg->record_format == SPLAT_RECORDS_LIT32;
}

// the fields the public composite entry points share, under the names of include/splat.h's arguments
static CompositeArgs composite_public_args(const void *color_opacity, uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                                           const void *projected, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                           uint32_t width, uint32_t height, void *out_rgba8, void *out_rgba32f, void *consumed_dptr,
                                           const splat_aov *aov) {
    CompositeArgs a;
    a.color_opacity = color_opacity, a.color_stride_vec4 = color_stride_vec4;
    a.normals = normals, a.normal_stride_vec4 = normal_stride_vec4;
    a.projected = projected;
    a.tile_indices = tile_indices, a.tile_counts = tile_counts, a.tile_offsets = tile_offsets;
    a.width = width, a.height = height;
    a.out_rgba8 = out_rgba8, a.out_rgba32f = out_rgba32f;
    a.consumed = consumed_dptr;
    a.aov = aov;
    return a;
}

extern "C" int splat_composite_aov(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                   uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                                   const void *projected, const void *tile_indices, const void *tile_counts,
                                   const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8, void *out_rgba32f,
                                   void *consumed_dptr, const splat_aov *aov) {
    if (ctx && lit_disc_records(cfg))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_composite: the oriented-disc footprint composites from SPLAT_RECORDS_PROJECTED (32-byte disc "
                                                "records) or SPLAT_RECORDS_DISC48; lit disc records are internal to splat_render_frame");
    return composite_launch(ctx, cfg, composite_public_args(color_opacity, color_stride_vec4, normals, normal_stride_vec4, projected, tile_indices,
                                                            tile_counts, tile_offsets, width, height, out_rgba8, out_rgba32f, consumed_dptr, aov));
}

// splat_composite_aov with the AOV depth of splat i read from depth_f32[i * depth_stride_floats], for every footprint and record
// format splat_composite_aov takes (the caller's own z; the records need not carry one)
extern "C" int splat_composite_aov_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                         uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                                         const void *projected, const void *tile_indices, const void *tile_counts,
                                         const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8, void *out_rgba32f,
                                         void *consumed_dptr, const splat_aov *aov, const void *depth_f32, uint32_t depth_stride_floats) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, depth_f32 != nullptr && depth_stride_floats >= 1 && ((uintptr_t)depth_f32 & 3) == 0);
    if (lit_disc_records(cfg))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_composite_aov_depth: the oriented-disc footprint composites from SPLAT_RECORDS_PROJECTED "
                                                "(32-byte disc records) or SPLAT_RECORDS_DISC48; lit disc records are internal to splat_render_frame");
    CompositeArgs a = composite_public_args(color_opacity, color_stride_vec4, normals, normal_stride_vec4, projected, tile_indices, tile_counts,
                                            tile_offsets, width, height, out_rgba8, out_rgba32f, consumed_dptr, aov);
    a.ext_z = (const float *)depth_f32, a.ext_zstride = depth_stride_floats;
    return composite_launch(ctx, cfg, a);
}

// The composite with the frame's report attached.  Whatever happens to the launch — an empty band of tile rows, a rejected
// argument, a launch that did not go out — a report that was promised is sent (the host waits for it at its next call): on
// its own, when this function is left without a composite kernel carrying it.
int composite_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, const CompositeArgs &a) {
    struct Promise {
        splat_ctx *ctx;
        const CompositeArgs &a;
        bool launched = false;
        ~Promise() {
            if (!ctx || !a.report || launched) return;
            hipLaunchKernelGGL(k_frame_report, dim3(1), dim3(1), 0, ctx->stream, a.frame_total, a.report, a.report_seq);
            (void)hipGetLastError();
        }
    } report{ctx, a};
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, cfg != nullptr);
    const uint32_t T = cfg->tile_size, width = a.width, height = a.height;
    ARG_CHECK(ctx, T >= 1 && T <= 4096);
    ARG_CHECK(ctx, cfg->mode == SPLAT_COMPOSITE_FRONT_TO_BACK || cfg->mode == SPLAT_COMPOSITE_REFERENCE_LITERAL);
    ARG_CHECK(ctx, cfg->record_format <= SPLAT_RECORDS_LIT32);
    ARG_CHECK(ctx, width >= 1 && height >= 1);
    // (k_composite_tile's grid: ceil(T / 16)^2 windows of 16x16 pixels per tile, up to 65535 in x and in y)
    ARG_CHECK(ctx, T == CT ? (width <= 65535u * CT && height <= 65535u * CT)
                           : (div_up64(width, T) * div_up(T, CT) <= 65535u && div_up64(height, T) * div_up(T, CT) <= 65535u));
    // the records carry the lit colour (isotropic: 32-byte lit composite records; disc: the colour behind each disc record): no colour / normal arrays
    const bool lit32 = cfg->record_format == SPLAT_RECORDS_LIT32;
    ARG_CHECK(ctx, lit32 || (a.color_opacity && (a.normals || cfg->prelit)));
    ARG_CHECK(ctx, a.projected && a.tile_indices && a.tile_counts && a.tile_offsets);
    ARG_CHECK(ctx, a.color_stride_vec4 >= 1 && a.normal_stride_vec4 >= 1);
    ARG_CHECK(ctx, a.out_rgba8 || a.out_rgba32f);
    ARG_CHECK(ctx, (((uintptr_t)a.color_opacity | (uintptr_t)a.normals | (uintptr_t)a.projected | (uintptr_t)a.out_rgba32f) & 15) == 0);
    ARG_CHECK(ctx, cfg->prelit <= 1 && cfg->footprint <= SPLAT_FOOTPRINT_SURFEL);
    // the oriented disc is SequentialRenderer's footprint: nearest-on-top "over" is its only blend, and its
    // records are the projector's 32-byte disc records.  The ellipsoid's records are disc records (ellipsoid.h) under the
    // same rules, and have no 48-byte exchange form: no band frame exists for them
    ARG_CHECK(ctx, cfg->footprint == SPLAT_FOOTPRINT_ISOTROPIC ||
                       (cfg->mode == SPLAT_COMPOSITE_FRONT_TO_BACK && cfg->record_format != SPLAT_RECORDS_COMPACT));
    ARG_CHECK(ctx, cfg->record_format != SPLAT_RECORDS_DISC48 || cfg->footprint == SPLAT_FOOTPRINT_DISC);
    ARG_CHECK(ctx, !a.ext_z || (a.ext_zstride >= 1 && ((uintptr_t)a.ext_z & 3) == 0));
    // where the auxiliary outputs' depth comes from: float `off` of every record, `stride` floats apart — the ProjectedSplat's
    // depth (SplatProjector.ts:77), which the compact, lit and 48-byte disc records carry as well; the projector's 32-byte
    // disc records carry none (a frame hands its ProjectedSplat records' depth words in as ext_z when it writes them).  A
    // caller's ext_z (splat_composite_aov_depth, a frame's ProjectedSplat depths) is read in place of the records' own.
    const bool is_disc = cfg->footprint != SPLAT_FOOTPRINT_ISOTROPIC;
    const float *zsrc = nullptr;
    uint32_t zoff = 0, zstride = 0;
    if (a.ext_z) {
        zsrc = a.ext_z;
        zstride = a.ext_zstride;
    } else if (!is_disc) {
        zsrc = (const float *)a.projected;
        zoff = cfg->record_format == SPLAT_RECORDS_PROJECTED ? 4u : 3u;
        zstride = cfg->record_format == SPLAT_RECORDS_COMPACT ? 4u : 8u;
    } else if (cfg->record_format == SPLAT_RECORDS_DISC48 || lit32) {
        zsrc = (const float *)a.projected; // {disc record, depth, -, -, -} / {disc record, lit r, g, b, depth}
        zoff = cfg->record_format == SPLAT_RECORDS_DISC48 ? 8u : 11u;
        zstride = 12u;
    }
    const splat_aov *aov = a.aov;
    if (aov) {
        const int arc = aov_check(ctx, cfg, aov, zsrc != nullptr);
        if (arc != SPLAT_OK) return arc;
    }
    const TileBand band = tile_band(width, height, T, cfg->tile_row0, cfg->tile_row1);
    if (band.empty()) return SPLAT_OK;
    const uint32_t ntx = band.ntx, nty = band.nty, r0 = band.row0, r1 = band.row1;
    CompositeParams p;
    p.color = (const float4 *)a.color_opacity;
    p.color_stride = a.color_stride_vec4;
    p.normals = (const float4 *)a.normals;
    p.normal_stride = a.normal_stride_vec4;
    p.projected = (const float4 *)a.projected;
    p.compact = cfg->record_format == SPLAT_RECORDS_COMPACT;
    p.lit32 = lit32;
    p.prelit = cfg->prelit != 0;
    p.disc = is_disc;
    p.disc_stride = (cfg->record_format == SPLAT_RECORDS_DISC48 || (p.disc && lit32)) ? 3u : 2u;
    p.disc_lit = p.disc && lit32;
    p.indices = (const uint32_t *)a.tile_indices;
    p.counts = (const uint32_t *)a.tile_counts;
    p.offsets = (const uint32_t *)a.tile_offsets;
    p.width = width;
    p.height = height;
    p.ntx = ntx;
    p.tile_row0 = r0;
    p.out_rgba8 = (uint32_t *)a.out_rgba8;
    p.out_rgba32f = (float4 *)a.out_rgba32f;
    p.consumed = (unsigned long long *)a.consumed;
    p.frame_total = a.frame_total;
    p.report = a.report;
    p.report_seq = a.report_seq;
    p.tile_order = nullptr; // (k_composite_px's hints: px_order_prepare sets the ones it has)
    p.tile_cost = nullptr;
    p.order_src = nullptr;
    p.order_dst = nullptr;
    p.cost_prev = nullptr;
    p.aov_depth = aov ? (float *)aov->depth_f32 : nullptr;
    p.aov_alpha = aov ? (float *)aov->alpha_f32 : nullptr;
    p.aov_id = aov ? (uint32_t *)aov->id_u32 : nullptr;
    // (without a depth to gather the kernels still read one word per entry: stride 0 keeps it on a valid one)
    p.aov_z = (aov && aov->depth_f32) ? zsrc + zoff : (const float *)a.tile_counts;
    p.aov_zstride = (aov && aov->depth_f32) ? zstride : 0u;
    // 16x16 tiles: k_composite_px / k_composite, whose quadrant mapping is built for them; any other size the binner
    // accepts: k_composite_tile (composite_tile.hip)
    if (T != CT) return composite_tile_launch(ctx, cfg, p, band, &report.launched);
    // Which kernel composites 16x16 tiles.  Nearest on top, on screens of at least PX_MIN_TILES tiles: k_composite_px
    // (composite_px.hip) — a builder and a consumer wave per tile, every lane walking its own entries; the oriented disc and
    // the ellipsoid as well, their footprint evaluated per queued pixel.  The whole screen decides, not the band of tile rows
    // this call renders: the ranks of a multi-GPU frame must run the same arithmetic for their bands to stitch into the
    // single-GPU image bit for bit.  Below that (C0's 256 tiles: 18 against 22 us), and for the reference-literal blend on
    // every screen: round 2's k_composite — four waves per tile, one per 8x8-pixel quadrant, each visiting every entry that
    // touches its quadrant.  SPLAT_COMPOSITE=pixel | quadrant or splat_composite_options force one of them for the
    // nearest-on-top blend (composite_uses_px: the ellipsoid backward asks the same rule).
    if (cfg->mode == SPLAT_COMPOSITE_FRONT_TO_BACK && composite_uses_px(ctx, ntx, nty)) return composite_px_launch(ctx, cfg, p, band, &report.launched);
    const bool ok = variant_dispatch(
        [&](auto mode, auto eo, auto disc, auto lit, auto aov_, auto ell) {
            if constexpr (composite_variant_exists(mode.value, disc.value, lit.value, aov_.value, ell.value)) {
                launch_kernel(ctx, SPLAT_STAGE_COMPOSITE, k_composite<mode.value, eo.value, disc.value, lit.value, aov_.value, ell.value>,
                              dim3(ntx, r1 - r0), dim3(256), p);
                return true;
            } else return false;
        },
        OneOf<SPLAT_COMPOSITE_FRONT_TO_BACK, SPLAT_COMPOSITE_REFERENCE_LITERAL>{(int)cfg->mode}, cfg->early_out != 0, p.disc != 0, lit32 && !p.disc,
        aov != nullptr, footprint_is_ell(cfg->footprint));
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "k_composite: no kernel for this footprint, record format, blend and outputs");
    report.launched = hipPeekAtLastError() == hipSuccess;
    LAUNCH_CHECK(ctx, "k_composite");
    return SPLAT_OK;
}

extern "C" int splat_composite_forget_history(splat_ctx *ctx) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    for (auto &h : ctx->px_hist) { // (the arrays stay: a slot's next launch starts a new streak in them)
        h.key = 0;
        h.streak = 0;
        h.last_use = 0;
    }
    return SPLAT_OK;
}

extern "C" int splat_composite_options(splat_ctx *ctx, int kernel, int ahead, int predict) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, kernel >= -1 && kernel <= 1 && ahead >= 0 && ahead <= 2 && predict >= -1 && predict <= 1);
    ctx->opt_composite_kernel = kernel;
    ctx->opt_px_ahead = ahead;
    ctx->opt_px_predict = predict;
    return splat_composite_forget_history(ctx); // (another schedule: its costs mean something else)
}
