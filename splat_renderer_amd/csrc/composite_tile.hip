// composite_tile.hip — the per-pixel alpha composite for every tile size but 16 (k_composite_tile).
//
// k_composite (composite.hip) and k_composite_px (composite_px.hip) have the 16x16 tile built into their structure.  For a
// tile of T x T pixels (T = 1 ... 4096, what splat_bin_create accepts) the screen's tiles are cut into 16x16-pixel WINDOWS
// anchored at each tile's origin, and a window is k_composite's workgroup over its tile's list: composite_quadrant.h, which
// holds the body and describes the design.  Here: the window of each workgroup, the per-tile counters of tiles of more than
// one window, and the launch.
#include "composite_quadrant.h"

template <int MODE, bool EARLY_OUT, bool DISC, bool LIT32, bool AOV = false, bool ELL = false>
__global__ __launch_bounds__(256) void k_composite_tile(CompositeParams p, uint32_t T, uint32_t wpt, uint2 *win_counts) {
    // workgroup = window (wx, wy) of tile (tx, ty)
    const uint32_t tx = blockIdx.x / wpt, wx = blockIdx.x - tx * wpt;
    const uint32_t ty0 = blockIdx.y / wpt, wy = blockIdx.y - ty0 * wpt;
    composite_window<true, MODE, EARLY_OUT, DISC, LIT32, AOV, ELL>(p, {tx, ty0 + p.tile_row0, wx, wy, T, wpt, win_counts});
}

// One thread per tile of the band: the largest {staged, consumed} over its windows (k_composite_tile's win_counts, laid out as
// its grid), added to the per-tile counters.
__global__ __launch_bounds__(256) void k_window_counts(const uint2 *__restrict__ win_counts, unsigned long long *consumed, uint32_t ntx,
                                                       uint32_t band_rows, uint32_t tile_row0, uint32_t wpt) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ntx * band_rows) return;
    const uint32_t tx = t % ntx, ty0 = t / ntx, row = ntx * wpt;
    uint32_t st = 0, us = 0;
    for (uint32_t wy = 0; wy < wpt; ++wy)
        for (uint32_t wx = 0; wx < wpt; ++wx) {
            const uint2 c = win_counts[(size_t)(ty0 * wpt + wy) * row + tx * wpt + wx];
            st = max(st, c.x);
            us = max(us, c.y);
        }
    if (st) {
        const size_t tile_idx = (size_t)(ty0 + tile_row0) * ntx + tx;
        consumed[tile_idx * 2] += (unsigned long long)st;
        consumed[tile_idx * 2 + 1] += (unsigned long long)us;
    }
}

int composite_tile_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, const CompositeParams &p, const TileBand &band, bool *launched) {
    const uint32_t T = cfg->tile_size, wpt = div_up(T, CT), r0 = band.row0, r1 = band.row1;
    const dim3 grid(p.ntx * wpt, (r1 - r0) * wpt), block(256);
    uint2 *win_counts = nullptr;
    if (p.consumed && wpt > 1) { // (every window of the launch writes its pair: nothing to clear)
        const uint32_t windows = grid.x * grid.y;
        const int rc = device_reserve(ctx, &ctx->d_window_counts, &ctx->window_counts_cap, windows, (size_t)windows * sizeof(uint2),
                                      "composite window counters hipMalloc");
        if (rc != SPLAT_OK) return rc;
        win_counts = ctx->d_window_counts;
    }
    // (the auxiliary outputs are nearest-on-top only: composite.hip's aov_check refused them for the reference-literal blend)
    const bool want_aov = p.aov_depth || p.aov_alpha || p.aov_id;
    const bool ok = variant_dispatch(
        [&](auto mode, auto eo, auto disc, auto lit, auto aov, auto ell) {
            if constexpr (composite_variant_exists(mode.value, disc.value, lit.value, aov.value, ell.value)) {
                launch_kernel(ctx, SPLAT_STAGE_COMPOSITE, k_composite_tile<mode.value, eo.value, disc.value, lit.value, aov.value, ell.value>,
                              grid, block, p, T, wpt, win_counts);
                return true;
            } else return false;
        },
        OneOf<SPLAT_COMPOSITE_FRONT_TO_BACK, SPLAT_COMPOSITE_REFERENCE_LITERAL>{(int)cfg->mode}, cfg->early_out != 0, p.disc != 0,
        p.lit32 && !p.disc, want_aov, footprint_is_ell(cfg->footprint));
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "k_composite_tile: no kernel for this footprint, record format, blend and outputs");
    *launched = hipPeekAtLastError() == hipSuccess;
    LAUNCH_CHECK(ctx, "k_composite_tile");
    if (win_counts) {
        const uint32_t band_tiles = p.ntx * (r1 - r0);
        hipLaunchKernelGGL(k_window_counts, dim3(div_up(band_tiles, 256)), dim3(256), 0, ctx->stream, (const uint2 *)win_counts, p.consumed,
                           p.ntx, r1 - r0, r0, wpt);
        LAUNCH_CHECK(ctx, "k_window_counts");
    }
    return SPLAT_OK;
}
