// tile_sort.hip — the frame path's per-tile depth sort: the last stage of the tile-first binner (tile_first.hip).
//
// PerTileSorter: one workgroup per tile sorts the tile's (depth key, splat index) elements by key,
// stable, and writes the tile's index list.
//
// LSD radix, 8 bits per pass, on (key - smallest key of the tile): a tile's keys span a narrow depth
// range (<= 24 bits of difference at the bench sizes), so 3 passes instead of 4, and none at all for
// a tile whose keys are equal.  Lists up to 5888 elements are sorted inside LDS — every thread
// holds its elements in registers across the pass's barrier, so one LDS array is read and rewritten
// in place.  Longer lists take the same passes through global memory (this tile's segment of the two
// pair-value buffers as ping-pong), 4096 elements at a time.
#include "common.h"
#include "block_scan.h"
#include "variant.h"

#include <cstdlib>

constexpr uint32_t TS_THREADS = 256, TS_WAVES = 4;
// Two size classes, one launch each over all tiles (a workgroup whose tile belongs to the other class
// exits at once): the kernel is latency-bound (six barriers per pass, dependent LDS round trips), so
// what matters is resident workgroups per CU, and most lists are short.
//   short  <= 2048 / 3072 / 4096 elements: 8 / 12 / 16 per thread, 16 / 24 / 32 KiB staged -> six / five / four workgroups per
//           CU.  Which of the three: by the frame's mean list length (tile_sort_launch) — the denser the lists, the more of
//           them are worth taking out of the long class at the price of fewer resident workgroups in the short one
//   long    the rest: up to 24 per thread, 46 KiB staged -> three workgroups per CU; beyond 5888 elements the passes go
//           through global memory
constexpr uint32_t TS_LONG_ITEMS = 24; // (the short class holds 8, 12 or 16 elements per thread: tile_sort_launch picks per frame)
constexpr uint32_t TS_LDS_ELEMS = 5888; // 46 KiB + 5 KiB of counters: three workgroups in a CU's 160 KiB
constexpr uint32_t TS_CHUNK_ITEMS = 16; // pairs per thread and chunk of the global-memory passes (at most: a class of fewer holds fewer)

struct TileSortShared {
    uint32_t wave_hist[TS_WAVES][256];
    uint32_t digit_base[256];
    uint32_t wave_sums[TS_WAVES];
    uint32_t kmin, kmax;
};

// The end of the in-LDS sort: the tile's index list goes out, and THE ORDER CHECK.  The tile's list must be in strictly
// increasing (depth key, splat index) order — that IS the contract (TileBinner.binSorted applied to the stable depth
// order), so verifying it here verifies every pass that led to it, in this kernel and in the two passes of the tile-id
// sort before it, whichever way they ranked: an unstable rank anywhere leaves equal digits out of their earlier order,
// i.e. keys or tied indices out of order in the final list.  A violation raises the frame's flag, and the host renders
// the frame again with ballot ranking (binner_settle).
// A wave takes 63 elements per step and reads 64: an element's successor sits in the next lane (wave_shl:1 — no LDS
// instruction: the kernel is bound by those), lane 63 holds the successor of lane 62 and writes nothing — the next step's
// lane 0 has that element.
__device__ __forceinline__ void tile_list_out(uint2 *s_el, uint32_t n, uint32_t *__restrict__ out, uint32_t *frame_flags, bool inject,
                                              uint32_t inject_pos, uint32_t tid) {
    const uint32_t lane = tid & 63, w = tid >> 6;
    if (inject) { // test hook (splat_debug_inject_order_fault): the check below must see this
        if (tid == 0 && n >= inject_pos + 2u) {
            const uint2 a = s_el[inject_pos];
            s_el[inject_pos] = s_el[inject_pos + 1];
            s_el[inject_pos + 1] = a;
        }
        __syncthreads();
    }
    bool bad = false;
    for (uint32_t s0 = 0; s0 * 63u < n; s0 += 4 * TS_WAVES) { // (uniform trip count: the lane shifts below want whole waves)
        uint2 a[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) { // four reads in flight, as in the passes
            const uint32_t p = (s0 + i * TS_WAVES + w) * 63u + lane;
            a[i] = s_el[p < n ? p : n - 1];
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t p = (s0 + i * TS_WAVES + w) * 63u + lane;
            if (p < n && lane < 63) out[p] = a[i].y;
            const uint32_t bx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a[i].x, 0x130, 0xf, 0xf, false);
            const uint32_t by = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a[i].y, 0x130, 0xf, 0xf, false);
#ifndef TS_NO_ORDER_CHECK // (measuring knob of tools/build_variant.sh: what the check costs, profiles/r03_d_order_check_cost.txt)
            const unsigned long long ka = ((unsigned long long)a[i].x << 32) | a[i].y, kb = ((unsigned long long)bx << 32) | by;
            if (p + 1 < n && lane < 63) bad |= ka >= kb;
#endif
        }
    }
    if (__any(bad) && lane == 0) atomicOr(frame_flags, FRAME_FLAG_ORDER);
}

// The test build (-DSPLAT_TEST_HOOKS, libsplat_hip_hooks.so: tests/ only) gives the kernel three more parameters: the tile whose
// finished list gets two neighbours swapped before the order check, where, and a dispatch order for the workgroups.  The shipped
// kernels do not carry them.
#ifdef SPLAT_TEST_HOOKS
#define TS_HOOK_PARAMS , uint32_t inject_tile, uint32_t inject_pos, const uint32_t *__restrict__ order
#define TS_HOOK_ARGS , inject, inject_pos, ctx->debug_sort_order
#else
#define TS_HOOK_PARAMS
#define TS_HOOK_ARGS
#endif
template <bool RANK_ATOMIC, uint32_t TS_MAX_ITEMS, bool LAST_CLASS>
__global__ __launch_bounds__(TS_THREADS, TS_MAX_ITEMS <= 8 ? 6 : TS_MAX_ITEMS <= 12 ? 5 : TS_MAX_ITEMS <= 16 ? 4 : 3) void k_tile_sort(const uint32_t *__restrict__ offsets, uint32_t tiles,
                                                                                    uint32_t n_above, uint2 *vals, uint2 *scratch,
                                                                                    uint32_t *__restrict__ out_idx,
                                                                                    uint32_t *__restrict__ counts,
                                                                                    uint32_t *__restrict__ frame_flags TS_HOOK_PARAMS) {
    static_assert(TS_MAX_ITEMS % 4 == 0, "items are processed in groups of four");
    constexpr uint32_t TS_CAP = TS_MAX_ITEMS * TS_THREADS < TS_LDS_ELEMS ? TS_MAX_ITEMS * TS_THREADS : TS_LDS_ELEMS;
    __shared__ TileSortShared sh;
    __shared__ uint2 s_el[TS_CAP];
    uint32_t *run_base = reinterpret_cast<uint32_t *>(s_el); // long-list path (s_el unused there): start of each digit's run
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#ifdef SPLAT_TEST_HOOKS
    const uint32_t t = order ? order[blockIdx.x] : blockIdx.x; // (splat_debug_set_tile_sort_order: any permutation gives the same lists)
#else
    const uint32_t t = blockIdx.x;
    constexpr uint32_t inject_tile = 0xffffffffu, inject_pos = 0; // (no tile is the victim: the swap below folds away)
#endif
    const uint32_t base = offsets[t], n = offsets[t + 1] - base;
    if (counts && tid == 0) { // (first launch: the tile counts the composite reads, and how many tiles are beyond this class)
        counts[t] = n;
        if (n > TS_MAX_ITEMS * TS_THREADS) atomicAdd(frame_flags + 2, 1u);
    }
    if (n <= n_above || (!LAST_CLASS && n > TS_CAP)) return; // empty, or another class's tile
    uint2 *src = vals + base, *dst = scratch + base;
    const bool in_lds = !LAST_CLASS || n <= TS_CAP;

    if (tid == 0) {
        sh.kmin = 0xffffffffu;
        sh.kmax = 0;
    }
    __syncthreads();

    // load (LDS path) and the tile's key range.  All of a thread's loads are issued before the first
    // is used: one load per loop trip left every workgroup waiting out up to 23 memory latencies in a
    // row (48 of the kernel's 76 us at C2 went there).  The pairs are loaded in the passes' own layout — position =
    // (wave, item, lane) — and stay in registers: the first pass ranks them from there (no staging write and read).
    uint32_t lo = 0xffffffffu, hi = 0;
    const uint32_t items = ((n + TS_THREADS - 1) / TS_THREADS + 3u) & ~3u;
    const uint32_t wbase = w * items * 64 + lane;
    uint2 el[TS_MAX_ITEMS];
    if (in_lds) {
#pragma unroll
        for (uint32_t g = 0; g < TS_MAX_ITEMS; g += 4) {
            if (g < items) {
#pragma unroll
                for (uint32_t i = g; i < g + 4; ++i) {
                    const uint32_t p = wbase + i * 64;
                    el[i] = src[p < n ? p : n - 1]; // (padding re-reads the last pair: harmless for the key range)
                }
            }
        }
#pragma unroll
        for (uint32_t g = 0; g < TS_MAX_ITEMS; g += 4) {
            if (g < items) {
#pragma unroll
                for (uint32_t i = g; i < g + 4; ++i) {
                    lo = min(lo, el[i].x);
                    hi = max(hi, el[i].x);
                }
            }
        }
    } else {
        for (uint32_t p = tid; p < n; p += TS_THREADS) {
            const uint32_t k = src[p].x;
            lo = min(lo, k);
            hi = max(hi, k);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d));
    }
    if (lane == 0) {
        atomicMin(&sh.kmin, lo);
        atomicMax(&sh.kmax, hi);
    }
    __syncthreads();
    const uint32_t kmin = sh.kmin, range = sh.kmax - kmin;
    const uint32_t passes = range == 0 ? 0u : (32u - (uint32_t)__builtin_clz(range) + 7u) / 8u;

    if (in_lds) {
        // per thread, wave-striped: position = (wave, item, lane).  Items go in groups of four so that
        // four LDS reads, then four returning atomics, are in flight together (a branch per item
        // would expose every round trip); positions past n are padding and do nothing.
        if (passes == 0) { // every key equal: the list is in order as it stands
#pragma unroll
            for (uint32_t g = 0; g < TS_MAX_ITEMS; g += 4) {
                if (g < items) {
#pragma unroll
                    for (uint32_t i = g; i < g + 4; ++i)
                        if (wbase + i * 64 < n) s_el[wbase + i * 64] = el[i];
                }
            }
            __syncthreads();
        }
        for (uint32_t pass = 0; pass < passes; ++pass) {
            const uint32_t shift = pass * 8;
            for (uint32_t i = tid; i < TS_WAVES * 256; i += TS_THREADS) (&sh.wave_hist[0][0])[i] = 0;
            __syncthreads();
            uint32_t rank[TS_MAX_ITEMS];
#pragma unroll
            for (uint32_t g = 0; g < TS_MAX_ITEMS; g += 4) {
                if (g < items) {
                    if (pass > 0) { // (the first pass's pairs are in registers)
#pragma unroll
                        for (uint32_t i = g; i < g + 4; ++i) {
                            const uint32_t p = wbase + i * 64;
                            el[i] = s_el[p < n ? p : n - 1];
                        }
                    }
#pragma unroll
                    for (uint32_t i = g; i < g + 4; ++i) {
                        const uint32_t p = wbase + i * 64;
                        rank[i] = 0;
                        if (p < n) rank[i] = wave_rank<RANK_ATOMIC>(sh.wave_hist[w], ((el[i].x - kmin) >> shift) & 255u);
                    }
                }
            }
            __syncthreads();
            // digit d's run starts at the exclusive scan of the digit totals and wave w's elements of digit d follow
            // those of the waves before it: both folded into the wave's own table — ONE lookup per element (the kernel
            // is bound by LDS operations: measured per phase, the passes are 60 % of a long tile's time once its loads
            // are hidden)
            const uint32_t c0 = sh.wave_hist[0][tid], c1 = sh.wave_hist[1][tid], c2 = sh.wave_hist[2][tid], c3 = sh.wave_hist[3][tid];
            const uint32_t excl = block_exclusive_scan<true>((c0 + c1) + (c2 + c3), sh.wave_sums);
            sh.wave_hist[0][tid] = excl;
            sh.wave_hist[1][tid] = excl + c0;
            sh.wave_hist[2][tid] = excl + c0 + c1;
            sh.wave_hist[3][tid] = excl + c0 + c1 + c2;
            __syncthreads();
#pragma unroll
            for (uint32_t g = 0; g < TS_MAX_ITEMS; g += 4) {
                if (g < items) {
                    uint32_t pos[4];
#pragma unroll
                    for (uint32_t i = g; i < g + 4; ++i) pos[i - g] = sh.wave_hist[w][((el[i].x - kmin) >> shift) & 255u] + rank[i];
#pragma unroll
                    for (uint32_t i = g; i < g + 4; ++i)
                        if (wbase + i * 64 < n) s_el[pos[i - g]] = el[i];
                }
            }
            __syncthreads();
        }
        tile_list_out(s_el, n, out_idx + base, frame_flags, t == inject_tile, inject_pos, tid);
        return;
    }

    // ---- long list: the same passes through global memory -------------------------------------
    // (in chunks of as many pairs per thread as the in-LDS path holds: a short class that runs as the last one must not
    // pay registers for this path)
    constexpr uint32_t CH_ITEMS = TS_MAX_ITEMS < TS_CHUNK_ITEMS ? TS_MAX_ITEMS : TS_CHUNK_ITEMS;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t shift = pass * 8;
        // digit totals of the whole list -> start of every digit's run
        sh.digit_base[tid] = 0;
        __syncthreads();
        for (uint32_t p = tid; p < n; p += TS_THREADS) atomicAdd(&sh.digit_base[((src[p].x - kmin) >> shift) & 255u], 1u);
        __syncthreads();
        const uint32_t tot = sh.digit_base[tid];
        const uint32_t start = block_exclusive_scan<true>(tot, sh.wave_sums);
        run_base[tid] = start;
        __syncthreads();
        for (uint32_t c0 = 0; c0 < n; c0 += CH_ITEMS * TS_THREADS) {
            for (uint32_t i = tid; i < TS_WAVES * 256; i += TS_THREADS) (&sh.wave_hist[0][0])[i] = 0;
            __syncthreads();
            uint2 el[CH_ITEMS];
            uint32_t rank[CH_ITEMS];
#pragma unroll
            for (uint32_t i = 0; i < CH_ITEMS; ++i) {
                const uint32_t p = c0 + w * (CH_ITEMS * 64) + i * 64 + lane;
                el[i] = src[p < n ? p : n - 1];
                rank[i] = 0;
                if (p < n) rank[i] = wave_rank<RANK_ATOMIC>(sh.wave_hist[w], ((el[i].x - kmin) >> shift) & 255u);
            }
            __syncthreads();
            const uint32_t dcount = ts_wave_prefixes(sh.wave_hist, tid);
            const uint32_t rb = run_base[tid];
            sh.digit_base[tid] = rb; // this chunk's elements of digit tid start here
            run_base[tid] = rb + dcount;
            __syncthreads();
#pragma unroll
            for (uint32_t i = 0; i < CH_ITEMS; ++i) {
                const uint32_t p = c0 + w * (CH_ITEMS * 64) + i * 64 + lane;
                if (p < n) {
                    const uint32_t d = ((el[i].x - kmin) >> shift) & 255u;
                    dst[sh.digit_base[d] + sh.wave_hist[w][d] + rank[i]] = el[i];
                }
            }
            __syncthreads();
        }
        uint2 *tmp = src; src = dst; dst = tmp;
        __threadfence_block(); // the next pass reads what other waves of this workgroup just stored
        __syncthreads();
    }
    bool bad = false; // the order check, as above
    for (uint32_t p = tid; p < n; p += TS_THREADS) {
        const bool inj = t == inject_tile && n >= inject_pos + 2u;
        uint2 a = src[p];
        if (inj && (p == inject_pos || p == inject_pos + 1)) a = src[p == inject_pos ? p + 1 : p - 1];
        out_idx[base + p] = a.y;
        if (p + 1 < n) {
            uint2 b = src[p + 1];
            if (inj && (p + 1 == inject_pos || p + 1 == inject_pos + 1)) b = src[p + 1 == inject_pos ? p + 2 : p];
            bad |= a.x > b.x || (a.x == b.x && a.y >= b.y);
        }
    }
    if (__any(bad) && lane == 0) atomicOr(frame_flags, FRAME_FLAG_ORDER);
}

// mean_list: the frame's pairs per tile of its band, as far as the host knows them (the previous frame's in a sync-free frame).
int tile_sort_launch(splat_ctx *ctx, const TileSortArgs &a) {
    uint32_t *const counts = a.counts, *const short_class_io = a.short_class_io;
    {
        int prc = ctx_resolve_rank_mode(ctx); // (probe of the LDS atomics' lane order, once per context)
        if (prc != SPLAT_OK) return prc;
    }
    const bool ra = rank_atomic_ok(ctx, true); // (every list is checked below: atomics are allowed here by default)
#ifdef SPLAT_TEST_HOOKS
    const uint32_t inject = ctx->inject_order_fault ? ctx->inject_order_fault - 1u : 0xffffffffu; // one-shot test hook
    const uint32_t inject_pos = ctx->inject_order_position;
    ctx->inject_order_fault = 0;
#endif
    // A screen — or a multi-GPU rank's band of tile rows — of so few tiles that the long class's kernel takes them in a round or
    // a few gains nothing from a second, denser class: one launch sorts every tile (a dependent launch costs ~5 us whatever it
    // does, and each launch ends with the life of its longest tile).  Measured with virtual ranks (profiles/r05_h_band_tile_sort_
    // one_class.txt): bands of 840 tiles (C2, eight ranks) 32 -> 22 us, of 2040 (four ranks) 35 -> 29, of ~3000 (C3, eight ranks)
    // 48 -> 44; a whole C2 screen (8160 tiles, 4969 of them non-empty) is slower with one launch (77 -> 83 us,
    // profiles/r03_j_tile_sort_one_launch_C2.txt).
    const bool one_class = (a.band_tiles ? a.band_tiles : a.tiles) <= 4200u;
    // The short class's size, by the frame's mean list length (measured, `bin_tile_sort` with 8 | 12 | 16 elements per thread:
    // C1, mean 570: 45.6 | 41.4 | 45.9 us; C3, mean 910: 193 | 180 | 188; C2, mean 1380: 77.0 | 76.6 | 72.9 — and a third
    // class in between loses its launch: profiles/r04_u_tile_sort_classes.txt).  SPLAT_TILE_SORT_SHORT=8 | 12 | 16 forces one.
    static const uint32_t force_short = [] {
        const char *e = getenv("SPLAT_TILE_SORT_SHORT");
        const int v = e ? atoi(e) : 0;
        return (v == 8 || v == 12 || v == 16) ? (uint32_t)v : 0u;
    }();
    const uint32_t short_items = force_short ? force_short : a.mean_list < 320u ? 8u : a.mean_list < 1152u ? 12u : 16u;
    const uint32_t short_cap = short_items * TS_THREADS;
    // (two passes of up to 12 bits instead of three of 8 — SPLAT_TILE_SORT_DIGITS=12 in rounds 3 and 4 — measured slower, 76 + 33
    // against 56 + 23 us at C2: profiles/r03_f_tile_sort_wide_digits_C2.txt; removed in round 5)
    // One launch over all tiles for one class: `items` elements per thread; `last`: the class also takes the tiles beyond its
    // LDS, through global memory; the tiles of at most `above` elements are another launch's.  The kernels that exist: the
    // long class as the last one, and each short class as the last one or not.
    auto launch_class = [&](uint32_t items, bool last, uint32_t above, uint32_t *class_counts) {
        return variant_dispatch(
            [&](auto ra_, auto items_, auto last_) {
                if constexpr (items_.value != (int)TS_LONG_ITEMS || last_.value) {
                    launch_kernel(ctx, NO_STAGE, k_tile_sort<ra_.value, (uint32_t)items_.value, last_.value>, dim3(a.tiles), dim3(TS_THREADS), a.offsets,
                                  a.tiles, above, a.vals, a.scratch, a.out_idx, class_counts, a.frame_flags TS_HOOK_ARGS);
                    return true;
                } else return false;
            },
            ra, OneOf<8, 12, 16, (int)TS_LONG_ITEMS>{(int)items}, last);
    };
    bool ok, no_long = false;
    if (one_class) {
        ok = launch_class(TS_LONG_ITEMS, true, 0u, counts);
    } else {
        // The frame before (same band, sync-free) had NO tile beyond the short class: the long class's launch would be 5 us of
        // workgroups that look at their tile and leave (C1: every frame).  The short class's kernel then runs as the last
        // class: a tile that has outgrown it since goes through its global-memory passes — slow, correct, and counted, so
        // that the next frame launches both classes again.
        // (the count is of the tiles beyond THAT frame's short class: it says nothing when the class has changed since)
        no_long = a.long_tiles_hint == 0u && short_class_io && *short_class_io == short_items;
        if (short_class_io) *short_class_io = short_items;
        ok = launch_class(short_items, no_long, 0u, counts);
        if (ok && !no_long) ok = launch_class(TS_LONG_ITEMS, true, short_cap, nullptr);
    }
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "k_tile_sort: no kernel for this class");
#ifdef SPLAT_TEST_HOOKS
    ctx->tile_sort_launches = one_class || no_long ? 1u : 2u;
#endif
    LAUNCH_CHECK(ctx, "k_tile_sort");
    return SPLAT_OK;
}

#ifdef SPLAT_TEST_HOOKS // (the test build only: include/splat.h)
extern "C" int splat_debug_set_tile_sort_order(splat_ctx *ctx, const void *order_dptr) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ctx->debug_sort_order = (const uint32_t *)order_dptr;
    return SPLAT_OK;
}

extern "C" int splat_debug_tile_sort_launches(splat_ctx *ctx, uint32_t *launches) {
    if (!ctx || !launches) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx/launches is NULL");
    *launches = ctx->tile_sort_launches;
    return SPLAT_OK;
}

extern "C" int splat_debug_inject_order_fault(splat_ctx *ctx, uint32_t tile, uint32_t position) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, tile != 0xffffffffu);
    ARG_CHECK(ctx, position < 0x3fffffffu); // (the kernel forms position + 2: no wrap, whatever a test passes)
    ctx->inject_order_fault = tile + 1u;
    ctx->inject_order_position = position;
    return SPLAT_OK;
}
#endif
