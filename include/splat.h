/*
 * splat.h — C ABI of libsplat_hip.so: the MI355X (gfx950) tile-raster hot path of
 * ath92/splat-renderer behind plain pointers and sizes.
 *
 * The reference has no FFI: its boundary is the TypeScript class surface of the stage classes
 * (SURVEY.md §8b).  Each entry point below replaces the GPU work of one reference verb; the
 * reference file:line it replaces is cited on every declaration (paths under /root/reference).
 * The bindings a maintainer adds on the reference side (N-API stub + host classes) are shown in
 * INTEGRATION.md; the Python mirror used by tests/bench is splat_renderer_amd/host.py.
 *
 * Conventions
 *  - every function returns SPLAT_OK (0) or a negative SPLAT_ERR_*; the message is available
 *    from splat_last_error(ctx).  No C++ exception crosses this boundary.
 *  - one ctx = one HIP device + one stream.  All work is enqueued on that stream in call order
 *    (the reference's "queue submission order").  A ctx is not thread-safe; distinct ctxs are
 *    independent.  Functions do not synchronise with the host unless documented.
 *  - "dptr" arguments are device pointers (from splat_buf_alloc, hipMalloc, or a
 *    torch.Tensor.data_ptr()) and must be 16-byte aligned.
 *  - there is NO CPU fallback anywhere behind this ABI.
 */
#ifndef SPLAT_H
#define SPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_ABI_VERSION 3 /* 3 (round 5): splat_composite_options lost its slack argument; splat_sort_lookback_timeouts and sort mode 1 are gone; the splat_debug_* hooks moved behind SPLAT_TEST_HOOKS */

#define SPLAT_OK 0
#define SPLAT_ERR_INVALID (-1)  /* bad argument */
#define SPLAT_ERR_HIP (-2)      /* a HIP runtime call failed */
#define SPLAT_ERR_OOM (-3)      /* device allocation failed */
#define SPLAT_ERR_CAPACITY (-4) /* a fixed-capacity object is too small for this call */
#define SPLAT_ERR_STATE (-5)    /* getter called before the verb that produces its result */
#define SPLAT_ERR_NO_DEVICE (-6)
#define SPLAT_ERR_COMM (-7)     /* RCCL call failed */
#define SPLAT_ERR_RETRY (-8)    /* the previous frame's tile lists failed the per-tile sort's order check (see
                                 * splat_rank_status): the context has switched to ballot ranking; render that frame again.
                                 * Returned where SPLAT_ERR_CAPACITY is for an overflowed sync-free frame, and handled the
                                 * same way by a caller: call the frame function again with the same arguments. */

typedef struct splat_ctx splat_ctx;
typedef struct splat_sorter splat_sorter;
typedef struct splat_binner splat_binner;
typedef struct splat_comm splat_comm;

/* Sizes of the reference's records (bytes). */
#define SPLAT_PROPS_BYTES 32     /* vec4(pos,radius), vec4(rgb,opacity): src/SplatPropertyManager.ts:1-5 */
#define SPLAT_PROJECTED_BYTES 32 /* ProjectedSplat: src/SplatProjector.ts:47-54 */
#define SPLAT_SORT_BLOCK 3840    /* key-buffer padding quantum: src/RadixSorter.ts:12-19,46-52 */

/* stage ids for splat_stage_time_ms */
enum {
    SPLAT_STAGE_PROJECT = 0, /* project + depth keys */
    SPLAT_STAGE_SORT = 1,
    SPLAT_STAGE_BIN = 2,     /* count + scan + fill */
    SPLAT_STAGE_COMPOSITE = 3,
    SPLAT_STAGE_EXCHANGE = 4, /* multi-GPU all-gather */
    /* parts of SPLAT_STAGE_BIN in the tile-first frame order (each inside the BIN interval): */
    SPLAT_STAGE_BIN_SCATTER = 5,   /* first pass of the tile-id sort fused with the pair expansion (+ its row scan) */
    SPLAT_STAGE_BIN_PASS2 = 6,     /* second pass (upsweep, row scan, downsweep) + tile offsets */
    SPLAT_STAGE_BIN_TILE_SORT = 7, /* PerTileSorter: depth order inside every tile */
    SPLAT_STAGE_COUNT = 8
};

/* ---- context ---------------------------------------------------------------------------- */
/* GPUDevice + queue equivalent (src/main.ts:16-36). */
int splat_ctx_create(int device_ordinal, splat_ctx **out);
/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int splat_ctx_create_on_stream(int device_ordinal, void *hip_stream, splat_ctx **out);
void splat_ctx_destroy(splat_ctx *ctx);
/* Last error text of this ctx (or of the calling thread when ctx is NULL). Never NULL. */
const char *splat_last_error(splat_ctx *ctx);
/* device.queue.onSubmittedWorkDone equivalent: wait for everything enqueued so far. */
int splat_sync(splat_ctx *ctx);
int splat_abi_version(void);
/* Enable per-stage hipEvent timing (off by default: events cost a few us per stage). */
int splat_set_timing(splat_ctx *ctx, int enabled);
/* Restrict event recording to the stages whose bit (1 << stage id) is set (default: all).  Each
 * recorded stage costs ~10 us of stream idle per frame, so a throughput measurement that only needs
 * one kernel's duration enables only that stage.  Bit 31 (SPLAT_TIMING_COUNT_ENTRIES, set by default):
 * a timed whole-frame call also counts, per tile, the list entries its composite staged and consumed
 * (splat_timing_consumed) — the counting instantiation of the kernel is a few per cent slower than the
 * one every other frame runs, so a measurement of the production kernel clears the bit and takes the
 * counts from a frame outside its timed region (they are a property of the input). */
#define SPLAT_TIMING_COUNT_ENTRIES 0x80000000u
int splat_set_timing_stages(splat_ctx *ctx, uint32_t stage_mask);
/* A stage that is ONE kernel (the composite) carries its event pair on the launch itself; even so a timed launch costs the
 * stream ~5 us (C2: 0.326 ms per frame with a pair on every composite, 0.321 with none).  every = n: only every n-th such
 * launch while timing is on is timed (the first one is); splat_stage_time_stats then averages over those.  Default 1. */
int splat_set_timing_sampling(splat_ctx *ctx, uint32_t every);
/* Duration of the most recent run of `stage`; synchronises on that stage's end event. */
int splat_stage_time_ms(splat_ctx *ctx, int stage, float *ms);
/* Every timed run of `stage` since timing was last enabled: number of samples and their summed
 * duration (synchronises).  Enabling timing again starts a new sample set. */
int splat_stage_time_stats(splat_ctx *ctx, int stage, uint32_t *samples, double *total_ms);
/* List entries of splat_render_frame's composite since timing was last enabled, summed over tiles and timed
 * frames; synchronises.  *consumed = P_used of SURVEY §8d: per tile, the entries its pixels visited before the
 * last of them reached alpha >= 0.99 (the whole list if one never did; = the pair total with early-out off).
 * *staged = what the kernel actually gathered: the same, rounded up to its 256-entry batches. */
int splat_timing_consumed(splat_ctx *ctx, uint64_t *staged, uint64_t *consumed);

/* ---- buffers (GPUBuffer equivalent: device.createBuffer / queue.writeBuffer / mapAsync) --- */
int splat_buf_alloc(splat_ctx *ctx, size_t bytes, void **dptr);
int splat_buf_free(splat_ctx *ctx, void *dptr);
int splat_buf_upload(splat_ctx *ctx, void *dst_dptr, const void *src_host, size_t bytes);   /* async on the stream, src is staged */
int splat_buf_download(splat_ctx *ctx, void *dst_host, const void *src_dptr, size_t bytes); /* synchronous */
int splat_buf_zero(splat_ctx *ctx, void *dptr, size_t bytes);
int splat_buf_copy(splat_ctx *ctx, void *dst_dptr, const void *src_dptr, size_t bytes); /* copyBufferToBuffer: device to device, async on the stream */

/* ---- SplatPropertyManager.updateFromCurvature  (src/SplatPropertyManager.ts:82-107,153-173) */
/* positions, curvature: vec4 per splat; props: 32-byte interleaved records. */
int splat_update_props(splat_ctx *ctx, const void *positions, const void *curvature, uint32_t n,
                       void *props);
/* The same update writing two planes (vec4(pos, radius) | vec4(rgb, opacity)) — SURVEY §8f row 1 — and the
 * one-off conversion of interleaved records into planes. */
int splat_update_props_planes(splat_ctx *ctx, const void *positions, const void *curvature, uint32_t n,
                              void *pos_radius, void *color_opacity);
int splat_props_to_planes(splat_ctx *ctx, const void *props, uint32_t n, void *pos_radius, void *color_opacity);

/* ---- SplatProjector.project  (src/SplatProjector.ts:64-132,174-194) ----------------------- */
/* uniforms: 22 host floats = VP column-major [0..15], eye [16..18], time [19], screenW [20],
 * screenH [21] (src/main.ts:126-144, src/SplatProjector.ts:35-41).
 * pos_radius: first vec4(pos,radius); consecutive splats are pr_stride_vec4 float4s apart
 * (2 = the reference's interleaved property buffer, 1 = a split plane).
 * projected: n 32-byte ProjectedSplat records (bit-exact vs oracle/orc_project).
 * keys/payload: if non-NULL the DepthKeyExtractor pass is fused in (n_padded entries, tail =
 * 0xFFFFFFFF); pass NULL to run the reference's unfused sequence. */
int splat_project(splat_ctx *ctx, const float *uniforms, const void *pos_radius,
                  uint32_t pr_stride_vec4, uint32_t n, void *projected, void *keys, void *payload,
                  uint32_t n_padded);

/* ---- DepthKeyExtractor.extract  (src/DepthKeyExtractor.ts:71-109, extract-depth-keys.wgsl:37-63) */
int splat_extract_keys(splat_ctx *ctx, const void *projected, uint32_t n, uint32_t n_padded,
                       void *keys, void *payload);

/* ---- RadixSorter  (src/RadixSorter.ts:39-100,197-271) ------------------------------------- */
/* Owns keys/keys_b/payload_a/payload_b for `capacity` pairs (capacity is rounded up to a
 * multiple of SPLAT_SORT_BLOCK like the reference's paddedSize). */
int splat_sort_create(splat_ctx *ctx, uint32_t capacity, splat_sorter **out);
void splat_sort_destroy(splat_sorter *s);
uint32_t splat_sort_capacity(const splat_sorter *s);
void *splat_sort_keys(splat_sorter *s);    /* getKeysBuffer():    input keys (u32)    */
void *splat_sort_payload(splat_sorter *s); /* getPayloadBuffer(): input payload (u32) */
/* sort(): stable ascending LSD sort of the first n pairs on key bits [bit_begin, bit_end).
 * The reference always sorts all 32 bits (4 x 8-bit passes). */
int splat_sort_run(splat_sorter *s, uint32_t n, uint32_t bit_begin, uint32_t bit_end);
/* getSortedIndicesBuffer(): payload in sorted order (valid after splat_sort_run). */
void *splat_sort_sorted_payload(splat_sorter *s);
void *splat_sort_sorted_keys(splat_sorter *s);
/* Hardware probe (diagnostic): runs ~2M wave instructions of returning LDS atomics with colliding
 * addresses and counts those whose return values were NOT in ascending lane order.  Synchronises. */
int splat_probe_lds_atomic_order(splat_ctx *ctx, uint64_t *mismatches);
/* How this sorter ranks equal digits: 0 = as the context's policy says (per-pass histogram + row scan + scatter; returning
 * LDS atomics only where the policy allows them, see the NOTE), 2 = always with ballots, -1 = library default (0).  (Round
 * 1's onesweep mode with decoupled look-back — the reference's structure, slower on MI355X — was removed in round 5.)
 * NOTE on ranking (mode 0, and the frame path's binning kernels).  Ranking a wave's keys with returning LDS atomics is
 * stable only if the lanes of one instruction that collide on an address complete in ascending lane order.  That is what
 * gfx950 does (splat_probe_lds_atomic_order: 0 mismatches in 8.4 M colliding instructions) but it is not an ISA guarantee,
 * and index lists are bit-exact work, so nothing rests on it unverified:
 *   - default: atomics are used ONLY by the tile-first frame path (splat_render_frame*, splat_band_frame), whose per-tile
 *     sort checks every tile's final list for strictly increasing (depth key, splat index) order — the contract itself,
 *     hence a complete check of every ranking pass that produced the list.  A frame that fails is reported like an
 *     overflowed sync-free frame (SPLAT_ERR_RETRY at the next call), the context ranks with ballots from then on, and the
 *     caller renders the frame again.  Every other sort (splat_sort_run, splat_bin_run, the sort-first frame order), whose
 *     result nothing checks, ranks with ballots: lane order by construction (8 ballots + mbcnt per key).
 *     WHAT IS GUARANTEED, precisely: frame N's image and lists are PROVISIONAL until frame N's report has been examined —
 *     by the next frame call on the same binner, by splat_bin_total / splat_bin_get_* / splat_band_settle, or by anything the
 *     host classes read results through (Renderer.finish / readPixels / readPixelsFloat call splat_bin_total first and
 *     render the frame again on SPLAT_ERR_RETRY / SPLAT_ERR_CAPACITY).  The output buffer of a frame that fails the check
 *     HAS been written from the wrong lists: a caller that maps it without settling the frame reads that image.  The
 *     context prints one line to stderr when it switches to ballots, and splat_rank_status counts the frames.
 *   - SPLAT_RANK=atomic: atomics wherever the start-up probe passes (the unchecked sorts too).
 *   - SPLAT_RANK=ballot: ballots everywhere.
 * The price of the guaranteed ranking on the frame path, measured on one MI355X (profiles/r03_a_rank_ab.txt): C0 0.048 ->
 * 0.054 ms, C1 0.177 -> 0.210, C2 0.359 -> 0.425, C3 0.878 -> 0.986 (+12..19 %); the price of the check: see DESIGN.md. */
int splat_sort_set_mode(splat_sorter *s, int mode);
/* Ranking status of this context: *policy = 0 checked default / 1 SPLAT_RANK=atomic / 2 ballots (SPLAT_RANK=ballot, or
 * after a failed order check); *atomics_ordered = the start-up probe's verdict (1 = in lane order, 0 = not or not asked);
 * *order_faults = frames of this context whose tile lists failed the order check (each was reported with
 * SPLAT_ERR_RETRY).  Runs the probe if it has not run yet (synchronises then). */
int splat_rank_status(splat_ctx *ctx, int *policy, int *atomics_ordered, uint32_t *order_faults);
#ifdef SPLAT_TEST_HOOKS
/* ---- test and experiment hooks: compiled only into libsplat_hip_hooks.so (-DSPLAT_TEST_HOOKS, built beside the library for
 * tests/ and tools/); the shipped library neither exports them nor carries their kernel parameters ---------------------- */
/* TEST HOOK: the next per-tile sort of this context swaps entries `position` and `position + 1` of tile `tile`'s finished
 * list just before its order check, as an out-of-lane-order ranking would have left them: the check must raise the
 * frame's flag, the next call return SPLAT_ERR_RETRY, and the frame rendered again be right.  One shot. */
int splat_debug_inject_order_fault(splat_ctx *ctx, uint32_t tile, uint32_t position);
/* EXPERIMENT HOOK: the order in which the lane-efficient composite's workgroups take the tiles of the rendered band
 * (a permutation of 0 .. tiles - 1 as u32 on the device; NULL = row-major).  Any order gives the same image. */
int splat_debug_set_tile_order(splat_ctx *ctx, const void *order_dptr);
/* EXPERIMENT HOOK: the same for the per-tile sort's workgroups (a permutation of ALL the screen's tiles; NULL = row-major). */
int splat_debug_set_tile_sort_order(splat_ctx *ctx, const void *order_dptr);
/* EXPERIMENT HOOK (tools/overlap_probe.py): the per-tile sort of the binner's last tile-first frame once more, on ctx's stream. */
int splat_debug_rerun_tile_sort(splat_ctx *ctx, splat_binner *binner);
/* TEST HOOK: how many k_tile_sort launches this context's last per-tile sort made (2: a short and a long size class; 1: a band of
 * few tiles, or a sync-free frame after one that had no tile beyond the short class). */
int splat_debug_tile_sort_launches(splat_ctx *ctx, uint32_t *launches);
/* EXPERIMENT HOOK (tools/lds_atomic_rate.py): milliseconds of a kernel that does iters x 4 LDS instructions per wave at random
 * counters of the wave's own 256-entry table, workgroups_per_cu four-wave workgroups per CU: kind 0 returning atomic adds (the
 * sort kernels' ranking instruction), 1 plain reads, 2 non-returning atomic adds. */
int splat_debug_lds_rate(splat_ctx *ctx, int kind, uint32_t workgroups_per_cu, uint32_t iters, float *ms);
#endif
/* The lane-efficient composite keeps, per context, for each of the last few (four) bands of tile rows it composited (a band
 * = these rows of this binner's lists), what its previous launch over that band cost per tile (chunks of
 * 32 list entries walked): the next launch over the same band takes its tiles longest-first and builds / gathers for each
 * tile only what that launch needed ahead of need (a tile that needs more pays one exposed gather).  Both are hints — any
 * history, stale or from another scene, gives the same image.  This forgets the history (the next two launches run
 * row-major and without a bound, as a context's first do): for measurements and tests that want the kernel's first-frame
 * behaviour. */
int splat_composite_forget_history(splat_ctx *ctx);
/* Per-context choices the environment otherwise makes for the whole process (environment table).  EVERY call
 * sets all three: a value of -1 (kernel, predict) or 0 (ahead) means "the process default", i.e. what the environment
 * variable named beside it says — not "leave as it is"; a per-context choice takes precedence over the environment:
 *   kernel  -1 default (SPLAT_COMPOSITE: lane-efficient k_composite_px on screens of >= 2048 tiles), 0 k_composite ("quadrant"),
 *            1 k_composite_px ("pixel") — for nearest-on-top frames of either footprint; the reference-literal blend always
 *            takes k_composite;
 *   ahead    0 default (SPLAT_PX_AHEAD: 1 for the isotropic footprint with the early-out, 2 otherwise), 1 or 2: chunks
 *            k_composite_px's builder wave stays ahead of its consumer wave (2: lanes whose queue for a chunk is empty go on
 *            with the next chunk's);
 *   predict -1 default (SPLAT_PX_PREDICT, on), 0 / 1: bound each tile's look-ahead by what the previous launch walked.
 * ahead and predict change the schedule only: the same bytes.  The two kernels evaluate the Gaussian differently
 * (k_composite_px builds an entry's table by a recurrence from five exponentials) and agree within the composite's stated
 * tolerance, 2e-5 per float channel, <= 1 LSB on rgba8 (tests/test_gpu_stages.py runs the oracle comparisons over all of
 * them).  Forgets the composite's history. */
int splat_composite_options(splat_ctx *ctx, int kernel, int ahead, int predict);

/* ---- PrefixSumScanner.scan  (src/PrefixSumScanner.ts:74-87, prefix-sum.wgsl:28-96) -------- */
/* Exclusive scan of n u32 (out[0] = 0); in may equal out.  total_dptr (optional) receives the
 * sum of all inputs as one u32.  Entirely on the device for any n (the reference falls back to
 * a CPU loop above 512 elements: src/PrefixSumScanner.ts:131-162). */
int splat_scan_u32(splat_ctx *ctx, const void *in, void *out, uint32_t n, void *total_dptr);

/* ---- GPUTileBinner  (src/GPUTileBinner.ts:35-50,190-377) ---------------------------------- */
/* Lists are exactly TileBinner.binSorted's (src/TileBinner.ts:426-495): splats fully
 * off-screen are culled and every tile's list is in `sorted` order. */
int splat_bin_create(splat_ctx *ctx, uint32_t tile_size, splat_binner **out);
void splat_bin_destroy(splat_binner *b);
/* binSplats(): sorted = n_sorted u32 splat indices (entries >= n_splats are padding and are
 * skipped).  Only tile rows [tile_row0, tile_row1) are binned (0, UINT32_MAX = all rows) —
 * the multi-GPU band.
 * Host round trips: the FIRST run (and any run whose pair buffers must grow) reads the 4-byte pair
 * total back to size the fill.  After that, while the previous run's total leaves 50 % headroom,
 * runs are sync-free: the total is read on the device, grids are sized from the previous total, and
 * it returns through an async copy examined by the next splat_bin_* call on this binner.  If a
 * frame's pairs outgrew that limit (more than 1.5x the previous frame's), its lists are incomplete
 * and that next call returns SPLAT_ERR_CAPACITY after raising the capacity: render the frame
 * again.  The getters below wait for the async copy. */
int splat_bin_run(splat_binner *b, const void *projected, uint32_t n_splats, const void *sorted,
                  uint32_t n_sorted, uint32_t width, uint32_t height, uint32_t tile_row0,
                  uint32_t tile_row1);
uint32_t splat_bin_tile_size(const splat_binner *b);        /* getTileSize() */
int splat_bin_counts(splat_binner *b, void **dptr);          /* getTileCountsBuffer()  u32[numTiles] */
int splat_bin_offsets(splat_binner *b, void **dptr);         /* getTileOffsetsBuffer() u32[numTiles] (+1: [numTiles] = total) */
int splat_bin_indices(splat_binner *b, void **dptr);         /* getTileIndicesBuffer() u32[total]    */
int splat_bin_total(splat_binner *b, uint64_t *total_pairs); /* sum of counts of the last run */
/* Order of work inside splat_render_frame (results are identical, tests hold both to the same lists):
 *   SPLAT_FRAME_SORT_FIRST  global depth sort of the splats, then bin in sorted order (the staged API's order);
 *   SPLAT_FRAME_TILE_FIRST  bin in index order, then depth-sort every tile's list (PerTileSorter,
 *                           src/PerTileSorter.ts:66-122) — needs tile coordinates that fit 8 bits (screens of at
 *                           most 256 x 256 tiles; beyond them every frame bins sort-first);
 *   SPLAT_FRAME_ORDER_DEFAULT  the library's choice (environment SPLAT_FRAME_ORDER=sortfirst|tilefirst overrides). */
#define SPLAT_FRAME_ORDER_DEFAULT (-1)
#define SPLAT_FRAME_SORT_FIRST 0
#define SPLAT_FRAME_TILE_FIRST 1
int splat_bin_set_frame_order(splat_binner *b, int order);
int splat_bin_dims(splat_binner *b, uint32_t *ntx, uint32_t *nty);

/* ---- PerTileSorter.sort  (src/PerTileSorter.ts:66-122,174-213) --------------------------------- */
/* The reference re-sorts every tile's list by depth in LDS (racy, capped at 2048: SURVEY I3).
 * splat_bin_run bins an already sorted order, so its lists leave it in (depth key, index) order and
 * for the staged API the stage is a CHECK: counts adjacent pairs of one tile that are not strictly
 * increasing in (depth key, splat index).  (Inside splat_render_frame's tile-first order the per-tile
 * sort is real — any list length, stable — see splat_bin_set_frame_order.)
 * tile_offsets must have num_tiles + 1 entries (as splat_bin_offsets returns).  Synchronises. */
int splat_validate_tile_order(splat_ctx *ctx, const void *projected, const void *tile_offsets,
                              uint32_t num_tiles, const void *tile_indices, uint64_t total_pairs,
                              uint64_t *violations_host);

/* ---- ComputeShaderRenderer.render / TileRenderer.render  (src/ComputeShaderRenderer.ts:97-198,362-422) */
#define SPLAT_COMPOSITE_FRONT_TO_BACK 0     /* SURVEY §8a contract 3: nearest on top (default) */
#define SPLAT_COMPOSITE_REFERENCE_LITERAL 1 /* src/ComputeShaderRenderer.ts:175-190 as written */
#define SPLAT_RECORDS_PROJECTED 0
#define SPLAT_RECORDS_COMPACT 1
#define SPLAT_RECORDS_DISC48 2 /* oriented-disc exchange records, see splat_project_slice_disc (footprint DISC only) */
#define SPLAT_RECORDS_LIT32 3  /* lit composite records: float4 {centre x, y, screen radius, depth}, float4 {lit r, g, b, opacity} per
                                * splat — everything evaluateSplat (src/ComputeShaderRenderer.ts:117-147) reads of a splat in ONE
                                * 32-byte line: the ProjectedSplat's bounds are centre -/+ radius * 1.5 in the projector's operation
                                * order (src/SplatProjector.ts:119-121), the colour already carries the shading of :143-145.
                                * splat_render_frame* writes them in place of the ProjectedSplat records when asked to (isotropic
                                * footprint), on every screen the binner takes; the composite then gathers one line per
                                * staged list entry instead of three. */
#define SPLAT_FOOTPRINT_ISOTROPIC 0
#define SPLAT_FOOTPRINT_DISC 1
#define SPLAT_FOOTPRINT_ELLIPSOID 2 /* an anisotropic 3D Gaussian (extension, no reference counterpart): splat_project_ellipsoid */
#define SPLAT_FOOTPRINT_SURFEL 3    /* a 2D Gaussian surfel (extension; "2D Gaussian surfels" below): splat_project_surfel; the
                                     * staged composites, the composite backward, the feature channels, splat_composite_surfel_depth,
                                     * splat_composite_surfel_distortion and splat_composite_backward_distortion take it */
typedef struct splat_composite_cfg {
    uint32_t mode;       /* SPLAT_COMPOSITE_* */
    uint32_t early_out;  /* 1 = stop a pixel at alpha >= 0.99 (reference :187-190) */
    uint32_t tile_size;  /* must equal the binner's: 1 ... 4096 (16: k_composite_px / k_composite; any other: k_composite_tile) */
    uint32_t tile_row0;  /* render tile rows [tile_row0, tile_row1) (multi-GPU band) */
    uint32_t tile_row1;  /* UINT32_MAX = to the last row */
    uint32_t record_format; /* what `projected` / `records` point at: SPLAT_RECORDS_PROJECTED (32-byte
                             * ProjectedSplat, the reference's struct), SPLAT_RECORDS_COMPACT (16-byte
                             * exchange records, see splat_project_slice_compact) or SPLAT_RECORDS_LIT32 (color_opacity
                             * and normals are then not read and may be NULL).  In splat_render_frame*: the format the
                             * frame's projector leaves in `projected` — PROJECTED or LIT32 */
    uint32_t prelit;        /* 1 = color_opacity holds LIT colours (splat_lit_colors): the composite then gathers two
                             * lines per staged entry instead of three and does not read normals (may be NULL) */
    uint32_t footprint;     /* SPLAT_FOOTPRINT_ISOTROPIC: ComputeShaderRenderer's screen-space Gaussian (default).
                             * SPLAT_FOOTPRINT_DISC: SequentialRenderer's / TileRenderer's oriented disc —
                             * `projected` then points at the 32-byte DISC records of splat_project_disc, mode must
                             * be FRONT_TO_BACK and record_format PROJECTED; in splat_render_frame* the projector
                             * used is splat_project_disc (normals are required even when prelit) and `projected`
                             * may be NULL (the ProjectedSplat records are then not written: a disc frame's composite
                             * reads the disc records)
                             * SPLAT_FOOTPRINT_ELLIPSOID: the anisotropic 3D Gaussian of splat_project_ellipsoid — its records
                             * are disc records and every disc rule above holds (nearest on top, PROJECTED records to
                             * splat_composite*, projected may be NULL in its frame); exp(-0.5 d^T Sigma2^-1 d) inside 3 sigma.
                             * Its frame is splat_render_frame_ellipsoids; splat_band_frame refuses it */
} splat_composite_cfg;
/* color_opacity / normals: vec4 per splat, *_stride_vec4 float4s apart.  out_rgba8 (W*H*4 bytes,
 * rgba8unorm, may be NULL) and out_rgba32f (W*H*16 bytes, may be NULL) are full-frame images;
 * only pixels of the rendered tile rows are written.  consumed_dptr (optional): u64[2 * ceil(W/16) *
 * ceil(H/16)], two counters per tile; a rendered tile's counters are incremented by {entries staged,
 * entries consumed} (see splat_timing_consumed; the sum of the second over tiles is P_used). */
/* The reference shades every splat with kd = 0.85 + 0.15 * max(dot(normal, (1,1,1)/sqrt 3), 0)
 * (src/ComputeShaderRenderer.ts:143-145).  lit[i] = vec4(rgb * kd, opacity): computed once per property
 * update instead of once per staged entry; the same bits either way (explicitly rounded operations). */
int splat_lit_colors(splat_ctx *ctx, const void *color_opacity, uint32_t color_stride_vec4,
                     const void *normals, uint32_t normal_stride_vec4, uint32_t n, void *lit);
int splat_composite(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                    uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                    const void *projected, const void *tile_indices, const void *tile_counts,
                    const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8,
                    void *out_rgba32f, void *consumed_dptr);

/* ---- auxiliary outputs of a Gaussian frame: alpha, depth and splat id beside the image ----------------------------
 * Nearest-on-top frames only (SPLAT_COMPOSITE_FRONT_TO_BACK).  Per pixel, over the list entries the pixel consumes (those
 * after its early-out stop contribute nothing): T_i = the transmittance before entry i, g_i = its footprint value (the
 * isotropic Gaussian or the oriented disc's), w_i = T_i g_i — the product the colour uses.  Each buffer is W*H elements,
 * full frame, 16-byte aligned, and may be NULL (not written); at least one must be non-NULL.  Only pixels of the rendered
 * tile rows are written, as for the image.
 *   alpha_f32  1 - T_end, T_end the transmittance the background term is multiplied by: rgb = C + bg (1 - alpha).  0 where
 *              nothing contributed.
 *   depth_f32  sum w_i z_i / sum w_i, z_i the splat's ProjectedSplat depth (distance from the camera to its centre,
 *              src/SplatProjector.ts:77; the depth the sort orders by), for both footprints.  +inf where sum w_i = 0.
 *   id_u32     the splat index (the list entry's value) of the entry with the largest w_i; on equal w the earlier entry, the
 *              nearer one, wins.  0xFFFFFFFF where nothing contributed.
 * The image of a call with buffers is bit for bit the image of the same call without them (same kernel, same schedule), and
 * rgba32f's alpha channel stays 1.0.  SPLAT_ERR_INVALID: all three NULL, a misaligned buffer, SPLAT_COMPOSITE_REFERENCE_LITERAL
 * (an entry's final weight there is not known until its list ends), or depth asked of records that do not carry it:
 *   - splat_composite_aov with SPLAT_FOOTPRINT_DISC and SPLAT_RECORDS_PROJECTED (the projector's 32-byte disc records; the
 *     48-byte SPLAT_RECORDS_DISC48 exchange records carry the depth);
 *   - a disc frame (splat_render_frame*_aov, SPLAT_FOOTPRINT_DISC) with SPLAT_RECORDS_PROJECTED and projected == NULL (with
 *     `projected` the frame writes ProjectedSplat records and the depth is read there; with SPLAT_RECORDS_LIT32 the frame's
 *     lit disc records carry it).
 * Every other record format (PROJECTED, COMPACT, LIT32 isotropic; DISC48 and lit disc records) carries the depth. */
typedef struct splat_aov {
    void *depth_f32;
    void *alpha_f32;
    void *id_u32;
} splat_aov;
/* splat_composite plus the auxiliary outputs (aov == NULL: splat_composite itself) */
int splat_composite_aov(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                        uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                        const void *projected, const void *tile_indices, const void *tile_counts,
                        const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8,
                        void *out_rgba32f, void *consumed_dptr, const splat_aov *aov);
/* splat_composite_aov with the caller's per-splat depth: the AOV depth reads z_i = depth_f32[i * depth_stride_floats] instead
 * of the records' own (ProjectedSplat records: projected + 4 floats with stride 8; a plain n-float array: stride 1).  Valid
 * for every footprint and record format splat_composite_aov takes, the projector's 32-byte disc and ellipsoid records
 * included.  The aov struct still decides which buffers are written; the image is splat_composite_aov's bit for bit.
 * SPLAT_ERR_INVALID as for splat_composite_aov, and for depth_f32 NULL, depth_stride_floats 0 or depth_f32 not 4-byte
 * aligned. */
int splat_composite_aov_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                              uint32_t color_stride_vec4, const void *normals, uint32_t normal_stride_vec4,
                              const void *projected, const void *tile_indices, const void *tile_counts,
                              const void *tile_offsets, uint32_t width, uint32_t height, void *out_rgba8,
                              void *out_rgba32f, void *consumed_dptr, const splat_aov *aov, const void *depth_f32,
                              uint32_t depth_stride_floats);

/* ---- whole frame: project -> keys -> sort -> bin -> composite ----------------
 * With cfg->tile_row0/1 set to a strict band of tile rows (multi-GPU, no exchange: every rank renders its band from
 * its own copy of the splats) only that band's pixels, lists and counts are produced, and `projected` holds records
 * only for splats that may reach the band (the projector skips the others after a conservative test).
 * Every screen the binner takes (at most 65535 tiles a side, 2^24 in all) accepts every record format and, for disc
 * frames, projected == NULL: the projector leaves each splat's clamped tile range per index — 4 bytes with 8-bit
 * coordinates up to 256 x 256 tiles, 8 bytes with 16-bit coordinates beyond (sort-first order there) — and the
 * binner bins from that range, never from the records. */
int splat_render_frame(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                       const splat_composite_cfg *cfg, const float *uniforms, const void *props,
                       const void *normals, uint32_t n, uint32_t width, uint32_t height,
                       void *projected, void *out_rgba8, void *out_rgba32f);
/* The same frame from the MI355X-native property layout: two planes of vec4 per splat instead of the
 * reference's interleaved 32-byte records (the projector then reads 16 useful bytes per 16 fetched
 * instead of per 32).  splat_update_props_planes / splat_props_to_planes produce them. */
int splat_render_frame_planes(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                              const splat_composite_cfg *cfg, const float *uniforms,
                              const void *pos_radius, const void *color_opacity, const void *normals,
                              uint32_t n, uint32_t width, uint32_t height, void *projected,
                              void *out_rgba8, void *out_rgba32f);
/* The two frames plus the auxiliary outputs (splat_aov above; aov == NULL: the frame itself).  Every route a frame takes
 * writes them: either frame order, screens beyond 256 x 256 tiles, strict bands; a frame rendered again after
 * SPLAT_ERR_CAPACITY / SPLAT_ERR_RETRY rewrites them with its image. */
int splat_render_frame_aov(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                           const splat_composite_cfg *cfg, const float *uniforms, const void *props,
                           const void *normals, uint32_t n, uint32_t width, uint32_t height,
                           void *projected, void *out_rgba8, void *out_rgba32f, const splat_aov *aov);
int splat_render_frame_planes_aov(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                                  const splat_composite_cfg *cfg, const float *uniforms,
                                  const void *pos_radius, const void *color_opacity, const void *normals,
                                  uint32_t n, uint32_t width, uint32_t height, void *projected,
                                  void *out_rgba8, void *out_rgba32f, const splat_aov *aov);

/* ---- anisotropic 3D Gaussians (SPLAT_FOOTPRINT_ELLIPSOID; an extension, no reference counterpart) ----------------------
 * One splat = four planes of one vec4 each, *_stride_vec4 float4s apart: position xyz (w ignored), scale sigma x, y, z in world
 * units (w ignored), rotation quaternion (w, x, y, z) of any non-zero length (q and -q give the same record), and the final
 * colour and opacity (rgb, opacity: not shaded — an ellipsoid has no normal; see splat_sh_colors).
 * Per splat: Sigma3 = R S S^T R^T; J the exact derivative at the centre of the projector's screen map ((W/2)(1 + c.x/c.w),
 * (H/2)(1 - c.y/c.w)), c = VP [p; 1] (= 3DGS's J W for a perspective VP); Sigma2 = J Sigma3 J^T + 0.3 I (px^2, the 3DGS
 * low-pass dilation).  The footprint is g(d) = exp(-0.5 d^T Sigma2^-1 d) where d^T Sigma2^-1 d <= 9, 0 elsewhere (d = pixel
 * centre - screen centre); the blend is the other footprints' (nearest on top, alpha = opacity g, the early-out), with no
 * 0.99 clamp of alpha and no 1/255 skip as in the 3DGS CUDA rasteriser.
 * splat_project_ellipsoid writes
 *   records[i]   = the 32-byte disc record {c.x, c.y, B00, B01, 0, B11, 0, 0}, B = U / 3, U upper-triangular with U^T U =
 *                  Sigma2^-1 (so (u, v) = B d is inside the disc record's unit circle exactly at 3 sigma); all zeros when the
 *                  centre's clip w is not > 0, the 3-sigma ellipsoid reaches w = 0 (c.w - 3 sqrt(m3 Sigma3 m3^T) <= 0, m3 the w
 *                  row of VP), det Sigma2 <= 0 or anything is not finite;
 *   projected[i] = a ProjectedSplat: bounds of the record as for discs (the exact 3-sigma box), depth as splat_project,
 *                  screenRadius = half the larger extent;
 * and keys / payload exactly as splat_project.  Sort and bin with `projected`; composite with cfg.footprint =
 * SPLAT_FOOTPRINT_ELLIPSOID and `records`.  The operation order is stated in csrc/ellipsoid.h. */
int splat_project_ellipsoid(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                            const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                            uint32_t n, void *projected, void *records, void *keys, void *payload, uint32_t n_padded);
/* View-dependent colour from spherical harmonics of degree 0-3 (the real basis and constants of 3D Gaussian splatting):
 * color_opacity_out[i] = vec4(max(0.5 + sum_k Y_k(dir) sh_k, 0), opacity_f32[i]), dir = normalize(p_i - eye), with the
 * coefficient of basis k < (degree + 1)^2 and channel c at sh[i * sh_stride_floats + 3 k + c].  eye3 is a host pointer.
 * Where |p_i - eye| (binary32) is not a positive finite number - a splat at the eye - dir = (0, 0, 0): the colour is
 * max(0.5 + C0 sh_0, 0), finite.  Its backward then writes C0 g into row 0 of dL/dsh and zeros into the other rows, zeros into
 * dL/dposition, adds nothing to dL/deye, and passes dL/dopacity through as for any splat. */
int splat_sh_colors(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                    uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, uint32_t n, void *color_opacity_out);
/* The whole frame of anisotropic Gaussians: splat_render_frame_planes_aov with cfg->footprint = SPLAT_FOOTPRINT_ELLIPSOID,
 * cfg->prelit = 1 (color_opacity is used as is), planes of stride 1 and the ellipsoid projector.  Both frame orders, record
 * formats PROJECTED and LIT32, projected == NULL and every screen the binner takes work as for a disc frame; AOV depth follows
 * the disc rules above (not with PROJECTED records and projected == NULL).  A strict band of tile rows is refused. */
int splat_render_frame_ellipsoids(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                                  const splat_composite_cfg *cfg, const float *uniforms, const void *positions,
                                  const void *scales, const void *rotations, const void *color_opacity, uint32_t n,
                                  uint32_t width, uint32_t height, void *projected, void *out_rgba8, void *out_rgba32f,
                                  const splat_aov *aov);

/* ---- antialiased frames of anisotropic 3D Gaussians: the 2D Mip filter (an extension; opt-in, nothing above changes) ----
 * Sigma2 = J Sigma3 J^T + 0.3 I draws a splat whose projected variance is far below a pixel with variance 0.3 px^2 and its
 * full opacity: many times the energy it should deposit.  The antialiased mode (Mip-Splatting's 2D filter, gsplat's
 * rasterize_mode = "antialiased") keeps the footprint and scales the opacity by
 *     rho = sqrt(det(Sigma2 - 0.3 I) / det Sigma2)
 * so that opacity * rho * 2 pi sqrt(det Sigma2) = opacity * 2 pi sqrt(det(Sigma2 - 0.3 I)): what the undilated Gaussian holds.
 * In binary32, from the projector's own a, b, c (csrc/ellipsoid.h states the order): a0 = |T0|^2 and c0 = |T1|^2
 * (a and c before their 0.3), det0 = a0 c0 - b b, rho = det0 > 0 ? sqrt(det0 / det) : 0; one rounding per operator, no contraction.
 * rho <= 1 always (no clamp is needed); rho = 0 for every splat whose record is all zeros (culled) and where det0 <= 0, which
 * binary32 cancellation produces for needle splats whose true det0 is tiny against a0 c0 (gsplat's float32 has the same).
 * The dilation stays 0.3 px^2.  The drawn opacity is fl32(opacity * rho); the record, the cut, the bounds, the keys and the
 * blend are the classic mode's.
 *
 * splat_project_ellipsoid_aa: splat_project_ellipsoid's arguments, checks and outputs (projected, records, keys and payload
 * byte for byte), then
 *   rho_out            n floats, 4-byte aligned, or NULL: rho per splat;
 *   color_opacity      (r, g, b, opacity) per splat, color_stride_vec4 float4s apart, 16-byte aligned, or NULL;
 *   color_opacity_out  n x float4, 16-byte aligned, or NULL: (r, g, b, fl32(opacity * rho)).  It requires color_opacity
 *                      (else SPLAT_ERR_INVALID).
 * One kernel, one thread per splat. */
int splat_project_ellipsoid_aa(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                               const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                               uint32_t n, void *projected, void *records, void *keys, void *payload, uint32_t n_padded,
                               void *rho_out, const void *color_opacity, uint32_t color_stride_vec4, void *color_opacity_out);
/* splat_render_frame_ellipsoids' arguments, checks and outputs (the AOVs included), antialiased: image and AOVs are bit for bit
 * those of splat_render_frame_ellipsoids given the plane (r, g, b, fl32(opacity * rho)).  That plane (16 bytes per splat) is
 * written by one pass of the antialiased projector into a buffer the ctx owns, then the classic frame runs on it.  With stage
 * timing on, a frame still records one SPLAT_STAGE_PROJECT interval (its projector's); the compensation pass is in no stage. */
int splat_render_frame_ellipsoids_aa(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                                     const splat_composite_cfg *cfg, const float *uniforms, const void *positions,
                                     const void *scales, const void *rotations, const void *color_opacity, uint32_t n,
                                     uint32_t width, uint32_t height, void *projected, void *out_rgba8, void *out_rgba32f,
                                     const splat_aov *aov);
/* The sampling rate Mip-Splatting's 3D smoothing filter is sized by (its compute_3D_filter), one camera per call:
 * with c = VP [p_i; 1] and the screen centre (sx, sy) formed as splat_project forms them (W = uniforms[20], H = uniforms[21]),
 *     rate_inout[i] = fmaxf(rate_inout[i], focal_px / c.w)   if c.w > near, fl32(-margin W) <= sx <= fl32((1 + margin) W) and
 *                                                             fl32(-margin H) <= sy <= fl32((1 + margin) H),
 * and rate_inout[i] is left as it is otherwise (a NaN fails the comparisons).  All binary32, one rounding per operator.
 * rate_inout: n floats, 4-byte aligned, read and written; positions: vec4 per splat, 16-byte aligned.  One thread per splat,
 * no atomics.  Start from zeros, call once per training camera; the 3D filter's sigma is then sqrt(variance) / rate. */
int splat_sampling_rate_max(splat_ctx *ctx, const float *uniforms, float focal_px, float near, float margin, const void *positions,
                            uint32_t pos_stride_vec4, uint32_t n, void *rate_inout);

/* ---- gradients of a frame of anisotropic 3D Gaussians (SPLAT_FOOTPRINT_ELLIPSOID; an extension) ------------------------
 * The backward of the staged ellipsoid frame: splat_project_ellipsoid -> sort -> splat_bin_run -> splat_composite_aov.  L is
 * the loss, G = (dL/drgb, dL/dalpha) per pixel.  Per pixel the forward takes its list in order with T_0 = 1, T_{i+1} =
 * T_i (1 - alpha_i), alpha_i = opacity_i exp(-4.5 d2) inside the record's cut (d2 = |B d|^2 <= 1) and 0 elsewhere, and stops
 * after the first entry with 1 - T_{i+1} >= 0.99; L_px entries are consumed.  rgb = sum T_i alpha_i c_i + T_L bg (bg =
 * (0.05, 0.05, 0.1)), alpha = 1 - T_L.  Gradients are those of this function with the cut and the stop held fixed (zero
 * outside the cut and for entries a pixel did not consume, as 3DGS treats its cut).  No 0.99 clamp of alpha is needed: every
 * consumed entry but a pixel's last has 1 - alpha > 0.01 (T_{i+1} > 0.01 and T_{i+1} <= 1 - alpha_i), and the last one's
 * T_{L-1} is recomputed front to back, never divided for.
 * The per-splat sums are float atomic adds whose order of arrival varies: gradients are reproducible to rounding, not bit for
 * bit, from run to run (splat_composite_backward_det, below, is the fixed-order form).
 *
 * splat_composite_backward: the lists (tile_indices / counts / offsets) must be the ones the forward composited, for the same
 * records (splat_project_ellipsoid's 32-byte records), color_opacity and screen.  grad_rgba32f: W*H float4, dL/drgb in xyz and
 * dL/dalpha in w.  ADDS into grad_records (n x 8 f32 per splat: c.x, c.y, B00, B01, -, B11, -, -; the unused columns are not
 * touched) and grad_color_opacity (n x 4 f32: r, g, b, opacity).  cfg must say footprint ELLIPSOID, FRONT_TO_BACK, early_out =
 * 1, tile_size = 16, record_format PROJECTED and the whole screen (tile_row0 = 0, tile_row1 >= the tile rows); anything else,
 * or a buffer not 16-byte aligned, is SPLAT_ERR_INVALID.  Every screen the binner takes works.
 * The backward follows the forward's kernel selection: it replays the transmittance updates and stop tests of the kernel
 * splat_composite_aov picks for this ctx and screen (splat_composite_options, else SPLAT_COMPOSITE, else k_composite_px on
 * screens of >= 2048 tiles), whose roundings differ where T lands within an ulp of the stop.  Differentiate on the ctx that
 * drew the frame, with its options unchanged; splat_composite_backward_depth does the same. */
int splat_composite_backward(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                             const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                             uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                             void *grad_color_opacity);
/* Gradients of the depth map (splat_composite_aov_depth's AOV depth).  Per pixel, over the entries it consumed (the cut and the
 * stop held fixed as above): w_i = T_i alpha_i, ws = sum w_i, zw = sum w_i z_i, D = zw / ws (+inf where ws = 0), z_i any
 * per-splat float the caller supplies (the ProjectedSplat depth, the distance from the eye to the centre, by default; not
 * view-space z).  With G_D = dL/dD:
 *   dL/dz_i = G_D w_i / ws;
 *   through alpha, D is a fifth channel of the recurrence above with colour z_i - D (centred), background 0 and upstream
 *   G_D / ws: cg_i = G_rgb . c_i + G_A + (G_D / ws)(z_i - D), dL/dalpha_i = T_i (cg_i - S_i), S as before.  Centred, because
 *   sum w_i (z_i - D) = 0 makes this the derivative of zw / ws, without the cancellation of G_A - (G_D / ws) D against
 *   (G_D / ws) z_i where the depth spread is much smaller than the depth.
 * G_D is not read where ws = 0: such a pixel has no gradient, and a NaN or inf upstream there is harmless.  Where ws is tiny the
 * gradient is large: that is the function's own gradient.  Sums are float atomics as above, reproducible to rounding only.
 *
 * splat_composite_backward_depth: splat_composite_backward's arguments and checks (every screen the binner takes) plus
 * depth_f32 / depth_stride_floats (the z the forward read: z_i = depth_f32[i * depth_stride_floats]), grad_depth_f32 (W*H
 * floats, dL/dD) and grad_depth (n floats, dL/dz, ADDED into).  NULL depth_f32 / grad_depth_f32 / grad_depth (n > 0), stride 0,
 * or one of the three not 4-byte aligned: SPLAT_ERR_INVALID. */
int splat_composite_backward_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                   const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                   uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                   void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                   const void *grad_depth_f32, void *grad_depth);
/* The two functions above with the per-splat sums in a fixed order: no float atomics anywhere, and the same inputs give the same
 * bits on every run, on every ctx.  Opt-in: it costs a workspace and a second pass, and the atomic entry points are unchanged.
 *
 * Arguments, checks and kernel selection are splat_composite_backward's (and, when any of depth_f32 / depth_stride_floats /
 * grad_depth_f32 / grad_depth is given, splat_composite_backward_depth's: all four NULL / 0 is the colour-only variant), plus
 *   projected    the ProjectedSplat array the lists were binned from (its bounds give each splat's tile rectangle, its depth
 *                the list order); 16-byte aligned;
 *   total_pairs  tile_offsets[num_tiles] (splat_bin_total); at most 2^32 - 1;
 *   workspace    a DEVICE pointer, 16-byte aligned, of workspace_bytes >= splat_composite_backward_det_workspace_bytes(
 *                total_pairs, num_tiles, n, with_depth) = 16 num_tiles + 16 ceil(n / 4) + 4 NV total_pairs bytes, NV = 9, or 10
 *                with depth (num_tiles = ceil(W / 16) ceil(H / 16)): a table row per tile, a slot index per splat and NV
 *                floats per pair.  Its content before the call does not matter and is unspecified after it.
 * A NULL projected, a NULL, misaligned or too small workspace, or total_pairs >= 2^32: SPLAT_ERR_INVALID, and nothing is launched.
 *
 * The sums.  Let P(i, t, k) be what one tile t adds for splat i and number k (k over c.x, c.y, B00, B01, B11, r, g, b, opacity,
 * and dL/dz with depth): the sum over the tile's 256 pixels that splat_composite_backward hands to its atomic add, formed in the
 * same order as there (each wave's DPP tree, then (w0 + w1) + (w2 + w3)).  Let [tx0, tx1] x [ty0, ty1] be splat i's tile
 * rectangle, the binner's: the tile range of projected[i].bounds on the whole screen, ntx tiles wide.  In binary32, one rounding
 * per add:
 *   row(ty)   = (((+0 + P(i, ty ntx + tx0, k)) + P(i, ty ntx + tx0 + 1, k)) + ...) + P(i, ty ntx + tx1, k)
 *   total     = ((+0 + row(ty0)) + row(ty0 + 1)) + ... + row(ty1)
 *   out[i][k] = prior[i][k] + total           (the "ADDS into" above, in one add)
 * A tile that did not consume splat i's entry (its position in the tile's list is at or past the largest L of the tile's
 * pixels) adds nothing.  A splat no tile consumed keeps its prior bits; so do the unused record columns.
 *
 * Lists that were not binned from this `projected` give unspecified gradients but no error and no store outside the buffers:
 * a list entry whose tile lies outside its splat's rectangle is dropped, and every slot index is bounded by total_pairs.
 * All work goes to the ctx's stream; nothing waits on the host. */
uint64_t splat_composite_backward_det_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth);
int splat_composite_backward_det(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                 const void *records, const void *projected, const void *tile_indices, const void *tile_counts,
                                 const void *tile_offsets, uint64_t total_pairs, uint32_t width, uint32_t height,
                                 const void *grad_rgba32f, uint32_t n, void *grad_records, void *grad_color_opacity,
                                 const void *depth_f32, uint32_t depth_stride_floats, const void *grad_depth_f32, void *grad_depth,
                                 void *workspace, uint64_t workspace_bytes);
/* The composite backwards with AbsGS's absolute screen-space gradient beside the signed one (Ye et al. 2024, "homodirectional
 * gradient"; gsplat's absgrad).  3DGS densifies by the norm of a splat's summed dL/dc; the sum is signed, so a large splat whose
 * pixels pull its centre in opposite directions cancels to a small statistic and is never split.  Summing |term| does not cancel.
 * Opt-in: the four functions above are unchanged, and these give their outputs plus
 *   grad_center_abs   n x 2 f32, 8-byte aligned, ADDED into: [i][0] = sum |term_cx|, [i][1] = sum |term_cy| over the (pixel,
 *                     consumed entry inside the cut) pairs of splat i, term_cx / term_cy being exactly the per-pair terms whose
 *                     signed sums go to grad_records[i][0] and [i][1] (so [i][k] >= |grad_records[i][k]| up to rounding).  A
 *                     splat no pixel consumed keeps its prior bits.  NULL with n > 0, or not 8-byte aligned: SPLAT_ERR_INVALID,
 *                     and nothing is launched.
 *
 * splat_composite_backward_abs: splat_composite_backward_depth's arguments plus grad_center_abs; as with the det entry point,
 * the four depth arguments all NULL / 0 select the colour-only variant (then splat_composite_backward's checks), any of them
 * given the depth variant with its checks.  The two absolute sums take the path of the other numbers (each wave's DPP tree under
 * the same ballot, (w0 + w1) + (w2 + w3), one float atomic add per touched (entry, number)): reproducible to rounding.
 *
 * splat_composite_backward_det_abs: splat_composite_backward_det's arguments plus grad_center_abs, the workspace sized by
 * splat_composite_backward_det_abs_workspace_bytes(total_pairs, num_tiles, n, with_depth) = 16 num_tiles + 16 ceil(n / 4) +
 * 4 NV total_pairs bytes with NV = 11, or 12 with depth (a smaller one: SPLAT_ERR_INVALID).  The numbers of a pair, in slot
 * order: c.x, c.y, B00, B01, B11, r, g, b, opacity, (dL/dz,) |c.x|, |c.y|.  The two new ones are summed as "The sums" above
 * states for the others: rows left to right from +0, the rows top to bottom from +0, then one add into grad_center_abs.  The
 * signed outputs are formed by the same additions in the same order as splat_composite_backward_det's: the same bits.
 *
 * All other checks, the kernel selection and the stream behaviour are those of the functions above.  The price: two more wave
 * sums per entry on top of nine or ten, and 8 more bytes per pair of the det workspace. */
int splat_composite_backward_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                 const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                 uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                 void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                 const void *grad_depth_f32, void *grad_depth, void *grad_center_abs);
uint64_t splat_composite_backward_det_abs_workspace_bytes(uint64_t total_pairs, uint32_t num_tiles, uint32_t n, int with_depth);
int splat_composite_backward_det_abs(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                     const void *records, const void *projected, const void *tile_indices, const void *tile_counts,
                                     const void *tile_offsets, uint64_t total_pairs, uint32_t width, uint32_t height,
                                     const void *grad_rgba32f, uint32_t n, void *grad_records, void *grad_color_opacity,
                                     const void *depth_f32, uint32_t depth_stride_floats, const void *grad_depth_f32, void *grad_depth,
                                     void *workspace, uint64_t workspace_bytes, void *grad_center_abs);
/* splat_project_ellipsoid's backward: dL/drecords (n x 8, splat_composite_backward's layout) -> dL/dposition (xyz, w = 0),
 * dL/dscale (xyz, w = 0) and dL/drotation (w, x, y, z of the quaternion as given, through its normalisation), all n x 4 f32,
 * OVERWRITTEN.  The centre and J move with the position.  The cull decisions are the forward's (csrc/ellipsoid.h); a culled
 * splat gets exact zeros.  Computed in float64 per splat. */
int splat_project_ellipsoid_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                     const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                     uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales, void *grad_rotations);
/* splat_project_ellipsoid_backward plus grad_depth (n floats, 4-byte aligned): dL/dz of the ProjectedSplat depth z = |p - eye|
 * (eye = uniforms[16..18]), whose term gz (p - eye) / |p - eye| is added, in float64, to dL/dposition.  A culled splat still
 * gets exact zeros, its depth term included.  Where grad_depth[i] = 0 the outputs are splat_project_ellipsoid_backward's bit for
 * bit. */
int splat_project_ellipsoid_backward_depth(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                           const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                           uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales,
                                           void *grad_rotations, const void *grad_depth);
/* splat_sh_colors' backward: dL/dcolor_opacity (n x 4) -> dL/dsh (same layout and stride as sh; the floats past
 * 3 (degree + 1)^2 in a row are not written), dL/dposition (n x 4, through dir = normalize(p - eye); w = 0) and dL/dopacity
 * (n floats: the fourth column passed through), OVERWRITTEN.  Zero colour gradient where the forward's max(., 0) clamped.
 * opacity_f32 is the forward's (not read; may be NULL). */
int splat_sh_colors_backward(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                             uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, const void *grad_color_opacity,
                             uint32_t n, void *grad_sh, void *grad_positions, void *grad_opacity);
/* Gradients of the camera.  A frame reads its 22-float uniform block {VP (16, column-major, m[4 k + r]), eye (3), time, W, H}
 * in three places: the records {c.x, c.y, B00, B01, B11} read rows 0, 1 and 3 of VP (through c = VP [p; 1] and the Jacobian J of
 * the screen position; row 2 is not read), the ProjectedSplat depth z = |p - eye| reads the eye (dz/deye = -(p - eye) / z), and
 * the SH direction normalize(p - eye) reads the eye (dL/deye = -sum_i dL/dp_i of the SH term).  time is not read; W and H are
 * the screen's integers, not parameters: no gradient is offered for them.  Sort keys and tile lists are decisions, not
 * differentiated; the cull, the cut and the stop are held fixed as above.
 * Unlike the per-splat sums above, these sums over all splats are bit-reproducible from run to run: each splat's numbers are
 * formed in float64 and summed in float64 in a fixed order (the 64 lanes of a wave; one partial per wave in a scratch buffer of
 * the ctx; then one summing kernel for up to 1024 partials, two above that: 64 contiguous slices of the partials, each added in
 * index order, then the slices in order) and rounded once to float32.  Which kernels run, and so the order, depends on n only.
 * Each is ONE sum over every splat the projector did not cull: a single splat whose own gradient is huge (an ill-conditioned
 * footprint, Sigma2 of condition number beyond 1e4, say) or a single non-finite upstream value reaches the whole camera
 * gradient, where it would spoil only its own row of the per-splat outputs.  A caller refining a pose masks such splats'
 * upstream (or makes them transparent) first.
 *
 * splat_project_ellipsoid_backward_camera: splat_project_ellipsoid_backward's arguments, checks and per-splat outputs
 * (grad_positions / grad_scales / grad_rotations bit for bit those of splat_project_ellipsoid_backward when grad_depth is NULL,
 * else of splat_project_ellipsoid_backward_depth), then grad_depth (n floats, 4-byte aligned, or NULL) and grad_uniforms: a
 * DEVICE pointer to 22 floats, 16-byte aligned, OVERWRITTEN (for n = 0 too: all zeros), laid out as the uniform block:
 * dL/dVP in [0, 16) (entries 2, 6, 10, 14, row 2, are exact zeros), dL/deye of the depth term in [16, 19) (zeros when grad_depth
 * is NULL), zeros in [19, 22).  A culled splat contributes exact zeros.  NULL or misaligned grad_uniforms: SPLAT_ERR_INVALID. */
int splat_project_ellipsoid_backward_camera(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                            const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                            uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales,
                                            void *grad_rotations, const void *grad_depth, void *grad_uniforms);
/* The backward of splat_project_ellipsoid_aa: splat_project_ellipsoid_backward_camera's arguments, of which grad_depth AND
 * grad_uniforms may be NULL here (NULL grad_uniforms: no camera sums run), then grad_rho: n floats, 4-byte aligned, dL/drho.
 * The same float64-per-splat kernel; with rho^2 = det0 / det, A0 = A - 0.3, C0 = C - 0.3 the term
 *     drho/dA = (C0 / det - rho^2 C / det) / (2 rho),  drho/dC = (A0 / det - rho^2 A / det) / (2 rho),
 *     drho/dB = (-2 B / det)(1 - rho^2) / (2 rho)
 * times grad_rho joins dL/d(A, B, C) and the existing chain carries it to position, scale, rotation and the camera sums (rho
 * reads VP through J only).  Where the forward's binary32 rho is 0 (culled, or det0 <= 0) the term is exactly zero: rho is not
 * differentiable there.  Where grad_rho[i] = 0 the per-splat outputs are bit for bit those of the entry point above with the
 * same grad_depth / grad_uniforms choice; with all of grad_rho zero so is grad_uniforms.  The camera sums keep their fixed
 * order: bit-reproducible from run to run. */
int splat_project_ellipsoid_backward_aa(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                        const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                        uint32_t n, const void *grad_records, void *grad_positions, void *grad_scales,
                                        void *grad_rotations, const void *grad_depth, void *grad_uniforms, const void *grad_rho);
/* splat_sh_colors_backward's arguments, checks and outputs (bit for bit), then grad_eye: a DEVICE pointer to 4 floats, 16-byte
 * aligned, OVERWRITTEN (for n = 0 too) with dL/deye in xyz and 0 in w: minus the float64 sum of the splats' grad_positions. */
int splat_sh_colors_backward_camera(splat_ctx *ctx, const float *eye3, const void *positions, uint32_t pos_stride_vec4, const void *sh,
                                    uint32_t sh_stride_floats, uint32_t degree, const void *opacity_f32, const void *grad_color_opacity,
                                    uint32_t n, void *grad_sh, void *grad_positions, void *grad_opacity, void *grad_eye);

/* ---- 2D Gaussian surfels (SPLAT_FOOTPRINT_SURFEL; an extension, no reference counterpart; 2DGS, Huang et al. 2024) ---------
 * A surfel is the ellipsoid's four planes read differently: position xyz, scales (x and y used: standard deviations along the
 * tangent axes; z and w ignored), rotation quaternion (w, x, y, z) of any non-zero length, colour and opacity.  Its tangent axes
 * are columns 0 and 1 of R(q), its normal column 2, its half-axes e0 = 3 s.x R[:,0], e1 = 3 s.y R[:,1]: a planar quad, whose
 * 8-float record {c.x, c.y, B00, B01, B10, B11, q0, q1} is the oriented disc's (splat_project_disc) from the half-axes on.  Per
 * pixel, (u, v) = B d / (1 - q.d), d = pixel centre - c, is the exact ray-surfel intersection in the surfel's coordinates (no
 * affine approximation), the record's unit circle is the 3-sigma cut, and alpha = opacity exp(-4.5 (u^2 + v^2)): the
 * ellipsoid's exponent.  The record is all zeros (culled) when a corner of the 3-sigma quad has clip w <= 0, when det == 0 (an
 * edge-on surfel, a zero scale), when the quaternion is zero and when anything is not finite.  Binary32, one IEEE operation per
 * operator in the order stated in csrc/surfel.h.
 *
 * splat_project_surfel: splat_project_ellipsoid's arguments and checks.  Writes `records` (n x 8 floats), `projected` (bounds:
 * the record's exact screen extent; depth |p - eye|, as splat_project: surfels sort by the distance to their centre;
 * screenRadius half the larger extent), keys and payload exactly as splat_project_ellipsoid, and, when clip_w_out is not NULL
 * (n floats, 4-byte aligned), the centre's clip w (0 for a culled surfel).
 *
 * Forward images need no kernel of their own: a surfel frame is sort -> bin -> splat_composite / splat_composite_aov with
 * cfg->footprint = SPLAT_FOOTPRINT_SURFEL over these records, which runs the ellipsoid's kernels (they evaluate B10 and q of
 * every record): the same bits as cfg->footprint = SPLAT_FOOTPRINT_ELLIPSOID over the same records.  splat_composite_aov's depth
 * stays the blend of one number per splat, as for every footprint.
 *
 * The intersection depth.  With c = VP [P; 1] for the plane point P = p + u e0 + v e1 a pixel sees, c.w = cw / (1 - q.d), cw the
 * centre's clip w: a pixel's depth on surfel i is z_i rd_i, rd = 1 / (1 - q.d), the reciprocal the footprint already forms.
 * splat_composite_surfel_depth: one walk of the frame's lists writes D = sum w_i z_i rd_i / sum w_i over the entries the pixel
 * consumed (w_i = T_i alpha_i, the image's own weights and stop), +inf where nothing contributed, to out_depth_f32 (W x H
 * floats), and 1 - T to out_alpha_f32 when that is not NULL.  z_i = depth_f32[i * depth_stride_floats]: the caller's float, by
 * default clip_w_out, which makes D the clip w of the blended intersections (SPLAT_DEPTH_Z for splat_depth_normals).  cfg:
 * footprint SURFEL, FRONT_TO_BACK, early_out = 1, tile_size = 16, PROJECTED records, the whole screen.
 *
 * Gradients.  splat_composite_backward and splat_composite_backward_depth take cfg->footprint = SPLAT_FOOTPRINT_SURFEL: the
 * contract above (the cut and the stop held fixed, float atomic sums ADDED into the outputs, the drawing kernel's operation
 * order by splat_composite_options), with gradients to all eight record columns.  _depth differentiates the intersection depth
 * map D above (not the centre blend): grad_depth receives dL/dz_i, and the q and c columns the terms through rd.  Every other
 * splat_composite_features and splat_composite_features_backward take it too ("Feature channels of a frame", below): the same
 * contract with the surfel's alpha, the map blended with the surfel image's own weights, the record gradient in all eight
 * columns.  Every other entry point that takes a cfg and replays a frame refuses SPLAT_FOOTPRINT_SURFEL with SPLAT_ERR_INVALID
 * and a message naming it (the _det, _abs and _det_abs backwards, splat_composite_contribution): their kernels take B10 = 0
 * and q = 0, and none runs with q ignored.  The ellipsoid's projector entry points (the _aa projector, the
 * _camera backwards) take no cfg: a surfel's planes given to them are projected as an ellipsoid's.
 *
 * Depth distortion (2DGS's and Mip-NeRF 360's regulariser, over the intersection depth).  With 0 < near < far (far = +inf
 * allowed; anything else is SPLAT_ERR_INVALID) and t_i = z_i rd_i the depth above, m_i = far (t_i - near) / ((far - near) t_i)
 * maps depth to [0, 1) (far = +inf: m_i = 1 - near / t_i), and per pixel
 *     Dist = sum_{i > j} w_i w_j (m_i - m_j)^2
 * over the entries the pixel consumed that are inside the cut and whose t_i is finite and > 0; an entry inside the cut whose
 * t_i is not draws the image as before, takes no part in Dist and receives nothing from it.  0 where nothing took part.  It is
 * formed front to back, Dist += w_i (m'_i^2 A + Q - 2 m'_i M), then A += w_i, M += w_i m'_i, Q += w_i m'_i^2, over
 * m'_i = m_i - m_first, m_first the m of the pixel's first participating entry: the term depends on differences only, and the
 * sums of unshifted m's (or W Q - M^2) cancel four digits away in binary32.  m'_i is formed as c (1 / t_first - 1 / t_i),
 * c = near far / (far - near) (near when far = +inf): the same difference without its common constant.  One binary32
 * rounding per operator in the order stated in csrc/surfel.h.
 * splat_composite_surfel_distortion: splat_composite_surfel_depth's arguments and cfg, then near, far and out_distortion_f32
 * (W x H floats, 4-byte aligned).  One walk, one launch; out_depth_f32 and out_alpha_f32 are each optional here, and what they
 * receive is bit for bit what splat_composite_surfel_depth writes.
 * splat_composite_backward_distortion: splat_composite_backward_depth's arguments, contract and cfg (footprint SURFEL only),
 * then near, far and grad_distortion_f32 (W x H floats: dL/dDist; not read where nothing took part).  One launch adds the
 * image's, the depth map's and the distortion's gradients: through the weights Dist is one more colour channel with the
 * per-entry colour e_i = sum_j w_j (m_i - m_j)^2 and background 0, and through m_i, with dm/dt = c / t^2, dL/dt_i = dL/dDist
 * 2 w_i (m'_i W - M) c / t_i^2 joins the depth map's term: grad_depth receives dL/dz_i, and all eight record columns their
 * share.  grad_depth_f32 may be NULL here (no depth-map term).  With grad_distortion_f32 all zeros the outputs are
 * splat_composite_backward_depth's, to the order of the atomic sums.  Both refuse every other footprint with a message.
 *
 * splat_project_surfel_backward: per splat, in float64, the chain of csrc/surfel.h reversed.  grad_records (n x 8 floats) and
 * grad_clip_w (n floats, or NULL: zeros) in; grad_positions, grad_scales (x and y; z and w exactly 0) and grad_rotations
 * (through the quaternion's normalisation) OVERWRITTEN, n x 4 floats each.  The cull is the projector's own: a culled surfel
 * gets exact zeros. */
int splat_project_surfel(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4, const void *scales,
                         uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4, uint32_t n, void *projected,
                         void *records, void *keys, void *payload, uint32_t n_padded, void *clip_w_out);
int splat_composite_surfel_depth(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                 const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                 uint32_t width, uint32_t height, const void *depth_f32, uint32_t depth_stride_floats, uint32_t n,
                                 void *out_depth_f32, void *out_alpha_f32);
int splat_composite_surfel_distortion(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                      const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                      uint32_t width, uint32_t height, const void *depth_f32, uint32_t depth_stride_floats, uint32_t n,
                                      void *out_depth_f32, void *out_alpha_f32, float near, float far, void *out_distortion_f32);
int splat_composite_backward_distortion(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                        const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                        uint32_t width, uint32_t height, const void *grad_rgba32f, uint32_t n, void *grad_records,
                                        void *grad_color_opacity, const void *depth_f32, uint32_t depth_stride_floats,
                                        const void *grad_depth_f32, void *grad_depth, float near, float far,
                                        const void *grad_distortion_f32);
int splat_project_surfel_backward(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                                  const void *scales, uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4,
                                  uint32_t n, const void *grad_records, const void *grad_clip_w, void *grad_positions, void *grad_scales,
                                  void *grad_rotations);

/* ---- Contribution of every splat to a frame: hit count, largest and summed blend weight (an extension) --------------------
 * Which splats does a view actually see, and how much?  RadSplat prunes a fit on the largest blend weight a splat reaches in any
 * training view, LightGaussian on hit counts, Mini-Splatting on summed weights: all three are per-splat reductions of one
 * forward walk of the frame's tile lists.  One call scores one view; the outputs ACCUMULATE, so a call per view builds the
 * statistic over views (the caller zeroes the buffers before the first).
 *
 * The pair and its weight.  Per pixel, over the entries it consumed (up to and including the one its early-out stopped at, as
 * for the gradients above): w_i = T_i alpha_i for an entry inside the record's cut.  (pixel, entry) is then a pair.  An entry
 * outside the cut or past the stop is no pair.  w_i is formed in the operation order of the kernel that draws this frame on this
 * ctx (splat_composite_backward's rule, above: k_composite's w = T (g opacity), or k_composite_px's w = (T g) opacity with
 * T = fma(-opacity, T g, T)): score a view on the ctx that draws it, with its options unchanged.
 * The pixel mask.  m = pixel_weight_f32[y W + x] clamped to [0, 1], NaN -> 0; m = 1 everywhere when the pointer is NULL.
 * wm = m w in binary32 (clamped to [0, 1], NaN -> 0: that changes nothing for opacities in [0, 1]).  A pixel with m = 0
 * contributes to no output and counts no hit.
 * The outputs, n entries each; each may be NULL (not wanted), not all three:
 *   weight_max_f32[i] = max(prior, max over the splat's pairs of wm)                                   (float32)
 *   weight_sum_u64[i] += sum over its pairs of q, q = (uint32) rintf(wm 2^24): fixed point in units of 2^-24  (uint64; q <= 2^24)
 *   hits_u32[i]       += the number of its pairs with wm >= min_weight; the count wraps at 2^32         (uint32)
 * min_weight >= 0 (0: every pair is a hit); negative or NaN is SPLAT_ERR_INVALID.  A splat in no pair with m > 0 keeps its prior
 * bytes in all three.
 * Bit reproducibility.  The maximum of non-negative floats (taken on their bit patterns, which order as the values do), integer
 * sums and integer counts do not depend on the order they are formed in: the same inputs give the same bytes on every run.  That
 * is why the sum is fixed point and not a float: a float sum over atomics would depend on their arrival order.  No float atomic
 * is used anywhere.  (Each pair's q is within 2^-25 of wm; a sum of P pairs is within P 2^-25 of the sum of the wm.)
 *
 * splat_composite_contribution: splat_composite_backward's frame arguments and checks (footprint ELLIPSOID, FRONT_TO_BACK,
 * early_out = 1, tile_size = 16, PROJECTED records, the whole screen; the lists the forward composited, on the ctx that drew the
 * frame; every screen the binner takes).  color_opacity / records 16-byte aligned, weight_sum_u64 8-byte, the lists,
 * pixel_weight_f32, hits_u32 and weight_max_f32 4-byte; a misaligned or NULL required pointer, or all three outputs NULL, is
 * SPLAT_ERR_INVALID and nothing is launched.  n = 0: success, nothing launched.  All work goes to the ctx's stream; nothing
 * waits on the host. */
int splat_composite_contribution(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                                 const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                                 uint32_t width, uint32_t height, const void *pixel_weight_f32 /* W*H floats or NULL */, float min_weight,
                                 uint32_t n, void *hits_u32, void *weight_max_f32, void *weight_sum_u64);

/* ---- Feature channels of a frame: per-splat floats blended with the image's own weights, with gradients (an extension) -------
 * Normals for a normal-consistency term, (1, z, z^2) for a depth-distortion regulariser, learned embeddings, an expected depth
 * that is not divided by sum w: anything a caller wants blended with the weights w_i = T_i alpha_i of the staged ellipsoid frame
 * that splat_composite_backward differentiates.  The lists, the cut, the stop and the kernel selection (composite_uses_px) are
 * that frame's.  Each splat carries K = `channels` floats f_i[0..K), 1 <= K <= SPLAT_MAX_FEATURE_CHANNELS, at
 * features_f32[i * feature_stride_floats + k]; feature_stride_floats >= channels, so a column slice of a wider tensor can be
 * passed as it lies.
 *
 * Forward.  Per pixel, over the entries it consumed (up to and including the one its early-out stopped at):
 *   F[k] = sum_i w_i f_i[k],
 * w_i formed in the operation order of the kernel that draws this frame on this ctx, exactly as splat_composite_contribution
 * defines its weight (above).  There is no background term and no division by sum w; F is 0 where nothing contributed.
 * out_f32[(y W + x) * channels + k], W H channels floats, is WRITTEN at every pixel of the screen.
 * Backward.  With G_F = dL/dF per pixel (grad_out_f32, laid out as out_f32), the cut and the stop held fixed:
 *   dL/df_i[k] = sum over pixels of w_i G_F[k]
 *   s_i = G_F . f_i (all K channels),  dL/dalpha_i = T_i (s_i - S_i),  S_{i-1} = alpha_i s_i + (1 - alpha_i) S_i,
 * S = 0 behind the last consumed entry (the background of every feature is 0); T_i as in splat_composite_backward (T_{L-1} kept
 * from the forward walk, T_i = T_{i+1} / (1 - alpha_i) elsewhere).  dL/dalpha_i goes on to the record's five numbers and to the
 * opacity by splat_composite_backward's formulas.  The recurrence is linear in the upstream: this is the feature loss's own
 * additive share of grad_records and of the opacity column, to be added to splat_composite_backward's for a loss that has both.
 *   grad_records        n x 8 floats: ADDED into columns 0, 1, 2, 3, 5 (c.x, c.y, B00, B01, B11); columns 4, 6, 7 not touched
 *   grad_color_opacity  n x 4 floats: ADDED into column 3 only; columns 0 - 2 not touched
 *   grad_features_f32   ADDED into [i * grad_feature_stride_floats + k], k < channels; floats past `channels` of a row not touched
 * The sums are float atomic adds: reproducible to rounding, NOT bit for bit (no fixed-order variant exists).
 * One pass for any K: the kernels are instantiated for K rounded up to 1, 2, 3, 4, 6, 8, 12, 16, 24 or 32.  Measured on one MI355X
 * at 5 M splats, 1920x1080: forward 0.35 ms at K = 3, 0.37 at K = 8 (splat_composite_contribution: 0.42);
 * backward 1.13 ms at K = 3, 1.35 at K = 8 (splat_composite_backward: 1.10).
 *
 * Both: splat_composite_backward's frame arguments and checks (footprint ELLIPSOID, FRONT_TO_BACK, early_out = 1, tile_size = 16,
 * PROJECTED records, the whole screen, every screen the binner takes).  color_opacity / records / grad_records /
 * grad_color_opacity 16-byte aligned; the lists and every feature pointer 4-byte.  SPLAT_ERR_INVALID, nothing launched: channels
 * 0 or above SPLAT_MAX_FEATURE_CHANNELS, a stride below channels, a NULL or misaligned required pointer.  n = 0: the forward
 * writes zeros, the backward is success with nothing launched (features / the gradient planes may then be NULL).  All work goes
 * to the ctx's stream; nothing waits on the host. */
#define SPLAT_MAX_FEATURE_CHANNELS 32
int splat_composite_features(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity, uint32_t color_stride_vec4,
                             const void *records, const void *tile_indices, const void *tile_counts, const void *tile_offsets,
                             uint32_t width, uint32_t height, const void *features_f32, uint32_t feature_stride_floats,
                             uint32_t channels, uint32_t n, void *out_f32 /* W*H*channels floats */);
int splat_composite_features_backward(splat_ctx *ctx, const splat_composite_cfg *cfg, const void *color_opacity,
                                      uint32_t color_stride_vec4, const void *records, const void *tile_indices, const void *tile_counts,
                                      const void *tile_offsets, uint32_t width, uint32_t height, const void *features_f32,
                                      uint32_t feature_stride_floats, uint32_t channels, const void *grad_out_f32 /* W*H*channels */,
                                      uint32_t n, void *grad_records /* n x 8 */, void *grad_color_opacity /* n x 4 */,
                                      void *grad_features_f32, uint32_t grad_feature_stride_floats);

/* ---- Image loss: the photometric objective of 3D Gaussian splatting (an extension) -----------------------------------------
 * How far a rendered image x is from a target y, both width x height pixels of 3 float32 channels:
 *   loss = (1 - lambda) l1 + lambda (1 - ssim),   l1 = mean |x - y|,   ssim = mean m,   both means over all N = 3 W H values.
 * With g the normalised 1-D window g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), k = 0..10, sum g = 1, and conv(.) the separable 11 x 11
 * convolution with g (x) g, per channel, ZERO padding (same output size as its input; its own adjoint):
 *   mu_x = conv(x), mu_y = conv(y), s_x = conv(x x) - mu_x^2, s_y = conv(y y) - mu_y^2, s_xy = conv(x y) - mu_x mu_y,
 *   A = 2 mu_x mu_y + C1, B = 2 s_xy + C2, C = mu_x^2 + mu_y^2 + C1, D = s_x + s_y + C2, C1 = 0.01^2, C2 = 0.03^2,
 *   m = A B / (C D).
 * The gradient with respect to x (none is offered for the target):
 *   dm/dmu_x = 2 mu_y B / (C D) - 2 mu_x m / C - 2 mu_y A / (C D) + 2 mu_x m / D,  dm/ds_x = -m / D,  dm/ds_xy = 2 A / (C D),
 *   dloss/dx = (1 - lambda) sign(x - y) / N - (lambda / N) [conv(dm/dmu_x) + 2 x conv(dm/ds_x) + y conv(dm/ds_xy)],
 * sign(0) = 0.  x is not clamped (a composite may exceed 1).  Images smaller than the window are legal, down to 1 x 1.
 *
 * An image is (pointer, pixel stride in floats >= 3): pixel p's channels are the first three floats at pointer + p * stride,
 * pixels in row-major order without row padding.  The float4 image of splat_composite_aov is (out_rgba32f, 4), read in place; a
 * packed RGB image is (ptr, 3).  A fourth word may be loaded but never enters a result (NaN there is harmless); of the
 * gradient's pixels only the first three floats are written.  Pointers are 4-byte aligned, the workspace 16-byte.
 *
 * splat_image_loss writes out4 (DEVICE, 4 floats) = {loss, l1, ssim, 0}.  The two sums are made without atomics: each
 * workgroup's float64 partial goes to a slot of its own in a scratch buffer of the ctx and one small kernel adds the slots in
 * index order and rounds once, so the same inputs give the same bits.  `workspace` (DEVICE, at least
 * splat_image_loss_workspace_bytes(width, height) = 36 W H bytes rounded up to 16) receives the three derivative maps for
 * splat_image_loss_backward.  lambda = 0 with workspace == NULL runs the L1 part alone: ssim is then NaN (not computed) and
 * loss = l1; lambda = 0 with a workspace computes all three.
 * splat_image_loss_backward OVERWRITES the first three floats of every pixel of (grad_image, grad_stride) with `upstream[0]`
 * (DEVICE, one float: dL/dloss, read on the device so that no caller has to synchronise) times dloss/dx.  image, target,
 * strides, size and lambda must be those of the splat_image_loss call that filled `workspace`; with lambda = 0 the workspace
 * is not read and may be NULL.  It is a gather with no atomics: bit-reproducible.
 * Nothing here waits on the host; all work goes to the ctx's stream.
 * SPLAT_ERR_INVALID: a NULL image, target, out4, upstream or grad_image; width or height 0 or above 65535; a stride below 3;
 * lambda outside [0, 1] (or NaN); a misaligned pointer; a workspace that is needed and NULL or smaller than
 * splat_image_loss_workspace_bytes. */
uint64_t splat_image_loss_workspace_bytes(uint32_t width, uint32_t height);
int splat_image_loss(splat_ctx *ctx, const void *image, uint32_t image_stride, const void *target, uint32_t target_stride,
                     uint32_t width, uint32_t height, float lambda, void *workspace, uint64_t workspace_bytes, void *out4);
int splat_image_loss_backward(splat_ctx *ctx, const void *image, uint32_t image_stride, const void *target, uint32_t target_stride,
                              uint32_t width, uint32_t height, float lambda, const void *workspace, uint64_t workspace_bytes,
                              const void *upstream, void *grad_image, uint32_t grad_stride);

/* ---- Normals of a depth map: the surface a depth map describes, and 2DGS's normal-consistency loss (an extension) -------------
 * Rays.  VP is the uniform block's matrix (VP[r][c] = uniforms[4 c + r], as pinhole_uniforms and Camera store it); M is the 3 x 3
 * of its rows 0, 1, 3 acting on xyz and m their fourth column.  A pinhole camera has M eye + m = 0, and the point seen at pixel
 * centre (x + 1/2, y + 1/2) with clip w = s is eye + s d(x, y),
 *   d(x, y) = M^-1 (2 (x + 1/2) / W - 1, 1 - 2 (y + 1/2) / H, 1)^T = D0 + x Dx + y Dy,
 * affine in the pixel index.  The host computes D0, Dx, Dy in float64 and the handedness sign
 *   sigma = -sign((Dy x Dx) . d_c),  d_c = M^-1 (0, 0, 1) the ray of the screen's centre,
 * with which every normal below faces the eye (N . d < 0) whether or not the camera mirrors an axis.  A camera whose M is
 * singular (|det M| <= 1e-14 |row 0| |row 1| |row 3|: an orthographic VP is one) or whose sigma is 0 is refused with
 * SPLAT_ERR_INVALID, and splat_last_error says which.  uniforms[16..21] are not read by the device entry points (the eye cancels:
 * a normal is a difference of points; the screen is the width and height arguments).
 *
 * Ray parameter.  depth_kind says what the depth map holds: SPLAT_DEPTH_DISTANCE, |P - eye| (what splat_project_ellipsoid's depth
 * and so the AOV depth of a Gaussian frame are): s = depth / |d|;  SPLAT_DEPTH_Z, clip w (planar depth): s = depth.
 *
 * Normal at pixel p = (x, y), from the ray parameters s_l, s_r, s_u, s_d of (x-1, y), (x+1, y), (x, y-1), (x, y+1):
 *   a_x = (s_r - s_l) d(p) + (s_r + s_l) Dx,   a_y = (s_d - s_u) d(p) + (s_d + s_u) Dy,   n = sigma (a_y x a_x),   N = n / |n|:
 * the central difference P(x+1) - P(x-1) of 2DGS's depth_to_normal, written with d affine so that only the depth difference
 * cancels, not two world points.  The kernels evaluate the same n with the cross product expanded,
 *   n = sigma [(s_d - s_u)(s_r + s_l) d x Dx + (s_d + s_u)(s_r - s_l) Dy x d + (s_d + s_u)(s_r + s_l) Dy x Dx]
 * (the d x d term is zero and is not formed), in binary32 from ray parameters rounded once; 1 / |d| and the three cross products
 * are made in float64.
 * Validity.  N = (0, 0, 0), and the pixel passes no gradient, unless 1 <= x <= W - 2 and 1 <= y <= H - 2, all four neighbour
 * depths are finite and > 0 (an empty pixel of the AOV depth is +inf), and |n|^2 is finite and > 0.  The pixel's own depth is not
 * read.  Screens with W < 3 or H < 3 are legal and give all zeros.
 *
 * splat_depth_normals WRITES the first three floats of every pixel of (normals, normal_stride) (an image as the image loss
 * defines one: pixel stride in floats >= 3, other words not touched).
 * splat_depth_normals_backward OVERWRITES grad_depth (W H floats) with dL/ddepth given dL/dN (grad_normals, grad_stride).  A
 * depth pixel q enters the normals of q + (1, 0), q - (1, 0), q + (0, 1), q - (0, 1) (as their left, right, upper, lower
 * neighbour); the up to four contributions are gathered and added in that order, then multiplied by ds/ddepth: no atomics, the
 * same bits on every run.  A pixel whose depth is not finite gets exactly 0.  The upstream of an invalid pixel is not read (it
 * is selected away, not multiplied by zero): NaN or inf there reaches nothing.  The camera gets no gradient.
 *
 * The loss, 2DGS's normal_error.mean():  L = (1 / (W H)) sum_p (1 - w_p F_p . N_p),  F the blended normal map (normal_map,
 * map_stride: an (H, W, K) feature map whose first three channels are the normal is read in place), w an optional W H weight
 * (2DGS: the detached alpha; NULL: 1).  An invalid pixel contributes the constant 1, and its F and w are not read.
 * splat_normal_consistency writes out4 (DEVICE, 4 floats) = {L, fraction of valid pixels, 0, 0}; the sum is made of float64
 * per-workgroup partials in a scratch buffer of the ctx, added in index order by one small kernel and rounded once.
 * splat_normal_consistency_backward, one launch, with g = upstream[0] (DEVICE, one float, read on the device):
 *   dL/dF_p = -(g / (W H)) w_p N_p   OVERWRITES the first three floats of every pixel of (grad_map, grad_map_stride) (0 at an
 *                                    invalid pixel; other words not touched),
 *   dL/ddepth                        OVERWRITES grad_depth, splat_depth_normals_backward's gather with dL/dN_p = -(g / (W H)) w_p F_p.
 * w gets no gradient.
 *
 * splat_camera_rays: host only, no ctx, no device: out10 = {D0, Dx, Dy, sigma} in float64 for the screen uniforms[20], [21].
 * All device work goes to the ctx's stream; nothing waits on the host; no caller workspace.  SPLAT_ERR_INVALID, nothing
 * launched: a NULL pointer (weight may be NULL), width or height 0 or above 65535, a stride below 3, an unknown depth_kind, a
 * pointer that is not 4-byte aligned, a refused camera. */
#define SPLAT_DEPTH_DISTANCE 0u
#define SPLAT_DEPTH_Z 1u
int splat_camera_rays(const float *uniforms, double *out10);
int splat_depth_normals(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, uint32_t width, uint32_t height,
                        void *normals, uint32_t normal_stride);
int splat_depth_normals_backward(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, uint32_t width,
                                 uint32_t height, const void *grad_normals, uint32_t grad_stride, void *grad_depth);
int splat_normal_consistency(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth, const void *normal_map,
                             uint32_t map_stride, const void *weight, uint32_t width, uint32_t height, void *out4);
int splat_normal_consistency_backward(splat_ctx *ctx, const float *uniforms, uint32_t depth_kind, const void *depth,
                                      const void *normal_map, uint32_t map_stride, const void *weight, uint32_t width, uint32_t height,
                                      const void *upstream, void *grad_map, uint32_t grad_map_stride, void *grad_depth);

/* ---- TSDF fusion and mesh extraction: from depth maps to a surface (an extension) ---------------------------------------------
 * What 2DGS, GOF, RaDe-GS and PGSR do with a finished fit: render its depth from the training cameras, fuse the maps into a
 * truncated signed distance volume, pull a triangle mesh out of it.  No kernel here uses atomics and every sum has a fixed
 * order: the same inputs give the same bytes on every run.
 *
 * The volume is a grid of nx x ny x nz NODES, dims = {nx, ny, nz}; node (i, j, k) sits at origin + voxel (i, j, k) and has the
 * linear index i + nx (j + ny k).  LIMITS: 1 <= nx, ny, nz <= 2048 and nx ny nz <= 2^30; anything beyond is refused.  It lives in
 * caller-owned DEVICE planes: tsdf, one float per node, the signed distance over trunc, in [-1, 1]; weight, one float per node,
 * 0 = never observed; color, optional, 3 floats per node (node-major).  A fresh volume is weight = 0 everywhere: the tsdf and
 * colour of a node of weight 0 are never read, so nothing else needs clearing.
 *
 * splat_tsdf_integrate fuses one view: uniforms (the block splat_depth_normals reads: VP[r][c] = uniforms[4 c + r], the eye in
 * [16..18]; [19..21] are not read), depth_kind (SPLAT_DEPTH_DISTANCE, |X - eye|, what the AOV depth of a Gaussian frame is, or
 * SPLAT_DEPTH_Z, clip w), a width x height depth map, an optional width x height observation weight (obs_weight; NULL: 1), an
 * optional image (pixel stride image_stride >= 3 floats, the first three read) and max_weight.  Per node X, in binary32, every
 * quantity formed from (i, j, k) alone (X_c = fma(voxel, i_c, origin_c)), so that the result does not depend on how the grid is
 * walked:
 *   1. clip = VP (X, 1), each row fma(VP[r][0], x, fma(VP[r][1], y, fma(VP[r][2], z, VP[r][3])));  skip unless clip.w > 0.
 *   2. u = (clip.x / clip.w * 0.5 + 0.5) W,  v = (0.5 - 0.5 clip.y / clip.w) H: continuous pixel coordinates, pixel (x, y)'s
 *      centre at (x + 1/2, y + 1/2), the convention of the rays in "Normals of a depth map".
 *   3. ix = floor(u), iy = floor(v);  skip unless 0 <= u < W and 0 <= v < H.
 *   4. D = depth[iy W + ix];  skip unless D is finite and > 0 (an empty pixel of the AOV depth is +inf).
 *   5. a = obs_weight[iy W + ix], skip unless a > 0;  without a map a = 1.  (a must be finite.)
 *   6. r = |X - eye| (DISTANCE) or clip.w (Z): the node's own depth in the map's unit.
 *   7. s = D - r;  skip if s < -trunc (the node is hidden behind the surface by more than the band).
 *   8. f = min(1, s / trunc),  w' = w + a.
 *   9. tsdf = (tsdf w + f a) / w';  with both color and image given, color_c = (color_c w + image_c a) / w' likewise.  (w = 0: the
 *      old value is taken as 0 without reading it.)
 *  10. weight = max_weight > 0 ? min(w', max_weight) : w'.
 * A node that is skipped is not written.  The kernel works in bricks of 32 x 4 x 4 nodes and leaves a brick without a load when
 * its eight corner nodes are all behind the eye, or all safely in front of it and beyond the same side of the screen by more
 * than a pixel; the margins exceed the binary32 error of steps 1-3, so the cull never changes a byte.
 *
 * The mesh is marching tetrahedra on the Kuhn split: the cube with lower corner (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is
 * cut into six tetrahedra, one per permutation pi of the axes, numbered by the lexicographic order of pi: v0 = (0,0,0),
 * v1 = v0 + e_pi1, v2 = v1 + e_pi2, v3 = (1,1,1).  All six share the body diagonal and every cube face is cut by the diagonal
 * from its lowest to its highest corner, so neighbouring cubes agree and the surface has no cracks.
 *   Nodes.     VALID: weight > min_weight (a NaN weight is invalid).  INSIDE: tsdf < 0 (exactly 0, -0 and NaN are outside).
 *   Cubes.     MESHED only when all eight corners are valid.
 *   Edges.     Every tetrahedron edge is owned by its lower node and has one of 7 directions, numbered 0-6:
 *              (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).
 *   Vertices.  One on an edge exactly when its endpoints differ in the inside test and at least one of the cubes the edge lies
 *              in (four for an axis edge, two for a face diagonal, one for the body diagonal) is meshed: no vertex is left
 *              unreferenced.  Position p0 + t (p1 - p0), t = f0 / (f0 - f1) from the lower endpoint, as fma(t, p1 - p0, p0) per
 *              component with p = fma(voxel, index, origin); the colour likewise from the endpoints' colours.  A shared vertex is
 *              one value, not one per triangle.  Ordered by (owning node's linear index, edge number).
 *   Triangles. Ordered by (cube's lower-corner linear index, tetrahedron number, triangle number).  A tetrahedron with one or
 *              three inside vertices gives one triangle; with two, a quad: its four vertices are taken in the cyclic order that
 *              runs counter-clockwise seen from outside, starting at the smallest vertex id q0, and split along the diagonal
 *              from it: (q0, q1, q2) then (q0, q2, q3).  Every triangle starts at its smallest vertex id and is wound
 *              counter-clockwise seen from outside: (b - a) x (c - a) points from the tetrahedron's inside vertices towards its
 *              outside ones.
 *   Degenerate triangles (two corners at one position) are legal output where a tsdf is exactly 0 beside a negative one (t = 0 or
 *   t = 1).  The tsdf of a valid node should be finite: a NaN counts as outside and gives NaN positions on its edges.  The mesh is
 *   a function of the volume's bytes alone.  Vertex ids are 32-bit: a volume whose mesh has 2^32 or more vertices or triangles
 *   (some 6 10^8 active edges) is beyond this section and is not detected.
 *
 * splat_tsdf_mesh_workspace_bytes(nx, ny, nz): the size of the DEVICE workspace count and emit share (10 bytes per node and
 * some alignment; 0 for dimensions beyond the limits).  splat_tsdf_mesh_count classifies every node and cube into it (per node
 * a 7-bit mask of active edges and its cube's inside pattern; two splat_scan_u32 scans give the vertex and triangle bases) and
 * writes the two counts to HOST pointers: it waits for the stream, the one host synchronisation of this section.
 * splat_tsdf_mesh_emit writes the mesh from the same volume and the workspace count left, repeating none of the classification:
 * vertices (3 floats each), vertex_colors (3 floats each; optional, needs color), triangles (3 uint32 each); exactly the counted
 * numbers, nothing beyond them.  The tsdf plane is read again only at the endpoints of active edges.
 *
 * All work goes to the ctx's stream.  SPLAT_ERR_INVALID, nothing launched and nothing written: a NULL grid, ctx or required
 * pointer (color, obs_weight, image and vertex_colors may be NULL; vertex_colors without color is refused); a plane or buffer that
 * is not 4-byte aligned, a workspace that is not 16-byte aligned or smaller than splat_tsdf_mesh_workspace_bytes; dimensions
 * beyond the limits; voxel or trunc not finite and > 0; a non-finite origin; an unknown depth_kind; an image with a stride below
 * 3; width or height 0 or above 65535; max_weight or min_weight negative or not finite. */
typedef struct splat_tsdf_grid {
    float origin[3]; /* position of node (0, 0, 0) */
    float voxel;     /* node spacing */
    uint32_t dims[3]; /* nx, ny, nz */
    float trunc;     /* truncation distance, in world units */
} splat_tsdf_grid;
int splat_tsdf_integrate(splat_ctx *ctx, const splat_tsdf_grid *grid, void *tsdf, void *weight, void *color, const float *uniforms,
                         uint32_t depth_kind, const void *depth, const void *obs_weight, const void *image, uint32_t image_stride,
                         uint32_t width, uint32_t height, float max_weight);
uint64_t splat_tsdf_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int splat_tsdf_mesh_count(splat_ctx *ctx, const splat_tsdf_grid *grid, const void *tsdf, const void *weight, float min_weight,
                          void *workspace, uint64_t workspace_bytes, uint32_t *n_vertices_host, uint32_t *n_triangles_host);
int splat_tsdf_mesh_emit(splat_ctx *ctx, const splat_tsdf_grid *grid, const void *tsdf, const void *color, const void *workspace,
                         uint64_t workspace_bytes, void *vertices, void *vertex_colors, void *triangles);

/* ---- Density control and optimiser: what fitting a cloud of 3D Gaussians needs beside the frame (an extension) --------------
 * The parameters are 3DGS's raw ones, contiguous float32 DEVICE planes: means (n, 3), log_scales (n, 3), rotations (n, 4) as
 * (w, x, y, z), unnormalised, opacity_logits (n), sh (n, 3 K) basis-major as splat_sh_colors takes it.  The activations
 * (scale = exp, opacity = sigmoid) are the caller's.  Everything here goes to the ctx's stream; only splat_densify_plan waits
 * on the host.  No kernel uses atomics: the same inputs give the same bits.
 *
 * splat_adam_step: one fused Adam update (torch's, without amsgrad or weight decay) of ONE plane of rows x floats_per_row
 * floats, per element
 *   m = beta1 m + (1 - beta1) g,   v = beta2 v + (1 - beta2) g^2,   p -= step m / (sqrt(v) inv_sqrt_bc2 + eps),
 * where the caller computes step = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) for its step count t.  The
 * hyperparameters cross as doubles and are rounded to binary32 once (1 - beta is formed in double first); the arithmetic is
 * binary32.  Columns < head_floats of a row use step_head, the others step_tail (the SH plane's two learning rates, DC and
 * rest, without splitting the tensor); pass head_floats = floats_per_row for one rate.  visible_u8 (`rows` bytes, or NULL): a
 * row whose byte is 0 keeps param, m and v bit for bit and its state is not loaded; the other rows get the bits the unmasked
 * call gives them.  Planes that are all 16-byte aligned are moved with 16-byte loads and stores, others (4-byte aligned) with
 * scalar ones; both give the same bits.  rows = 0: success, nothing launched.  SPLAT_ERR_INVALID: a NULL or misaligned plane,
 * floats_per_row = 0, head_floats > floats_per_row, rows x floats_per_row above 2^32 - 257, a beta outside [0, 1). */
int splat_adam_step(splat_ctx *ctx, void *param, const void *grad, void *m, void *v, uint32_t rows, uint32_t floats_per_row,
                    uint32_t head_floats, double step_head, double step_tail, double beta1, double beta2, double inv_sqrt_bc2,
                    double eps, const void *visible_u8);
/* splat_density_accumulate: one frame's statistics.  records: the forward's n x 8 floats {c.x, c.y, B00, B01, 0, B11, 0, 0}
 * (splat_project_ellipsoid); grad_records: dL/drecords, n x 8 floats of which [0], [1] are read (both 16-byte aligned).  Splat i
 * is VISIBLE when its record is not the culled all-zero record and its 3-sigma box c -/+ (hx, hy) overlaps the screen:
 *   hx = sqrt(B01^2 + B11^2) / (B00 B11),  hy = 1 / B11   (disc_bounds()'s half-widths),
 *   c.x + hx > 0, c.x - hx < W, c.y + hy > 0, c.y - hy < H,
 * evaluated in binary32, one rounding per operation as written.  A visible splat gets
 *   grad_accum[i] += hypot(g.x W / 2, g.y H / 2)   (3DGS's NDC scaling: its 2e-4 threshold carries over),
 *   denom[i] += 1,   max_radius[i] = max(max_radius[i], max(hx, hy));
 * an invisible one keeps all three.  visible_u8[i] is WRITTEN 1 or 0 for every splat: this frame's mask, the one
 * splat_adam_step takes.  grad_accum, denom, max_radius: n floats each, zeroed by the caller before the first frame. */
int splat_density_accumulate(splat_ctx *ctx, const void *records, const void *grad_records, uint32_t n, uint32_t width,
                             uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8);
/* splat_density_accumulate_abs: splat_density_accumulate with the gradient read from grad_center_abs, the n x 2 plane of
 * splat_composite_backward_abs (g.x = [i][0], g.y = [i][1]; 8-byte aligned), instead of columns 0 and 1 of the n x 8 plane: the
 * same visibility rule, the same hypot(g.x W / 2, g.y H / 2), the same updates of denom, max_radius and visible_u8, by the same
 * kernel.  A plane that copies columns 0 and 1 of a grad_records gives splat_density_accumulate's bits.  The absolute statistic
 * is several times the signed one (it does not cancel): gsplat recommends a densification threshold of 8e-4 with it, not 2e-4. */
int splat_density_accumulate_abs(splat_ctx *ctx, const void *records, const void *grad_center_abs, uint32_t n, uint32_t width,
                                 uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8);
/* splat_densify_plan: decide, count and lay out the next cloud.  Per splat, in binary32:
 *   g = denom > 0 ? grad_accum / denom : 0,  s = exp(max log-scale) (NaN if any is),  o = sigmoid(logit),  r = max_radius;
 *   DEAD       when !(o >= min_opacity), or max_screen_radius > 0 && r > max_screen_radius, or max_world_scale > 0 &&
 *              !(s <= max_world_scale): no rows, never densified (a NaN logit or scale is dead, where that rule is on);
 *   WANTS MORE otherwise when g >= grad_threshold (false for a NaN): SPLIT when s > scale_threshold (two new rows, the parent
 *              dropped), else CLONE (the parent and one copy);
 *   the cap    a clone and a split each add one row.  With max_splats > 0 they are granted in index order while
 *              survivors + extras granted so far < max_splats; a refused splat is kept as it is.  So the output never exceeds
 *              max_splats when the survivors alone fit, and is the survivors otherwise.
 * rows (DEVICE, room for 2 n uint32) receives one word per output row, parent index in bits 0-29, kind in bits 30-31: 0 a kept
 * original, 1 a clone's copy, 2 and 3 the children of a split; rows are in parent order, a clone's original before its copy.
 * *n_out_host and counts4_host = {pruned, kept, cloned, split} (splats, not rows: n_out = kept + 2 cloned + 2 split) are HOST
 * words: THIS CALL SYNCHRONISES THE STREAM ONCE to fill them (it runs every hundred steps or so).  workspace: DEVICE, 16-byte
 * aligned, at least splat_densify_plan_workspace_bytes(n).  The scans are splat_scan_u32's kernels.  n = 0: zeros, nothing
 * launched.  SPLAT_ERR_INVALID: n >= 2^30, a NULL or misaligned pointer, a workspace that is too small. */
typedef struct splat_densify_cfg {
    float grad_threshold, scale_threshold, min_opacity;
    float max_screen_radius; /* 0 = off */
    float max_world_scale;   /* 0 = off */
    uint32_t max_splats;     /* 0 = no cap */
    uint64_t seed;           /* read by splat_densify_geometry */
} splat_densify_cfg;
uint64_t splat_densify_plan_workspace_bytes(uint32_t n);
int splat_densify_plan(splat_ctx *ctx, const void *log_scales, const void *opacity_logits, const void *grad_accum, const void *denom,
                       const void *max_radius, uint32_t n, const splat_densify_cfg *cfg, void *workspace, uint64_t workspace_bytes,
                       void *rows, uint32_t *n_out_host, uint32_t *counts4_host);
/* Apply a plan: gathers over OUTPUT rows (contiguous writes); `rows` and n_out are splat_densify_plan's, the input planes the
 * ones it planned for (a row's parent index is not checked against them).  Outputs must not alias inputs.
 * splat_densify_geometry writes means_out and log_scales_out (n_out x 3 floats): kinds 0 and 1 copy their parent's; child
 * k = kind - 2 of a split gets log sigma - log 1.6 (rounded once) and mu + R(q) (sigma (.) xi_k), R the rotation matrix of the
 * normalised quaternion as csrc/ellipsoid.h forms it, sigma = exp(log_scales), xi_k a standard normal 3-vector from
 * Philox4x32-10 with key (seed low word, seed high word) and counter (parent, k, 0, 0): with its four words x_j,
 *   u_j = (x_j + 0.5) 2^-32,  xi = (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1, sqrt(-2 ln u2) cos 2 pi u3).
 * The same seed gives the same cloud.  rotations: 16-byte aligned.
 * splat_densify_rows moves any other plane of floats_per_row floats per splat: SPLAT_DENSIFY_COPY gives every row its parent's
 * (parameters); SPLAT_DENSIFY_ZERO_NEW copies for kind 0 and writes zeros for kinds 1-3 (Adam's moments: as in 3DGS, kept
 * splats keep theirs and new ones start at zero).  n_out x floats_per_row must not exceed 2^32 - 257. */
#define SPLAT_DENSIFY_COPY 0
#define SPLAT_DENSIFY_ZERO_NEW 1
int splat_densify_geometry(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *means, const void *log_scales,
                           const void *rotations, const splat_densify_cfg *cfg, void *means_out, void *log_scales_out);
int splat_densify_rows(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *in, void *out, uint32_t floats_per_row,
                       uint32_t mode);
/* Density control for 2D Gaussian surfels ("2D Gaussian surfels", above): the three entry points above that read what an
 * ellipsoid and a surfel do not share.  A surfel's log_scales plane is n x 2 floats (sx, sy), 4-byte aligned; everything not
 * said here - the other arguments, the checks, the stream, no atomics, n = 0 - is the peer's, and splat_adam_step and
 * splat_densify_rows move a surfel's planes as they are (floats_per_row = 2 for the log-scales and their moments).
 * splat_density_accumulate_surfel: splat_density_accumulate over splat_project_surfel's records, whose B10 and q are not zero.
 * With (x0, y0, x1, y1) the record's exact screen extent (csrc/disc.h, disc_bounds(): binary32, one rounding per operator; the
 * box splat_project_surfel wrote to `projected`), surfel i is VISIBLE when the extent exists (a culled all-zero record has none,
 * nor has one whose disc reaches the eye's plane) and x1 > 0, x0 < W, y1 > 0, y0 < H.  Its radius is
 * 0.5 max(x1 - x0, y1 - y0): the bits of projected[i].screenRadius.  grad_accum, denom, max_radius and visible_u8 as above.
 * SPLAT_ERR_INVALID also for n >= 2^30.
 * splat_densify_plan_surfel: splat_densify_plan with s = exp(max(l0, l1)) (NaN if either is) of the n x 2 plane: the same
 * workspace function, rows, cap rule and single host synchronisation.
 * splat_densify_geometry_surfel: log_scales and log_scales_out are n x 2 and n_out x 2.  Kinds 0 and 1 copy; child k of a split
 * gets log sigma - log 1.6 on both scales (rounded once) and mu + R[:,0] sx xi_x + R[:,1] sy xi_y, R as csrc/surfel.h forms it,
 * (xi_x, xi_y) the first two normals of splat_densify_geometry's Philox draw for (parent, k); the third is not used.  This is
 * 2DGS's split, stds = (sx, sy, 0): the children stay in the parent's plane. */
int splat_density_accumulate_surfel(splat_ctx *ctx, const void *records, const void *grad_records, uint32_t n, uint32_t width,
                                    uint32_t height, void *grad_accum, void *denom, void *max_radius, void *visible_u8);
int splat_densify_plan_surfel(splat_ctx *ctx, const void *log_scales, const void *opacity_logits, const void *grad_accum,
                              const void *denom, const void *max_radius, uint32_t n, const splat_densify_cfg *cfg, void *workspace,
                              uint64_t workspace_bytes, void *rows, uint32_t *n_out_host, uint32_t *counts4_host);
int splat_densify_geometry_surfel(splat_ctx *ctx, const void *rows, uint32_t n_out, const void *means, const void *log_scales,
                                  const void *rotations, const splat_densify_cfg *cfg, void *means_out, void *log_scales_out);

/* ---- MCMC relocation: 3DGS-MCMC's way of deciding where the splats live (Kheradmand et al., "3D Gaussian Splatting as Markov
 * Chain Monte Carlo", 2024; an extension) -----------------------------------------------------------------------------------------
 * The other strategy beside splat_densify_*: dead splats are moved onto live ones drawn in proportion to opacity, with opacity
 * and scale corrected so that the rendered image does not change; the cloud grows to an exact budget the same way; and the
 * means get opacity-gated noise at every step.  No gradient statistics, no screen-space thresholds, no opacity reset.  The
 * planes are the density block's (contiguous float32 DEVICE planes, 4-byte aligned unless said otherwise), everything goes to the
 * ctx's stream, and only splat_mcmc_sample waits on the host.  splat_mcmc_sample counts the draws per source with unsigned
 * integer atomic adds, whose result does not depend on their order; no kernel uses a floating-point atomic: the same inputs and
 * seed give the same bits.
 *
 * splat_mcmc_sample: who is dead, who is drawn, how often.  Per splat, in binary64:
 *   o = 1 / (1 + exp(-(double)logit)),   q = (uint32) floor(o 2^24)  (0 for a NaN logit),   q_min = ceil(min_opacity 2^24);
 *   DEAD when q < q_min, ALIVE otherwise; its weight is q when alive and 0 when dead.
 * The weights are summed exactly in uint64: C_i their inclusive prefix sum, T the total.  mode SPLAT_MCMC_RELOCATE: there is one
 * draw per dead splat, draw j belongs to the j-th dead splat in index order and targets[j] is its index (n_draws is ignored).
 * mode SPLAT_MCMC_ADD: n_draws draws, targets[j] = n + j.  Draw j: Philox4x32-10 with key (seed low word, seed high word) and
 * counter (j, 0, mode, 0) (a split's is (parent, k, 0, 0) and the noise's (i, step, 3, 0): none is shared), r = x0 | x1 << 32,
 * t = floor(r T / 2^64), sources[j] = the smallest i with C_i > t; counts[i] = the draws whose source is i.
 * targets, sources (DEVICE): room for n uint32 when relocating, n_draws when adding; counts (DEVICE): n uint32, all written.
 * counts3_host = {dead, alive, draws made} are HOST words: THIS CALL SYNCHRONISES THE STREAM ONCE to fill them.  With T = 0
 * (nobody alive) no draw is made: counts are zeros, draws made = 0, targets and sources are not written.  workspace: DEVICE,
 * 16-byte aligned, at least splat_mcmc_sample_workspace_bytes(n).  n = 0: zeros, nothing launched.  SPLAT_ERR_INVALID: n >= 2^30
 * (or n + n_draws above 2^30), an unknown mode, min_opacity outside [0, 1], a NULL or misaligned pointer, a workspace that is
 * too small. */
#define SPLAT_MCMC_RELOCATE 1
#define SPLAT_MCMC_ADD 2
uint64_t splat_mcmc_sample_workspace_bytes(uint32_t n);
int splat_mcmc_sample(splat_ctx *ctx, const void *opacity_logits, uint32_t n, uint32_t mode, uint32_t n_draws, double min_opacity,
                      uint64_t seed, void *workspace, uint64_t workspace_bytes, void *targets, void *sources, void *counts,
                      uint32_t *counts3_host);
/* splat_mcmc_apply: move the draws and correct the sources, in place.  targets, sources, counts, n and n_draws (the draws made)
 * are splat_mcmc_sample's; the planes hold `rows` rows: n when relocating, n + n_draws when adding (the first n filled by the
 * caller).  For a source i with c = counts[i] > 0, N = min(c + 1, 51), in binary64 from the source's OLD values:
 *   o' = 1 - (1 - o)^(1/N),
 *   D  = sum_{a=1..N} sum_{k=0..a-1} binom(a-1, k) (-1)^k o'^(k+1) / sqrt(k+1)      (o' unclamped; a 51 x 51 table of doubles),
 *   new logit      = logit(clamp(o', min_opacity, 1 - 2^-23)), rounded to binary32 once,
 *   new log_scales = (double)log_scale + log(o / D) per axis, rounded once.
 * (A) per draw j, row targets[j] of the five parameter planes gets row sources[j]: means, rotations and sh bit for bit, logit
 * and log_scales the new values; then (B) every source with c > 0 gets the same new values (the same bits).  Sources are alive
 * and a relocation's targets dead, so this is race-free in place.  Moments: both Adam moments of all five planes are ZEROED for
 * every target row AND every source with c > 0 (the paper's code zeroes only the sources; a moved row's old momentum belongs to
 * a splat that no longer exists).  m[k] / v[k] may be NULL (no such plane).  Rows that are neither target nor source are not
 * written.  A draw whose target is not below `rows` or whose source is not below n is skipped.  n_draws = 0: nothing launched.
 * SPLAT_ERR_INVALID: a NULL or misaligned pointer, rows < n, sh_floats outside 1-48, n_draws x (11 + sh_floats) above 2^32 - 257. */
typedef struct splat_mcmc_planes {
    void *param[5], *m[5], *v[5]; /* means, log_scales, rotations, opacity_logits, sh: 3, 3, 4, 1 and sh_floats floats per row */
    uint32_t sh_floats;
} splat_mcmc_planes;
int splat_mcmc_apply(splat_ctx *ctx, const void *targets, const void *sources, const void *counts, uint32_t n, uint32_t n_draws,
                     uint32_t rows, double min_opacity, const splat_mcmc_planes *planes);
/* splat_mcmc_noise: the per-step exploration term, one pass over the cloud (44 bytes read, 12 written per splat).  Per splat, in
 * binary32, R the rotation matrix of the normalised quaternion as csrc/ellipsoid.h forms it:
 *   o = sigmoid(logit),   g = 1 / (1 + exp(-100 (0.005 - o)))   (the paper's op_sigmoid(1 - o, k = 100, x0 = 0.995)),
 *   Sigma = R diag(exp(2 log_scales)) R^T,   xi = splat_densify_geometry's three normals from counter (i, step, 3, 0),
 *   means[i] += Sigma xi g scale.
 * scale (the caller's noise_lr x lr_means) crosses as a double and is rounded to binary32 once.  Planes that are all 16-byte
 * aligned are moved with 16-byte loads and stores, others with scalar ones; both give the same bits.  n = 0: nothing launched.
 * SPLAT_ERR_INVALID: n >= 2^30, a NULL or misaligned plane. */
int splat_mcmc_noise(splat_ctx *ctx, void *means, const void *log_scales, const void *rotations, const void *opacity_logits, uint32_t n,
                     double scale, uint32_t step, uint64_t seed);

/* ---- Initialisation from a point cloud: the scale 3DGS gives a new splat (simple_knn's distCUDA2; an extension) ----------------
 * What every fit starts from is a sparse point cloud; 3DGS sets the scale of the splat at each point to the root of the mean
 * squared distance to the point's three nearest neighbours.  splat_knn_mean_sq computes that mean, exactly as stated here, for
 * every point, without the n x n distances: the points are sorted along a 63-bit Morton curve with the caller's sorter, cut into
 * blocks of 64 with a bounding box each, and a block is left out of a query's search only when its box proves that none of its
 * members can change the result.  Everything goes to the ctx's stream and nothing waits on the host.
 *
 * THE CONTRACT, in binary32, every operator one correctly rounded operation, no contraction:
 *   d(i, j)    = ((dx dx + dy dy) + dz dz),   dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j;
 *   the candidates of i are the j != i whose d(i, j) is finite (a duplicate of point i is a candidate, at distance 0);
 *   b0 <= b1 <= b2 are the three smallest candidate values, padded with +inf when there are fewer than three;
 *   mean_sq[i] = ((b0 + b1) + b2) / 3.0f.
 * So: n < 4 gives +inf in every row; a point with a NaN or an infinite coordinate gets +inf and is nobody's neighbour (every
 * distance to it is NaN or infinite), and so does a point so far out that its squares overflow; ties need no rule, because only
 * the values enter; and the result is a function of the input alone, bit for bit, on every run and whatever the search skipped.
 * Why skipping is exact: for a box [lo, hi] and a query x, g = max(lo - x, x - hi, 0) per axis and lb = ((gx gx + gy gy) + gz gz),
 * in d's operation order.  Rounding is monotone: for a member q <= hi < x, fl(x - q) >= fl(x - hi), squares and sums of
 * non-negative terms in the same order keep the inequality, so lb <= d(i, j) for every member j.  A block is skipped only when
 * lb > b2 (equality is visited, and so is a NaN bound, which compares false); nothing depends on the Morton codes but the order
 * of the visits.
 *
 * points: DEVICE float32, 4-byte aligned; point i is the three floats at points + i * stride_floats, stride_floats >= 3 (3: a
 * fit's means; 4: a pos_radius plane, whose fourth word is not read).  mean_sq: DEVICE, n floats, all written.  sorter: capacity
 * >= n; its buffers are overwritten.  workspace: DEVICE, 16-byte aligned, at least splat_knn_workspace_bytes(n).
 * evaluations: NULL, or a DEVICE uint64 (8-byte aligned) that the call zeroes on the stream and that receives the number of
 * d(i, j) evaluations any lane performed, those done only because a wave runs its 64 queries in lockstep included (unsigned
 * integer atomic adds, one per wave: the sum does not depend on their order).  Brute force performs n (n - 1).
 * n = 0: success, nothing launched (evaluations is not written either).  SPLAT_ERR_INVALID: a NULL or misaligned pointer,
 * stride_floats < 3, n >= 2^30, a workspace that is too small or not 16-byte aligned.  SPLAT_ERR_CAPACITY: a sorter smaller than n. */
uint64_t splat_knn_workspace_bytes(uint32_t n);
int splat_knn_mean_sq(splat_ctx *ctx, splat_sorter *sorter, const void *points, uint32_t stride_floats, uint32_t n,
                      void *workspace, uint64_t workspace_bytes, void *mean_sq, void *evaluations);

/* ---- multi-GPU band path (no reference equivalent — the reference is single-device) */
/* The oriented-disc projector (src/SequentialRenderer.ts:68-71,91-112): the splat is the disc
 * p + r*(t*u + b*v), u^2+v^2 <= 1, in the tangent plane of its normal (t = normalize(cross(up, n)), b =
 * cross(n, t)).  Per splat it writes
 *   discs[i]     = 8 floats {c.x, c.y, B00, B01, B10, B11, q0, q1}: the inverse of the disc's plane-to-screen
 *                  homography about its screen centre c — (u,v) = B*d / (1 - q.d), d = pixel centre - c —
 *                  which is what the rasteriser's perspective-correct interpolation evaluates; all zeros when
 *                  the quad has a corner at w <= 0 or is seen edge-on;
 *   projected[i] = a ProjectedSplat whose bounds are the disc's exact screen extent (a pure function of the
 *                  disc record), depth as splat_project, screenRadius = half the larger extent;
 * and keys / payload exactly as splat_project.  Sort and bin as usual with `projected`; composite with
 * cfg.footprint = SPLAT_FOOTPRINT_DISC and `discs` as the records.  Bit-exact against the oracle. */
int splat_project_disc(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4,
                       const void *normals, uint32_t normal_stride_vec4, uint32_t n, void *projected, void *discs,
                       void *keys, void *payload, uint32_t n_padded);
/* Projects splats [first, first+count) of the scene into projected_slice[0..count) with
 * originalIndex = global index: the per-rank share of the projector before the all-gather. */
int splat_project_slice(splat_ctx *ctx, const float *uniforms, const void *pos_radius,
                        uint32_t pr_stride_vec4, uint32_t first, uint32_t count,
                        void *projected_slice);
/* The multi-GPU exchange format: 16 bytes per splat, float4 {screen centre x, y, screen radius, depth}.
 * The 32-byte ProjectedSplat is a pure function of it — bounds = centre -/+ radius * 1.5 in the
 * projector's own operation order (src/SplatProjector.ts:119-121), originalIndex = position in the
 * gathered array — so ranks all-gather half the bytes and splat_band_frame / splat_composite rebuild
 * what they need bit-exactly (cfg->record_format = SPLAT_RECORDS_COMPACT).  splat_expand_compact
 * materialises ProjectedSplat records (originalIndex = index_base + i) for callers that want them. */
int splat_project_slice_compact(splat_ctx *ctx, const float *uniforms, const void *pos_radius,
                                uint32_t pr_stride_vec4, uint32_t first, uint32_t count,
                                void *records16_slice);
/* The oriented-disc footprint's exchange records: 48 bytes per splat, 3 x float4 {disc record (8 floats, see
 * splat_project_disc), depth, 0, 0, 0}.  The disc's bounds are a pure function of the record and the index is the
 * position in the gathered array, so splat_band_frame (cfg->footprint = SPLAT_FOOTPRINT_DISC, cfg->record_format =
 * SPLAT_RECORDS_DISC48) needs nothing else.  DISC48 band frames take the tile-first order wherever it exists (screens of
 * at most 256 x 256 tiles: with the sort-first order set there they return SPLAT_ERR_INVALID) and bin sort-first only
 * beyond 256 x 256 tiles, where no tile-first order exists. */
int splat_project_slice_disc(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4,
                             const void *normals, uint32_t normal_stride_vec4, uint32_t first, uint32_t count,
                             void *records48_slice);
int splat_expand_compact(splat_ctx *ctx, const void *records16, uint32_t n, uint32_t index_base,
                         void *projected);
/* Stable compaction of the splats whose clamped tile-row range meets [tile_row0, tile_row1):
 * writes (depth key, global index) pairs in ascending index order into the sorter's input
 * buffers and the number kept to *n_kept_host (synchronises). */
int splat_band_keys(splat_ctx *ctx, splat_sorter *sorter, const void *projected, uint32_t n,
                    uint32_t width, uint32_t height, uint32_t tile_size, uint32_t tile_row0,
                    uint32_t tile_row1, uint32_t *n_kept_host);

/* One rank's frame after the exchange, without a host round trip: tile rows [cfg->tile_row0,
 * cfg->tile_row1) binned, depth-sorted and composited from the gathered records.  Tile-first order
 * (default): one pass over the records gives depth keys and tile ranges clamped to the band — a splat
 * outside it has an empty range — then the frame's binner and per-tile sort; sort-first order: band
 * filter (kept count on the device) -> depth sort -> bin, the only order beyond 256 x 256 tiles (there the
 * filter leaves each kept splat's 8-byte tile range for the binner).  records: n_records records in
 * cfg->record_format whose position is the global splat index (the all-gathered shards);
 * props/normals: the full scene in the reference's layouts (props = interleaved records); with
 * cfg->prelit, props is the plane of lit colours (splat_lit_colors) and normals may be NULL.
 * (cfg->record_format = SPLAT_RECORDS_LIT32 is not a band frame's format: round 4's variant that built lit composite records
 * for the splats a band keeps measured 20 us per rank slower on eight ranks and was removed.) */
int splat_band_frame(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner,
                     const splat_composite_cfg *cfg, const void *props, const void *normals,
                     const void *records, uint32_t n_records, uint32_t width, uint32_t height,
                     void *out_rgba8, void *out_rgba32f, void *consumed_dptr);
/* After the first frame splat_band_frame sizes its grids from the PREVIOUS frame's pair total (and, in
 * the sort-first order, kept count), x1.125, and learns its own asynchronously; a frame that outgrew
 * those bounds is reported by the next splat_band_frame / splat_band_settle call with
 * SPLAT_ERR_CAPACITY (render it again; the bounds have been raised).  splat_band_settle waits for the
 * last frame's readback, so on SPLAT_OK that frame's image is final; it returns the number of splats
 * with a tile in the band and the pair total. */
int splat_band_settle(splat_ctx *ctx, splat_sorter *sorter, splat_binner *binner, uint32_t *n_kept_host,
                      uint64_t *pairs_host);
/* Number of splats the last splat_band_frame / splat_band_keys kept (synchronises). */
int splat_band_kept(splat_ctx *ctx, splat_sorter *sorter, uint32_t *n_kept_host);

/* ---- SDF splat generation: the producer of the positions and normals this path consumes ----------
 * src/sdf/CodeGenerator.ts:97-225,276-353 (primitive / operation library, sceneSDF), src/GradientSampler.ts,
 * src/shaders/update-positions.wgsl:22-50, src/CurvatureSampler.ts:84-141.  The reference generates one WGSL function
 * per scene graph; here the graph is DATA: a postfix program (children first, then their operation — the order
 * CodeGenerator's traverse() emits) of at most SPLAT_SDF_MAX_INSTR instructions, handed over with every call (host
 * memory; it travels in the kernel arguments).  A value is vec4(distance, gradient).  Bit-exact against oracle/oracle.c. */
#define SPLAT_SDF_SPHERE 0u        /* a = {center.xyz, radius}                    sdgSphere  :100-106 */
#define SPLAT_SDF_BOX 1u           /* a = {center.xyz, half size.xyz}             sdgBox     :109-133 */
#define SPLAT_SDF_TORUS 2u         /* a = {center.xyz, major radius, minor radius} sdgTorus   :136-157 */
#define SPLAT_SDF_CAPSULE 3u       /* a = {center.xyz, height, radius}            sdgCapsule :160-176 */
#define SPLAT_SDF_UNION 16u        /* pops b, a; pushes the nearer               opUnion        :181-187 */
#define SPLAT_SDF_INTERSECTION 17u /*                                             opIntersection :190-196 */
#define SPLAT_SDF_SUBTRACTION 18u  /*                                             opSubtraction  :199-202 */
#define SPLAT_SDF_SMOOTH_UNION 19u /* a = {k}                                     opSmoothUnion  :206-224 */
#define SPLAT_SDF_MAX_INSTR 32u
typedef struct splat_sdf_instr {
    uint32_t op;
    float a[7];
} splat_sdf_instr;
/* GradientSampler.evaluateGradients: gradients[i] = sceneSDF(positions[i].xyz) (vec4 in, vec4 out). */
int splat_sdf_gradients(splat_ctx *ctx, const splat_sdf_instr *program, uint32_t n_instr, const void *positions, uint32_t n,
                        void *gradients);
/* PositionUpdater.updatePositions: next = vec4(pos - normalize(gradient) * distance, 0) (pos where the gradient vanishes). */
int splat_sdf_update_positions(splat_ctx *ctx, const void *positions, const void *gradients, uint32_t n, void *next_positions);
/* CurvatureSampler.computeScaleFactors: one f32 per point from the normals at six offsets of 0.02. */
int splat_sdf_scale_factors(splat_ctx *ctx, const splat_sdf_instr *program, uint32_t n_instr, const void *positions, uint32_t n,
                            void *scale_factors);
/* vec4(normalize(gradient), scale factor): the "curvatureData" layout splat_update_props reads
 * (src/SplatPropertyManager.ts:70-72; the reference's samplers write the two halves to separate buffers). */
int splat_sdf_curvature(splat_ctx *ctx, const void *gradients, const void *scale_factors, uint32_t n, void *curvature);
/* PointManager.generateRandomPositions (src/PointManager.ts:96-189) on the device: n points on the faces of the box
 * [aabb_min, aabb_max] (the caller's scaled global AABB of the scene: host floats), a face chosen with probability
 * proportional to its area, uniform on the face, w = 0.  The reference draws them from an unseeded Math.random on the
 * CPU and uploads them every frame (:220-231); here point i of a cloud is a pure function of (seed, i) — a 64-bit
 * counter hash (splitmix64 of seed * 0x9E3779B97F4A7C15 + 2 i and + 2 i + 1), 24 bits per uniform — so a frame's fresh
 * cloud costs one small kernel and no transfer, and the oracle restates it bit for bit (orc_sdf_seed_positions). */
int splat_sdf_seed_positions(splat_ctx *ctx, const float *aabb_min3, const float *aabb_max3, uint32_t n, uint64_t seed,
                             void *positions);
/* The producer half of the reference's frame (src/main.ts:146-180) in one launch: per point its fresh position
 * (aabb_min3 / aabb_max3 != NULL: drawn as splat_sdf_seed_positions draws point i of cloud `seed`; NULL: read from
 * positions_in), `steps` >= 1 rounds of {splat_sdf_gradients, splat_sdf_update_positions} (main.ts runs five), then
 * splat_sdf_scale_factors at the final position, splat_sdf_curvature with the gradient of the LAST evaluation (one step
 * behind the position, as main.ts:186 hands it on) and splat_update_props.  Outputs: final positions, that gradient
 * (optional), vec4(normal, scale), the 32-byte property records (optional) — bit for bit what the stage-by-stage calls
 * give (tests/test_gpu_sdf.py), without their thirteen launches. */
int splat_sdf_generate(splat_ctx *ctx, const splat_sdf_instr *program, uint32_t n_instr, const float *aabb_min3, const float *aabb_max3,
                       uint64_t seed, const void *positions_in, uint32_t n, uint32_t steps, void *positions_out, void *gradients_out,
                       void *curvature_out, void *props_out);

/* ---- Renderer.render: the image the reference app draws  (src/Renderer.ts:68-143,196-201,250-311; src/main.ts:183-190) ---
 * One opaque quad per point in the tangent plane of its SDF gradient (normal = normalize(gradient.yzw), the tangent frame
 * of computeTangent, half-side 0.025 * scale), two triangles, drawn in index order through a depth test ("less" against a
 * depth buffer cleared to 1), shaded from the normal, on the clear colour (0.05, 0.05, 0.1, 1).  Conventions:
 * pixel centres at +0.5, top-left fill rule, stored depth z/w (a fragment passes when 0 <= z/w < the stored value; on
 * equal depth the lower index wins), no clipper: a quad with a corner at w <= 0 is dropped, and a point whose normal,
 * scale or corners are not finite covers nothing.
 *   uniforms: the 22-float block of splat_project (VP = floats 0-15 are read);
 *   positions: vec4 (xyz used), pos_stride_vec4 float4s apart; gradients: vec4(distance, gradient), grad_stride_vec4
 *   apart; scales: the first point's f32 scale, the next scale_stride_f32 floats on (1: CurvatureSampler's scale-factor
 *   buffer; 4 with scales = curvature + 3 floats: the .w of the vec4(normal, scale) buffer splat_sdf_generate writes);
 *   outputs, each W*H and each optional (NULL = not written): out_rgba8 (rgba8unorm), out_rgba32f (vec4 f32), out_depth_f32
 *   (z/w of the visible fragment, 1.0 where none), out_ids (u32 index of the visible point, 0xFFFFFFFF where none).
 * The binner must have tile size 16 and serve this frame only: it bins every frame in index order, and the per-point
 * records the frame builds live in it.  Everything runs on the ctx stream; one host round trip per frame (the binner's
 * pair total is read back: no frame ever needs to be rendered again). */
int splat_point_frame(splat_ctx *ctx, splat_binner *binner, const float *uniforms, const void *positions, uint32_t pos_stride_vec4,
                      const void *gradients, uint32_t grad_stride_vec4, const void *scales, uint32_t scale_stride_f32, uint32_t n,
                      uint32_t width, uint32_t height, void *out_rgba8, void *out_rgba32f, void *out_depth_f32, void *out_ids);

/* ---- the multi-GPU frame's one exchange (no reference equivalent): RCCL over xGMI ------------------
 * One process per GPU.  Rank 0 makes a unique id (splat_comm_unique_id) and hands its SPLAT_COMM_ID_BYTES to the
 * other ranks by any channel the host has (a file, a socket, MPI, torch.distributed.broadcast); every rank then
 * calls splat_comm_init (collective: returns when all `world` ranks have joined).  A frame is then
 *     splat_project_slice_compact(my slice) -> splat_allgather_records(shard, gathered) -> splat_band_frame(gathered)
 * all enqueued on the ctx stream: no host synchronisation in between.  librccl is bound at run time, on first use:
 * when it cannot be loaded these return SPLAT_ERR_COMM (nothing falls back). */
#define SPLAT_COMM_ID_BYTES 128
int splat_comm_unique_id(void *id_out /* SPLAT_COMM_ID_BYTES host bytes */);
int splat_comm_init(splat_ctx *ctx, int rank, int world, const void *unique_id, splat_comm **out);
void splat_comm_destroy(splat_comm *comm);
int splat_comm_rank(const splat_comm *comm, int *rank, int *world);
/* What the communicator ITSELF reports (ncclCommCount / ncclCommUserRank), as opposed to what splat_comm_init was told:
 * a frame loop that records these can show that the ranks it timed really formed one communicator. */
int splat_comm_count(const splat_comm *comm, int *rccl_ranks, int *rccl_rank);
/* All-gather of equal shards: rank r's bytes_per_rank bytes at `shard` land at gathered + r * bytes_per_rank on every
 * rank (in place when shard == gathered + rank * bytes_per_rank).  Asynchronous on the ctx stream (any ctx of the
 * communicator's device); timed as SPLAT_STAGE_EXCHANGE. */
int splat_allgather_records(splat_ctx *ctx, splat_comm *comm, const void *shard, void *gathered, size_t bytes_per_rank);

#ifdef __cplusplus
}
#endif
#endif
