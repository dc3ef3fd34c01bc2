// composite_px.hip — k_composite_px, the composite of 16x16 tiles with a lane per 2x2 pixels, and the host code that is its
// own: which screens it draws (composite_uses_px), the per-band history of tile costs and orders its launches leave for
// one another (px_order_prepare), and its launch (composite_px_launch, called by composite.hip's composite_launch).
//
// Compiled with -ffp-contract=on, as composite.hip; the PX_WAVES and PX_PROFILE knobs of tools/build_variant.sh act here.
#include "composite.h"

#include <cstdlib>

// =====================================================================================================================
// k_composite_px — the lane-efficient composite (round 3; the default for the isotropic footprint, nearest on top).
//
// What k_composite spends its time on is lanes that get g = 0: one entry is evaluated by a whole 8x8-pixel wave although
// its box covers a quarter of it (18.5 live covered pixels per consumed entry at C2, 1.14 wave visits of 64 lanes).
// Here every lane walks ITS OWN entries, and the Gaussian is not evaluated per pixel at all:
//   * one WAVE per 16x16 tile (four tiles per workgroup, no workgroup barrier anywhere), lane = a 2x2-pixel block;
//   * the list is consumed in chunks of 32 entries.  Per chunk the wave stages, in its own 5 KB of LDS,
//       - the entry's Gaussian as two tables: gx[16] over the tile's pixel columns and gy[16] over its rows —
//         exp(-(dx^2+dy^2) k^2) = exp(-(dx k)^2) exp(-(dy k)^2), so 32 exponentials per entry serve all 256 pixels —
//         with the reference's box test (ComputeShaderRenderer.ts:118-121, exact: span_mask16) folded in as zeros,
//       - its lit colour;
//   * per lane a 32-bit queue: bit j = entry j's box touches this lane's 2x2 block (eight ballots transpose the
//     entries' column / row masks into per-column / per-row entry masks; a lane ANDs its column's with its row's);
//   * a trip = every lane with a non-empty queue takes its next entry: two 8-byte table reads (its two columns, its two
//     rows), one 16-byte colour read, then four pixels in packed arithmetic: g = gx*gy, w = T*g, C += c*w, T -= w.
//     Order per pixel is the list's order; pixels of different lanes work on different entries in the same instruction.
//   * the stop rule is per pixel (exactly :187-190): a pixel whose T reaches T_STOP takes its background term at once
//     and continues with T = 0 (it adds exact zeros from then on); a lane whose four pixels have stopped empties its
//     queue; the wave leaves when no pixel is left.
// Trips per consumed entry at C2: 0.30 (a wave instruction of up to 256 pixel-entries each) against 1.14 visits of a
// 64-pixel wave.  Reference semantics: /root/reference/src/ComputeShaderRenderer.ts:150-198.
// =====================================================================================================================
// One list entry as fetched, untouched (k_composite_px keeps a chunk of these in flight: nothing may be computed from
// them at issue).  LIT32: a = {centre.xy, radius, depth}, c = lit colour.  Otherwise a = bounds (or the compact record),
// c = colour, n = normal, r = radius.
struct PxRaw {
    float4 a, c, n;
    float r;
    float4 a2; // DISC: the disc record's second half
    float2 zi; // AOV: {depth, splat index (as bits)}
};
// DISC (the oriented-disc footprint): a, a2 = the 32-byte disc record (disc.h), c = colour, n = normal
// ELL: the ellipsoid's opacity in c.w (its lit records carry the depth there: the opacity comes from the colour plane)
template <bool ELL = false>
__device__ __forceinline__ void px_fetch_disc(const CompositeParams &p, uint32_t idx, PxRaw &o) {
    o.a = p.projected[(size_t)idx * p.disc_stride];
    o.a2 = p.projected[(size_t)idx * p.disc_stride + 1];
    if (p.disc_lit) { // (lit disc records: one 48-byte gather is all)
        o.c = p.projected[(size_t)idx * p.disc_stride + 2];
        if (ELL) o.c.w = p.color[(size_t)idx * p.color_stride].w;
        return;
    }
    o.c = p.color[(size_t)idx * p.color_stride];
    if (!p.prelit) o.n = p.normals[(size_t)idx * p.normal_stride];
}
template <bool LIT32>
__device__ __forceinline__ void px_fetch(const CompositeParams &p, uint32_t idx, PxRaw &o) {
    if constexpr (LIT32) {
        o.a = p.projected[(size_t)idx * 2];
        o.c = p.projected[(size_t)idx * 2 + 1];
    } else {
        if (p.compact) {
            o.a = p.projected[idx];
        } else {
            o.a = p.projected[(size_t)idx * 2];
            o.r = reinterpret_cast<const float *>(p.projected)[(size_t)idx * 8 + 5];
        }
        o.c = p.color[(size_t)idx * p.color_stride];
        if (!p.prelit) o.n = p.normals[(size_t)idx * p.normal_stride];
    }
}
// bounds, screen radius and lit colour of a fetched entry (fetch_entry's arithmetic, at the time of use)
template <bool LIT32>
__device__ __forceinline__ void px_unpack(const CompositeParams &p, const PxRaw &o, float4 &bounds, float &radius, float4 &lit) {
    if constexpr (LIT32) {
        bounds = lit_bounds(o.a);
        radius = o.a.z;
        lit = o.c;
    } else {
        if (p.compact) {
            bounds = lit_bounds(o.a); // the bounds must be the projector's: one rounding per operation
            radius = o.a.z;
        } else {
            bounds = o.a;
            radius = o.r;
        }
        lit = p.prelit ? o.c : lit_color(o.c, o.n);
    }
}

typedef uint32_t v2u __attribute__((ext_vector_type(2)));
constexpr int PXC = 32;     // entries per chunk = bits of a lane's queue
constexpr int PX_ROW = 35;  // float2 slots per table row: the idle slot, 32 entries, 2 of padding — rows 3 slots apart (mod 32),
                            // so the eight rows a wave reads for ONE entry fall into eight different bank pairs of a ds_read_b64
constexpr int PX_TROWS = 16;
// One chunk as the builder wave leaves it for the consumer wave.  Slot 0 of every row is the IDLE entry (zeros): what a
// lane with an empty queue "takes" — entry j lives at slot 1 + j, so ffbl's -1 for an empty queue addresses the idle
// slot without a select.
struct PxBuf {
    float2 t[PX_TROWS][PX_ROW]; // t[c][1 + j] = {gx_j(2c), gx_j(2c+1)}: entry j's factor at the tile's pixel columns 2c, 2c+1 (c < 8);
                                // t[8 + r][1 + j] = {gy_j(2r), gy_j(2r+1)} at its pixel rows; only the pairs entry j's box touches are
                                // written (no lane is ever sent to another)
    float4 col[PX_ROW];         // col[1 + j] = {lit r, g, b, 1}: ONE 16-byte read per trip (ds_read_b128, four LDS-array cycles) — as two
                                // 8-byte rows the compiler merged the pair into a ds_read2_b64: eight cycles on 32 banks
    uint4 q4[4];                // as uint2 q[8]: q[c].x: bit j = entry j's box meets pixel columns 2c, 2c+1; q[r].y: ... pixel rows 2r, 2r+1
};
static_assert(offsetof(PxBuf, col) % 16 == 0, "the colour entries are read 16 bytes at a time");
static_assert(sizeof(PxBuf) * 3 * 10 + 64 <= 160 * 1024, "ten tiles (twenty waves) per CU with three buffers");
// The same for the oriented-disc footprint (SequentialRenderer.ts:91-142; disc.h), which is not separable: no tables — per
// entry the inverse homography's eleven numbers, evaluated by the consumer for the four pixels of every lane the entry's
// box touches (k_composite evaluates it for all 64 pixels of every quadrant the box touches).
struct PxBufDisc {
    float4 par[PXC + 1][3]; // par[1 + j] = {c.x, c.y, -q0, -q1}, {B00, B10, B01, B11}, {lit r, g, b, 1}; par[0]: zeros (the idle entry)
    uint4 q4[4];            // the queue words, as PxBuf's
};
template <bool DISC> struct PxBufOf { typedef PxBuf type; };
template <> struct PxBufOf<true> { typedef PxBufDisc type; };

// Which tile each workgroup of k_composite_px takes: the tiles that took longest first.
// The kernel's duration is its longest tile's plus the time that tile spent sharing its SIMD before it was left alone:
// with every tile resident from the start (C2: 4969 workgroups with entries on 3840 slots) a silhouette tile that walks
// a thousand entries of pixels that never saturate finishes 60 us after tiles that need 150 — unless it is dispatched
// first: the hardware favours the oldest waves, and by the time the bulk has drained the long tiles are done as well
// (C2: 71 -> 57 us with the exact descending order, profiles/r03_c_px_tile_order_oracle_C2.txt).  Which tiles are long is
// not known before they are walked, but a frame resembles the ones before it: every launch leaves each tile's cost
// (chunks walked) behind, and ONE extra workgroup of the next launch — beside the tiles, costing the frame no launch —
// sorts them into nine classes, longest first, empty tiles last, for the launch after.  The order only says who goes
// first: any order (a stale one, one from another scene) gives the same image.
constexpr uint32_t PX_CLASSES = 9;
constexpr uint32_t PX_ORDER_SCRATCH = (PX_CLASSES * 128 + 2 * PX_CLASSES) * 4; // px_make_order's LDS, carved out of the table buffers
__device__ __forceinline__ uint32_t px_cost_class(uint32_t c) { // 0 = longest ... 8 = no entries
    return 8u - ((c >= 1) + (c >= 3) + (c >= 5) + (c >= 7) + (c >= 9) + (c >= 12) + (c >= 16) + (c >= 24));
}
__device__ __forceinline__ void px_make_order(const uint32_t *__restrict__ cost, uint32_t tiles, uint32_t *__restrict__ order, uint32_t *s_scratch) {
    // 128 threads; thread i owns the tiles [i * per, (i + 1) * per) — consecutive, so the order inside a class is the
    // row-major one — and reads their costs sixteen at a time (the arrays are padded to whole 16-byte reads:
    // px_order_prepare).  Its nine counters live in LDS (s_cnt[class][thread]: the class of a tile is a run-time index).
    // The workgroup shares its SIMDs with tile workgroups that would leave it an eighth of the issue slots: top priority.
    __builtin_amdgcn_s_setprio(3);
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t per = (((tiles + 127u) / 128u) + 15u) & ~15u, t0 = tid * per;
    uint32_t *s_cnt = s_scratch;                     // [PX_CLASSES][128]
    uint32_t *s_tot = s_scratch + PX_CLASSES * 128;  // [2][PX_CLASSES]
#pragma unroll
    for (uint32_t q = 0; q < PX_CLASSES; ++q) s_cnt[q * 128 + tid] = 0;
    for (uint32_t i = 0; i < per; i += 16) {
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = reinterpret_cast<const uint4 *>(cost + t0 + i)[j];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t c = reinterpret_cast<const uint32_t *>(v)[j];
            if (t0 + i + j < tiles) s_cnt[px_cost_class(c) * 128 + tid] += 1u; // (this thread's own words: no atomics)
        }
    }
    // exclusive scan over the threads, per class; then the classes one after the other
    uint32_t base[PX_CLASSES];
#pragma unroll
    for (uint32_t q = 0; q < PX_CLASSES; ++q) {
        const uint32_t mine = s_cnt[q * 128 + tid];
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t x = __shfl_up(incl, d);
            if ((int)lane >= d) incl += x;
        }
        if (lane == 63) s_tot[w * PX_CLASSES + q] = incl; // the wave's total
        base[q] = incl - mine;
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (uint32_t q = 0; q < PX_CLASSES; ++q) {
        const uint32_t c0 = s_tot[q], c1 = s_tot[PX_CLASSES + q];
        s_cnt[q * 128 + tid] = base[q] + run + (w ? c0 : 0u); // where this thread's next tile of class q goes
        run += c0 + c1;
    }
    for (uint32_t i = 0; i < per; i += 16) {
        uint4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = reinterpret_cast<const uint4 *>(cost + t0 + i)[j];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t c = reinterpret_cast<const uint32_t *>(v)[j];
            const uint32_t t = t0 + i + j;
            if (t < tiles) {
                uint32_t *slot = &s_cnt[px_cost_class(c) * 128 + tid];
                const uint32_t pos = *slot;
                *slot = pos + 1u;
                order[pos] = t;
            }
        }
    }
}

#ifndef PX_WAVES
#define PX_WAVES 5 // (tuning knob of tools/build_variant.sh: minimum waves per SIMD the register allocation must leave room for; LDS allows 5)
#endif
// One workgroup of TWO waves per tile.  Wave 1, the BUILDER, gathers the list's entries (two chunks ahead of their use)
// and per chunk of 32 builds the tables, the colours and the queue words into one of AH + 1 LDS buffers; wave 0, the
// CONSUMER, owns the tile's 256 pixels (2x2 per lane) and walks them.  One s_barrier per chunk: at barrier k the consumer
// has finished chunk k - 1 and the builder chunk k + AH - 1.
//
// Round 4, what changed and why (profiles/r04_*; DESIGN.md "k_composite_px"):
//   * the tables by RECURRENCE.  Along an axis the Gaussian at pixel pairs p0, p0 + 1, ... is G(u + 2k) = G(u) R(u),
//     R(u + 2k) = R(u) D with R(u) = exp2(-4k(u + k)), D = exp2(-8k^2): five v_exp_f32 seed a lane's table at the FIRST
//     COVERED pair of its entry (inside the box the Gaussian is >= exp(-4.5): nothing underflows) and every further pair
//     costs two packed multiplies instead of two exponentials, a packed multiply-add and a packed square; only the covered
//     pairs are written (the consumer's queues never send a lane to an uncovered pair), and the two half-covered edge
//     pairs get their zero by a masked 4-byte store instead of an and-mask on all sixteen values.  In binary32 the
//     recurrence is no less accurate than the direct form it replaces (worst case over 4e5 random entries: 2.1e-6
//     absolute against 2.6e-6 — the direct form cancels in x k - c k —; tools/px_recurrence_error.py).
//   * AH = 2: the builder stays TWO chunks ahead and a lane whose queue for chunk k is empty goes on with its queue for
//     chunk k + 1 (per-pixel order is the list's order either way).  A chunk's trips are its LONGEST queue's length; lanes
//     that ran ahead shorten the next chunk's.
//   * nothing is built that the previous frame did not need, and one chunk more than that is gathered: every launch
//     leaves each tile's cost (chunks touched) behind, and the next launch over the same band builds only that many chunks
//     ahead of need (`lim`).  A tile that turns out to need more — the camera moved — finds the next chunk's records in
//     registers, pays its build at the first chunk past the prediction (both waves meet at one extra barrier) and runs
//     eagerly from there.
//   * both waves execute the same barriers by construction: the consumer's "every pixel has stopped" is latched into
//     s_done[(k + 1) & 1] BEFORE barrier k + 1 and read by the builder AFTER it — the word the consumer may write while
//     walking chunk k + 1 is the other one.
// a tile that has come this far is one of the long ones the kernel's end waits for: its waves go first (measured worth nothing
// either way once the tiles are dispatched longest first: profiles/r04_i_px_priority_variants_C2.txt; kept: it costs nothing)
#define PX_PRIORITY(N)                                         \
    do {                                                       \
        if ((N) == 3u) __builtin_amdgcn_s_setprio(1);          \
        else if ((N) == 6u) __builtin_amdgcn_s_setprio(2);     \
        else if ((N) == 10u) __builtin_amdgcn_s_setprio(3);    \
    } while (0)
// clamp(a b + c, 0, 1) per component in one fused operation (the clamp is the instruction's output modifier).  Packed: with
// this kernel compiled WITHOUT the packed f32 instructions (-target-feature -packed-fp32-ops: 42 plain instead of 26 vector
// instructions per trip) a trip took 435 instead of 387 cycles, 348 instead of 285 for a wave alone on its SIMD
// (profiles/r04_o_trip_cost_C2.txt): a trip costs its instruction count.
__device__ __forceinline__ v2f fma_clamp01(v2f a, v2f b, v2f c) {
    v2f r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Whether any of a lane's four pixels still accumulates: T > T_STOP compared as bit patterns — for T >= 0 the same as the float
// comparison, and a pixel whose T went negative or NaN (it took a NaN Gaussian: see the builder) still counts, as a NaN alpha
// never reaches the reference's 0.99 (:187-190) and that pixel walks the whole list.  (As many instructions as the float form.)
__device__ __forceinline__ bool px_any_live(const v2f *T) {
    const uint32_t m = max(max(__float_as_uint(T[0].x), __float_as_uint(T[0].y)), max(__float_as_uint(T[1].x), __float_as_uint(T[1].y)));
    return m > __float_as_uint(T_STOP);
}

// AOV: also the auxiliary outputs (splat_aov).  The builder leaves {depth, splat index} of each entry of a chunk in s_aov
// (slot 0: the idle entry), the consumer reads it beside the entry's tables and keeps, per pixel, sum w z, sum w and the
// largest w with its index — w being the colour's own T g m.
// AOV, per pixel: the entry with the largest weight so far (strictly larger: on a tie the earlier one stays)
__device__ __forceinline__ void px_top(v2f w, uint32_t id, v2f &wmax, v2u &idmax) {
    const bool t0 = w.x > wmax.x, t1 = w.y > wmax.y;
    wmax = (v2f){t0 ? w.x : wmax.x, t1 ? w.y : wmax.y};
    idmax = (v2u){t0 ? id : idmax.x, t1 ? id : idmax.y};
}
__device__ __forceinline__ void px_aov_store(const CompositeParams &p, size_t o, float T_end, float zw, float ws, uint32_t id) {
    if (p.aov_alpha) p.aov_alpha[o] = 1.0f - T_end;
    if (p.aov_depth) p.aov_depth[o] = ws > 0.0f ? zw / ws : __builtin_inff();
    if (p.aov_id) p.aov_id[o] = id;
}

template <bool EARLY_OUT, bool LIT32, bool COUNT, int AH, bool DISC, bool AOV = false, bool ELL = false>
// (the AOV instantiations' sixteen more accumulators per lane do not fit the register budget of PX_WAVES waves per SIMD
// without spilling: they are allowed the budget of four)
__global__ __launch_bounds__(128, AOV ? 4 : PX_WAVES) void k_composite_px(CompositeParams p, uint32_t band_tiles) {
    constexpr uint32_t NB = AH + 1;
    typedef typename PxBufOf<DISC>::type Buf;
    constexpr uint32_t BUF_BYTES = NB * sizeof(Buf) > PX_ORDER_SCRATCH ? NB * sizeof(Buf) : PX_ORDER_SCRATCH;
    __shared__ __attribute__((aligned(16))) char s_raw[BUF_BYTES];
    Buf *const s_buf = reinterpret_cast<Buf *>(s_raw);
    __shared__ uint32_t s_done[2];
    __shared__ float2 s_aov[AOV ? NB : 1][PXC + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)); // 0 = consumer, 1 = builder (wave-uniform)
    if (blockIdx.x == 0) { // not a tile: the frame's report, and the next launch's tile order
        if (p.report && tid == 0) tile_report(p.frame_total, p.report, p.report_seq);
        if (p.order_dst) px_make_order(p.order_src, band_tiles, p.order_dst, reinterpret_cast<uint32_t *>(s_buf));
        return;
    }
    // (dealing the order's positions so that eight neighbouring tiles of a cost class — which gather many of the same records — run
    // behind ONE XCD's L2 changes nothing: C1 / C2 / C3 31.5 / 50.0 / 117.3 -> 30.8 / 49.3 / 117.6 us, profiles/r05_d_px_xcd_groups.txt)
    const uint32_t t_local = p.tile_order ? p.tile_order[blockIdx.x - 1u] : blockIdx.x - 1u;
    const uint32_t tx = t_local % p.ntx, ty = t_local / p.ntx + p.tile_row0;
    const uint32_t tile_idx = ty * p.ntx + tx; // ComputeShaderRenderer.ts:161-163
#ifdef PX_PROFILE
    const uint32_t count = min(p.counts[tile_idx], p.debug_cap), off = p.offsets[tile_idx];
#else
    const uint32_t count = p.counts[tile_idx], off = p.offsets[tile_idx];
#endif
    const uint32_t nchunks = (count + PXC - 1) / PXC;
    const float tile_x0 = (float)(tx * CT), tile_y0 = (float)(ty * CT);
    // chunks built and gathered ahead of need: what the previous launch over this band walked for this tile, at least one, at
    // most all.  Both waves derive the same value: it decides where they meet.  (Chunks of slack on top of it lose: every
    // tile then builds a chunk it does not walk — 54.6 against 47.2 us at C2, profiles/EXPERIMENTS.md §7.1.)
    uint32_t lim = nchunks;
    if (p.cost_prev) lim = min(max(p.cost_prev[t_local], 1u), nchunks);
    lim = (uint32_t)__builtin_amdgcn_readfirstlane((int)lim);

    if (role == 1) {
        // ================================================= builder =================================================
        if (count == 0) return; // (the consumer writes the background; no barrier is executed by either wave)
        const uint32_t e = lane & 31, h = lane >> 5; // lane (e, h) computes entry e's x (h = 0) or y (h = 1) table
        const float tile_c = (h ? tile_y0 : tile_x0) + 0.5f, tile_0 = h ? tile_y0 : tile_x0; // :169 pixel centres, this lane's axis
        if constexpr (DISC) {
            if (lane < 3 * NB) s_buf[lane / 3].par[0][lane % 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // the idle entry of every buffer
        } else if (lane <= PX_TROWS) { // the idle slots of every buffer
#pragma unroll
            for (uint32_t b = 0; b < NB; ++b) {
                if (lane < PX_TROWS) s_buf[b].t[lane][0] = make_float2(0.0f, 0.0f);
                else s_buf[b].col[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        if constexpr (AOV) {
            if (lane < NB) s_aov[lane][0] = make_float2(0.0f, __uint_as_float(0xffffffffu)); // the idle entry
        }
        // Entries are fetched two chunks ahead of their build and their indices three (the gather depends on the index).
        // Every load of this pipeline is UNCONDITIONAL — positions past the last one wanted re-read that one (one line for
        // the whole wave) and are ignored — and nothing is computed from a loaded value before its chunk comes up: a load
        // under a branch, or a use at issue, would make the compiler wait for everything in flight (s_waitcnt vmcnt(0))
        // where it can otherwise count.
        PxRaw ra = {}, rb = {}, rc = {};
        // last list position gathered without being asked for: one chunk beyond the last one BUILT ahead of need, so that a tile
        // which turns out to need one more chunk than the previous frame (the camera moved) finds its records in registers
        // already and pays a build, not a gather
        uint32_t fetch_lim = min(count, (lim + 1u) * PXC) - 1u;
        uint32_t idx_c = p.indices[off + min(2 * PXC + e, fetch_lim)];
// (AOV: the depth as unconditionally as the records — the host points aov_z at a valid word with stride 0 when it is not wanted)
#define PX_FETCH(IDX, DST)                                                                                 \
    do {                                                                                                   \
        const uint32_t i_ = (IDX);                                                                         \
        if constexpr (DISC) px_fetch_disc<ELL>(p, i_, DST); else px_fetch<LIT32>(p, i_, DST);                   \
        if constexpr (AOV) DST.zi = make_float2(p.aov_z[(size_t)i_ * p.aov_zstride], __uint_as_float(i_)); \
    } while (0)
        PX_FETCH(p.indices[off + min(e, fetch_lim)], ra);
        PX_FETCH(p.indices[off + min(PXC + e, fetch_lim)], rb);
        uint32_t staged = min(2u * PXC, fetch_lim + 1u);
        uint32_t built = 0; // chunks built so far = the next one to build
#ifdef PX_PROFILE
        const unsigned long long pb0 = __builtin_amdgcn_s_memtime();
        unsigned long long pb_wait = 0, pb_chunks = 0;
#endif
        for (uint32_t k = 0;;) { // before barrier k: every chunk below min(k + AH, lim) is built
            const uint32_t due = min(k + (uint32_t)AH, lim);
            while (built < due) {
                const uint32_t m = built, cb0 = m * PXC;
                PX_PRIORITY(m);
                PX_FETCH(idx_c, rc); // chunk m + 2
                idx_c = p.indices[off + min(cb0 + 3 * PXC + e, fetch_lim)];
                if (COUNT) staged = max(staged, min(cb0 + 3 * PXC, fetch_lim + 1u));
                Buf &B = s_buf[m % NB];
                float4 b, colr;
                float rad;
                if constexpr (DISC) { // the disc's exact screen bounds (what the binner's tile ranges came from); a culled or degenerate record has none
                    const DiscRecord drec = {ra.a, ra.a2};
                    rad = disc_bounds(drec, b) ? 1.0f : 0.0f;
                    colr = (p.prelit || p.disc_lit) ? ra.c : lit_color(ra.c, ra.n);
                } else {
                    px_unpack<LIT32>(p, ra, b, rad, colr);
                }
                // this lane's axis only: its span of covered pixel columns (rows), span_mask16's arithmetic; the other axis's
                // comes from the partner lane (e, 1 - h) — v_permlane32_swap, one instruction — because an entry that misses
                // the tile on EITHER axis draws nothing in it (ComputeShaderRenderer.ts:118-121)
                const float lo = h ? b.y : b.x, hi = h ? b.w : b.z;
                // The tables below are a recurrence seeded at the first covered pair, which holds only while the seed
                // exp2(-u0^2) is a normal float and R = exp2(-4k(u + k)) stays finite.  A projector record (box c +- 1.5 r)
                // starts at |u0| <= 6; a free box from the staged API may start far further out (c - 100 r: G underflows to
                // 0, R overflows, and the table holds 0 * inf = NaN, or zeros where the Gaussian is 1).  So the span starts
                // no further than 3.25 r left of the centre: pixels beyond have a per-axis factor < 2^-30, so 1 - g is 1 in
                // binary32 and their contribution is below 2^-30 of a colour — the same to the last bit for T, and far
                // inside the tolerance for colour.  For projector records this bound never bites (1.75 r >= 0.875 px of
                // margin), so their images are unchanged.  (fmaxf drops a NaN centre or radius: the span stays as it was.
                // DISC: rad is a flag there, and the disc's tables are not a recurrence.)
                const float reach = DISC ? -INFINITY : ceilf((lo + hi) * 0.5f - 3.25f * rad - tile_c);
                const float fa = fmaxf(fmaxf(ceilf(lo - tile_c), reach), 0.0f);
                const float fb = fminf(floorf(hi - tile_c), 15.0f);
                const uint32_t ia = (uint32_t)fminf(fa, 15.0f), ib = (uint32_t)fmaxf(fb, 0.0f); // (in range whatever the bounds: an empty span is rejected below)
                uint32_t own = ((2u << ib) - 1u) & ~((1u << ia) - 1u);
                if (!(fa <= fb) || !(cb0 + e < count) || rad < 0.5f) own = 0; // (NaN bounds;) past the list's end; :127-129 "too small"
                const v2u sw = __builtin_amdgcn_permlane32_swap(own, own, false, false);
                const uint32_t m16 = (h ? sw.x : sw.y) ? own : 0u; // covered columns (rows); zero unless the entry draws something in this tile
                if constexpr (DISC) {
                    // the inverse homography of the entry (disc.h: (u, v) = B d / (1 - q.d)) and its lit colour, as the consumer reads them
                    if (h == 0) {
                        B.par[1 + e][0] = make_float4(ra.a.x, ra.a.y, -ra.a2.z, -ra.a2.w);
                        B.par[1 + e][1] = make_float4(ra.a.z, ra.a2.x, ra.a.w, ra.a2.y); // B by columns
                    } else {
                        // (ELL: alpha = opacity g — the colour premultiplied by the opacity, and the opacity where the disc's
                        // 1 stands: T loses o T g, C gains c o T g)
                        if (ELL) B.par[1 + e][2] = make_float4(colr.x * colr.w, colr.y * colr.w, colr.z * colr.w, colr.w);
                        else B.par[1 + e][2] = make_float4(colr.x, colr.y, colr.z, 1.0f);
                    }
                } else {
                const uint32_t p0 = ia >> 1, npairs = m16 ? (ib >> 1) - p0 + 1u : 0u;
                // gaussian = exp(-0.5 (dist / r)^2 / 0.25) = exp2(-((dx k)^2 + (dy k)^2)), k = sqrt(2 log2 e) / r (:133-140), one
                // axis per lane, in tile-local coordinates.  u = (pixel centre - splat centre) k at the first covered pair's two
                // pixels; v_rcp_f32, 1 ulp: the correctly rounded quotient costs ten instructions on this wave's path.
                float k1 = 1.6986436005760381f * __builtin_amdgcn_rcpf(rad);
                const float cl = (lo + hi) * 0.5f - tile_0; // :124, then exact
                float u0 = ((float)(2u * p0) + 0.5f - cl) * k1, bias = 0.0f;
                if constexpr (EARLY_OUT) {
                    // A NaN Gaussian (NaN radius or centre on either axis, or an infinite centre with r = inf: NaN in the sum of
                    // the four bounds times k — the same for both lanes of the entry) must reach only the pixels still
                    // accumulating.  The consumer stops a pixel by a factor (w = T g m, m = 0 once T <= T_STOP), and NaN * 0 is
                    // NaN: a pixel that had stopped would turn NaN where the reference has left its loop (:187-190).  So such an
                    // entry's table is 2^60 on both axes (u = k = 0, bias 60: g = 2^120, finite): a stopped pixel takes
                    // T g 0 = 0, a live one w = T g >= T_STOP 2^120, which drives its T below zero — it then takes nothing
                    // more, and is written as NaN, what the reference's NaN gives (px_any_live keeps it walking the list).
                    const bool nan_g = __builtin_isnan(((b.x + b.z) + (b.y + b.w)) * k1);
                    u0 = nan_g ? 0.0f : u0;
                    k1 = nan_g ? 0.0f : k1;
                    bias = nan_g ? 60.0f : 0.0f;
                }
                const float u1 = u0 + k1, u2 = u1 + k1, k4 = 4.0f * k1;
                v2f G = {__builtin_amdgcn_exp2f(__builtin_fmaf(-u0, u0, bias)), __builtin_amdgcn_exp2f(__builtin_fmaf(-u1, u1, bias))};
                v2f R = {__builtin_amdgcn_exp2f(-(k4 * u1)), __builtin_amdgcn_exp2f(-(k4 * u2))}; // G(u + 2k) / G(u)
                const float Dd = __builtin_amdgcn_exp2f(-2.0f * (k4 * k1));                        // R(u + 2k) / R(u)
                const v2f D = {Dd, Dd};
                // (24-bit multiply: v_mul_lo_u32 is a quarter-rate instruction)
                float2 *row = reinterpret_cast<float2 *>(reinterpret_cast<char *>(&B.t[h * 8][1 + e]) + __umul24(p0, PX_ROW * 8u));
                // (nested: the set of lanes still writing only shrinks, and the loop ends with the wave's longest span)
#define PX_PAIR(I, REST)                                        \
    if (npairs > (I)) {                                         \
        row[(I) * PX_ROW] = make_float2(G.x, G.y);              \
        G *= R;                                                 \
        R *= D;                                                 \
        REST                                                    \
    }
                PX_PAIR(0, PX_PAIR(1, PX_PAIR(2, PX_PAIR(3, PX_PAIR(4, PX_PAIR(5, PX_PAIR(6, PX_PAIR(7, ))))))))
#undef PX_PAIR
                // the box test (ComputeShaderRenderer.ts:118-121, exact: span_mask16's set) on the two pairs the span may
                // cover by half: the uncovered pixel's factor is zero
                if (m16 && (ia & 1u)) row[0].x = 0.0f;
                if (m16 && !(ib & 1u)) reinterpret_cast<float2 *>(reinterpret_cast<char *>(row) + __umul24(npairs - 1u, PX_ROW * 8u))->y = 0.0f;
                // the lit colour beside the tables ({r, g | b, 1}: the 1 is the factor of T's update, PX_BLEND), a half per lane
                reinterpret_cast<float2 *>(&B.col[1 + e])[h] = h ? make_float2(colr.z, 1.0f) : make_float2(colr.x, colr.y);
                }
                if constexpr (AOV) {
                    if (h == 0) s_aov[m % NB][1 + e] = ra.zi;
                }
                // queue words: one ballot gives X[c] (lanes 0..31 test the x mask) and Y[c] (lanes 32..63 the y mask)
                const uint32_t mm = m16 | (m16 >> 1);
                unsigned long long bal[8];
#pragma unroll
                for (int c2 = 0; c2 < 8; ++c2) bal[c2] = __ballot((mm >> (2 * c2)) & 1u);
                if (lane == 0) {
#pragma unroll
                    for (int c2 = 0; c2 < 4; ++c2)
                        B.q4[c2] = make_uint4((uint32_t)bal[2 * c2], (uint32_t)(bal[2 * c2] >> 32), (uint32_t)bal[2 * c2 + 1], (uint32_t)(bal[2 * c2 + 1] >> 32));
                }
                ra = rb;
                rb = rc;
                ++built;
#ifdef PX_PROFILE
                pb_chunks++;
#endif
            }
#ifdef PX_PROFILE
            const unsigned long long pbw = __builtin_amdgcn_s_memtime();
#endif
            __syncthreads(); // barrier k (or the extra one after a misprediction: the consumer waits for chunk k)
#ifdef PX_PROFILE
            pb_wait += __builtin_amdgcn_s_memtime() - pbw;
#endif
            if (EARLY_OUT && __builtin_amdgcn_readfirstlane((int)s_done[k & 1])) break; // latched before this barrier
            if (k >= nchunks) break;
            if (k >= lim) {
                // the tile needs more than was predicted: chunk k's records are here (ra: gathered one chunk beyond the bound);
                // chunk k + 1's gather goes out now, chunk k (.. k + AH - 1) is built at the top of the loop, the consumer is
                // met at the extra barrier, and the tile runs eagerly from here on
                lim = nchunks;
                fetch_lim = count - 1u;
                idx_c = p.indices[off + min((k + 2u) * PXC + e, fetch_lim)];
                PX_FETCH(p.indices[off + min((k + 1u) * PXC + e, fetch_lim)], rb);
                if (COUNT) staged = max(staged, min((k + 2u) * PXC, count));
                built = k;
                continue; // (k stays)
            }
            ++k;
        }
#ifdef PX_PROFILE
        if (p.consumed && lane == 0)
            p.consumed[(size_t)tile_idx * 2] = (((__builtin_amdgcn_s_memtime() - pb0) >> 4) & 0xffffull) | (((pb_wait >> 4) & 0xffffull) << 16) |
                                               ((pb_chunks & 0xffffull) << 48);
        return;
#endif
        if (COUNT && p.consumed && lane == 0) p.consumed[(size_t)tile_idx * 2] += (unsigned long long)staged;
        return;
    }

    // ================================================= consumer ====================================================
    const uint32_t bx = lane & 7, by = lane >> 3; // this lane's 2x2 block: pixel columns 2bx, 2bx+1, rows 2by, 2by+1 of the tile
    const uint32_t px0 = tx * CT + 2 * bx, py0 = ty * CT + 2 * by;
    const bool okx0 = px0 < p.width, okx1 = px0 + 1 < p.width, oky0 = py0 < p.height, oky1 = py0 + 1 < p.height;
    // pixel (row k, column i) of the block: component i of the k-th pair.  T = transmittance; a pixel accumulates while
    // T > T_STOP (:187-190, see T_STOP); pixels outside the image start at 0 and never do
    v2f cr[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, cg[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, cb[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    v2f T[2] = {{(okx0 && oky0) ? 1.0f : 0.0f, (okx1 && oky0) ? 1.0f : 0.0f}, {(okx0 && oky1) ? 1.0f : 0.0f, (okx1 && oky1) ? 1.0f : 0.0f}};
    v2f zw[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, ws[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, wm[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}; // AOV
    v2u idm[2] = {{0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}};
    uint32_t stop_pos = 0; // COUNT: list position after the last entry this lane took while one of its pixels still accumulated
    uint32_t walked = 0;   // chunks this tile needed
    constexpr uint32_t NONE = 0xffffffffu;
    // byte offsets inside a PxBuf of slot 1 (entry 0) of this lane's x row; its y row and the colour rows relative to that
    // (DISC: slot 1 of the parameter array, the same for every lane)
    const uint32_t lane_x = DISC ? 48u : (bx * PX_ROW + 1u) * 8u;
    const uint32_t d_xy = ((8u + by - bx) * PX_ROW) * 8u;
    const uint32_t d_col = DISC ? 0u : (uint32_t)offsetof(PxBuf, col) + 16u - lane_x; // from that slot to slot 1 of the colours
    // DISC: this lane's pixel centres (:169; global coordinates, as the disc records' centres are)
    const v2f pxc = {(float)px0 + 0.5f, (float)px0 + 1.5f}, pyc = {(float)py0 + 0.5f, (float)py0 + 1.5f};
    const char *const lds = reinterpret_cast<const char *>(s_buf);
    v2f k_huge = {0x1p40f, 0x1p40f}, k_stop = {-T_STOP * 0x1p40f, -T_STOP * 0x1p40f}; // PX_BLEND's stop factor
    asm volatile("" : "+v"(k_huge), "+v"(k_stop)); // (kept in vector registers: as known constants they are moved there from scalar ones every trip)
    // PX_DISC_ROW's inside factor, (1 - d2) 2^23 + 1: 1 at d2 = 1, 0 at the next binary32 number above it, exact in one fused
    // operation (2^23 + 1 is the largest odd number a binary32 holds next to 2^23)
    v2f k_in_a = {-0x1p23f, -0x1p23f}, k_in_b = {0x1p23f + 1.0f, 0x1p23f + 1.0f};
    static_assert(0x1p23f + 1.0f == 8388609.0f, "2^23 + 1 is a binary32 number");
    if (DISC) asm volatile("" : "+v"(k_in_a), "+v"(k_in_b));
#ifdef PX_PROFILE
    const unsigned long long pc0 = __builtin_amdgcn_s_memtime();
    unsigned long long pc_wait = 0, pc_trips = 0, pc_ntrips = 0;
#endif
    if (count) {
        if (lane < 2) s_done[lane] = 0;
        bool finished = false;      // every pixel has stopped (latched in s_done for the builder)
        bool carried_ok = false;    // `carried` is what is left of this chunk's queues (the lanes ran ahead into it)
        uint32_t carried = 0;
        for (uint32_t k = 0;; ++k) {
#ifdef PX_PROFILE
            { const unsigned long long w0_ = __builtin_amdgcn_s_memtime(); __syncthreads(); pc_wait += __builtin_amdgcn_s_memtime() - w0_; }
#else
            __syncthreads(); // barrier k: chunks below min(k + AH, lim) are built; the buffer of chunk k - 1 is the builder's again
#endif
            if (EARLY_OUT && finished) break;
            if (k >= nchunks) break;
            if (k >= lim) { // chunk k was not predicted: the builder gathers and builds it now
                lim = nchunks;
                __syncthreads();
            }
            const uint32_t o0 = (k % NB) * (uint32_t)sizeof(Buf), o1 = ((k + 1u) % NB) * (uint32_t)sizeof(Buf);
            const uint32_t cb0 = k * PXC;
            walked = k + 1;
            PX_PRIORITY(k);
            const bool ahead = AH >= 2 && k + 1u < lim; // chunk k + 1 is built: lanes may run ahead into it
            // a lane whose four pixels have all stopped takes no more entries
            const bool lane_live = !EARLY_OUT || px_any_live(T);
            uint32_t mine, nxt = 0;
            {
                const uint2 *q0 = reinterpret_cast<const uint2 *>(lds + o0 + offsetof(Buf, q4));
                mine = carried_ok ? carried : (q0[bx].x & q0[by].y);
                if (ahead) {
                    const uint2 *q1 = reinterpret_cast<const uint2 *>(lds + o1 + offsetof(Buf, q4));
                    nxt = q1[bx].x & q1[by].y;
                }
                if (!lane_live) mine = nxt = 0;
                carried_ok = ahead;
            }
            const uint32_t nxt0 = nxt;
            const uint32_t ax0 = o0 + lane_x, ax1 = o1 + lane_x;
            // AOV: byte offsets of slot 1 of chunk k's and chunk k + 1's {depth, index} rows
            const uint32_t zi0 = ((k % NB) * (PXC + 1u) + 1u) * 8u, zi1 = (((k + 1u) % NB) * (PXC + 1u) + 1u) * 8u;
            // ---- trips.  Every lane takes its next entry — of chunk k while it has one, then of chunk k + 1, the idle one when
            // both queues are empty: no divergence, an idle lane adds exact zeros; the NEXT entry's table and colour reads are
            // issued before the current one is blended, so a trip costs its arithmetic, not an LDS round trip.
#define PX_POP(J, R, A, S)                                                                       \
    do {                                                                                         \
        uint32_t mc_ = mine;                                                                     \
        asm("" : "+v"(mc_)); /* (an opaque copy: left visible, the compiler derives `mine != 0` from the borrow of mine - 1 below — three instructions for one compare) */ \
        const bool sel_ = mc_ != 0;                                                              \
        R = __ballot(sel_); /* lanes that still have an entry of chunk k: none = the chunk is finished, this trip is not made */ \
        const uint32_t q_ = (AH >= 2) ? (sel_ ? mine : nxt) : mine;                              \
        asm("v_ffbl_b32 %0, %1" : "=v"(J) : "v"(q_)); /* -1 for 0 (the idle slot): no select; __builtin_ctz(0) is undefined */ \
        const uint32_t q2_ = q_ & (q_ - 1u);                                                     \
        if (AH >= 2) {                                                                           \
            mine = sel_ ? q2_ : 0u;                                                              \
            /* an entry of chunk k + 1 leaves a lane's queue only in a trip that is made (R != 0) and only while one of the lane's \
               pixels still accumulates (as of the blend before last: the walk's cost counts the chunks LIVE lanes touched);   \
               the mask is scalar work */                                                        \
            nxt = __builtin_amdgcn_inverse_ballot_w64((R ? R : ~0ull) | ~alive_m) ? nxt : q2_;   \
            A = sel_ ? ax0 : ax1;                                                                \
            if (AOV) A##_aov = sel_ ? zi0 : zi1;                                                 \
            if (COUNT) S = sel_ ? 0u : (uint32_t)PXC;                                            \
        } else {                                                                                 \
            mine = q2_;                                                                          \
            A = ax0;                                                                             \
            if (AOV) A##_aov = zi0;                                                              \
        }                                                                                        \
    } while (0)
#define PX_LOAD(J, A, E)                                                               \
    do {                                                                               \
        if constexpr (DISC) {                                                          \
            const float4 *a_ = reinterpret_cast<const float4 *>(lds + (A + (uint32_t)((int)J * 48))); \
            E.p0 = a_[0];                                                              \
            E.p1 = a_[1];                                                              \
            E.p2 = a_[2];                                                              \
        } else {                                                                       \
            const char *a_ = lds + (A + (uint32_t)((int)J * 8));                       \
            E.gx = *reinterpret_cast<const float2 *>(a_);                              \
            E.gy = *reinterpret_cast<const float2 *>(a_ + d_xy);                       \
            const float4 c_ = *reinterpret_cast<const float4 *>(lds + (A + d_col + (uint32_t)((int)J * 16))); \
            E.c0 = make_float2(c_.x, c_.y);                                            \
            E.c1 = make_float2(c_.z, c_.w);                                            \
        }                                                                              \
        if constexpr (AOV) E.zi = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(s_aov) + (A##_aov + (uint32_t)((int)J * 8))); \
    } while (0)
// The per-pixel stop (:187-190: a pixel that has reached alpha >= 0.99, i.e. T <= T_STOP, takes nothing more) as a FACTOR:
// m = clamp((T - T_STOP) 2^40, 0, 1) is exactly 1 while T > T_STOP (the smallest positive difference of two binary32 numbers
// near T_STOP is 2^-30) and exactly 0 from then on — one v_pk_fma_f32 with the clamp modifier per pixel PAIR and one packed
// multiply (w = T g m: the same bits as T g where m = 1), where a compare and a select per PIXEL stood before.
// CHECK (every other trip; every trip when the consumed entries are counted): which lanes still have a pixel accumulating —
// a lane with none gives up the rest of its queue at once, not at the next chunk, and when there is none at all the chunk's
// remaining trips are not made.  Neither changes a pixel: the factor does the stopping.
// DISC: the footprint of SequentialRenderer.ts:91-142 per pixel (disc.h): (u, v) = B d / (1 - q.d) with d = pixel centre -
// disc centre, inside when u^2 + v^2 <= 1 (:128-130), gaussian exp(-0.5 d2 / 0.16) (:132-133).  Per row of the lane's 2x2
// block the two columns go through packed arithmetic; the row's own terms (q1 dy, B01 dy, B11 dy) are scalars of it.
#define PX_DISC_ROW(DY, G)                                                                                                    \
    do {                                                                                                                      \
        const float s_ = __builtin_fmaf(E_.p0.w, DY, 1.0f);                         /* 1 - q1 dy */                            \
        const v2f den_ = (v2f){E_.p0.z, E_.p0.z} * dx_ + (v2f){s_, s_};             /* 1 - q.d   */                            \
        const v2f rd_ = {__builtin_amdgcn_rcpf(den_.x), __builtin_amdgcn_rcpf(den_.y)};                                       \
        const v2f by_ = (v2f){E_.p1.z, E_.p1.w} * (v2f){DY, DY};                    /* B01 dy, B11 dy */                       \
        const v2f nu_ = (v2f){E_.p1.x, E_.p1.x} * dx_ + (v2f){by_.x, by_.x};        /* (B d) */                                \
        const v2f nv_ = (v2f){E_.p1.y, E_.p1.y} * dx_ + (v2f){by_.y, by_.y};                                                  \
        /* :126 u^2 + v^2 = |B d|^2 / (1 - q.d)^2 — in this form no 0 * inf can arise (|B d| = 0 only at the centre, where    \
           1 - q.d = 1): a pixel on the disc plane's horizon line gets inf (outside), never NaN */                            \
        const v2f d2_ = (nu_ * nu_ + nv_ * nv_) * (rd_ * rd_);                                                                \
        const v2f ar_ = d2_ * (v2f){FootprintExp2<ELL>::scale, FootprintExp2<ELL>::scale};                                    \
        /* :128-133 discard outside the unit circle, as a factor: clamp((1 - d2) 2^23 + 1, 0, 1) is exactly 1 for d2 <= 1 and  \
           exactly 0 from the next binary32 number above 1 on (and for NaN): one packed multiply-add for two compares + selects */ \
        v2f in_;                                                                                                              \
        in_ = fma_clamp01(d2_, k_in_a, k_in_b);                                                                               \
        G = (v2f){__builtin_amdgcn_exp2f(ar_.x), __builtin_amdgcn_exp2f(ar_.y)} * in_;                                        \
    } while (0)
#define PX_BLEND(J, R, S, E, CHECK)                                                                                           \
    do {                                                                                                                      \
        const auto &E_ = E;                                                                                                   \
        v2f w0, w1;                                                                                                           \
        float2 C0, C1;                                                                                                        \
        if constexpr (DISC) {                                                                                                 \
            const v2f dx_ = pxc - (v2f){E_.p0.x, E_.p0.x};                                                                    \
            v2f g0_, g1_;                                                                                                     \
            PX_DISC_ROW(pyc.x - E_.p0.y, g0_);                                                                                \
            PX_DISC_ROW(pyc.y - E_.p0.y, g1_);                                                                                \
            w0 = T[0] * g0_;                                                                                                  \
            w1 = T[1] * g1_;                                                                                                  \
            C0 = make_float2(E_.p2.x, E_.p2.y);                                                                               \
            C1 = make_float2(E_.p2.z, E_.p2.w);                                                                               \
        } else {                                                                                                              \
            const v2f gxx = {E_.gx.x, E_.gx.y};                                                                               \
            w0 = T[0] * (gxx * (v2f){E_.gy.x, E_.gy.x});                            /* rows 2by, 2by+1: w = T g */             \
            w1 = T[1] * (gxx * (v2f){E_.gy.y, E_.gy.y});                                                                      \
            C0 = E_.c0;                                                                                                       \
            C1 = E_.c1;                                                                                                       \
        }                                                                                                                     \
        if (EARLY_OUT) {                                                                                                      \
            v2f m0, m1;                                                                                                       \
            m0 = fma_clamp01(T[0], k_huge, k_stop);                                                                          \
            m1 = fma_clamp01(T[1], k_huge, k_stop);                                                                          \
            if (CHECK) {                                                                                                      \
                const v2f ms_ = m0 + m1; /* the four factors are 0 or 1: their sum says whether any pixel of the lane still accumulates */ \
                const unsigned long long al_ = __ballot(ms_.x + ms_.y > 0.0f);                                               \
                /* COUNT: the last entry a lane takes while one of its pixels still accumulates is the one that stops its    \
                   last pixel (if they all stop) */                                                                           \
                if (COUNT) jlast = (__builtin_amdgcn_inverse_ballot_w64(al_) && J != NONE) ? J + S : jlast;                   \
                all_stopped = al_ == 0;                                                                                       \
                mine = __builtin_amdgcn_inverse_ballot_w64(al_) ? mine : 0u;                                                  \
                alive_m = al_;                                                                                                \
            }                                                                                                                 \
            w0 *= m0;                                                                                                         \
            w1 *= m1;                                                                                                         \
        }                                                                                                                     \
        if constexpr (AOV) { /* sum w z, sum w, the largest w and its index (strictly larger: the earlier entry keeps a tie) */ \
            /* (C1.y: 1 for an entry, 0 for the idle one — whose disc footprint is 1 at every pixel: w is the colour's weight \
               only once multiplied by it, exactly) */                                                                        \
            const v2f e_ = {C1.y, C1.y}, wa0 = w0 * e_, wa1 = w1 * e_;                                                        \
            const v2f z_ = {E_.zi.x, E_.zi.x};                                                                                \
            const uint32_t id_ = __float_as_uint(E_.zi.y);                                                                    \
            zw[0] = __builtin_elementwise_fma(z_, wa0, zw[0]); zw[1] = __builtin_elementwise_fma(z_, wa1, zw[1]);             \
            ws[0] += wa0; ws[1] += wa1;                                                                                       \
            px_top(wa0, id_, wm[0], idm[0]); px_top(wa1, id_, wm[1], idm[1]);                                                 \
        }                                                                                                                     \
        /* SURVEY §8a contract 3: nearest on top.  C += c w in ONE rounding (v_pk_fma_f32; this file is built, as composite.hip,    \
           with contraction on:the sum is within the composite's stated tolerance either way) */                             \
        cr[0] = __builtin_elementwise_fma((v2f){C0.x, C0.x}, w0, cr[0]); cr[1] = __builtin_elementwise_fma((v2f){C0.x, C0.x}, w1, cr[1]); \
        cg[0] = __builtin_elementwise_fma((v2f){C0.y, C0.y}, w0, cg[0]); cg[1] = __builtin_elementwise_fma((v2f){C0.y, C0.y}, w1, cg[1]); \
        cb[0] = __builtin_elementwise_fma((v2f){C1.x, C1.x}, w0, cb[0]); cb[1] = __builtin_elementwise_fma((v2f){C1.x, C1.x}, w1, cb[1]); \
        /* T (1 - g) with the product in hand; C1.y is 1.0 for an entry, 0 for the idle one: the product is exact, so this is \
           the same bits as T - w */                                                                                          \
        T[0] = __builtin_elementwise_fma((v2f){-C1.y, -C1.y}, w0, T[0]); T[1] = __builtin_elementwise_fma((v2f){-C1.y, -C1.y}, w1, T[1]); \
    } while (0)
#ifdef PX_PROFILE
            const unsigned long long pt0 = __builtin_amdgcn_s_memtime();
#endif
            uint32_t ja, jb, jlast = NONE, aa = 0, ab = 0, sa = 0, sb = 0, aa_aov = 0, ab_aov = 0;
            unsigned long long alive_m = __ballot(lane_live); // lanes with a pixel still accumulating (as of the last blend)
            bool all_stopped = false; // every pixel of the tile had stopped before the entry just blended: the rest of the chunk is zeros
            unsigned long long ra_, rb_;
            struct PxEnt { // what a trip reads of its entry: table values and colour, or (DISC) the three parameter vectors
                float2 gx, gy, c0, c1;
                float4 p0, p1, p2;
                float2 zi; // AOV
            } ea, eb;
            PX_POP(ja, ra_, aa, sa);
            PX_LOAD(ja, aa, ea);
            for (;;) {
                if (ra_ == 0) break;
#ifdef PX_PROFILE
                pc_ntrips++;
#endif
                PX_POP(jb, rb_, ab, sb);
                PX_LOAD(jb, ab, eb);
                __builtin_amdgcn_sched_barrier(0); // (the scheduler would sink the reads to their use, one trip later: the point is lost)
                PX_BLEND(ja, ra_, sa, ea, true);
                if (EARLY_OUT && all_stopped) break;
                if (rb_ == 0) break;
#ifdef PX_PROFILE
                pc_ntrips++;
#endif
                PX_POP(ja, ra_, aa, sa);
                PX_LOAD(ja, aa, ea);
                __builtin_amdgcn_sched_barrier(0);
                PX_BLEND(jb, rb_, sb, eb, COUNT);
                if (EARLY_OUT && all_stopped) break;
            }
#undef PX_POP
#undef PX_LOAD
#undef PX_BLEND
#undef PX_DISC_ROW
#ifdef PX_PROFILE
            if (__ballot(T[0].x > 1e30f) == 0) pc_trips += __builtin_amdgcn_s_memtime() - pt0;
#endif
            carried = nxt;
            // the tile's cost = the chunks it touched: if this turns out to be its last chunk and some lane took an entry of the next
            // one in passing, the next launch must find that one built as well (or the tile would need it and not have it every
            // other frame)
            if (AH >= 2) walked += __ballot(nxt != nxt0) != 0 ? 1u : 0u;
            if (COUNT && EARLY_OUT && jlast != NONE) stop_pos = cb0 + jlast + 1; // (a lane's entries come in list order: later ones overwrite)
            if (EARLY_OUT) {
                // the tile is finished when every pixel has stopped: both waves leave after the next barrier
                const bool live = px_any_live(T);
                finished = __ballot(live) == 0;
                if (finished && lane == 0) s_done[(k + 1u) & 1u] = 1;
            }
        }
    }

    if (p.tile_cost && lane == 0) p.tile_cost[t_local] = walked; // (what the next launch over this band is ordered and sized by)
#ifdef PX_PROFILE
    if (p.consumed && lane == 0)
        p.consumed[(size_t)tile_idx * 2 + 1] = (((__builtin_amdgcn_s_memtime() - pc0) >> 4) & 0xffffull) | (((pc_wait >> 4) & 0xffffull) << 16) |
                                               (((pc_trips >> 4) & 0xffffull) << 32) | ((pc_ntrips & 0xffffull) << 48);
#else
    if (COUNT && p.consumed && count) { // (uniform branch; timed / diagnostic runs only)
        uint32_t used = stop_pos;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) used = max(used, (uint32_t)__shfl_xor((int)used, d));
        const bool px_live = px_any_live(T);
        if (!EARLY_OUT || __ballot(px_live) != 0) used = count;
        if (lane == 0) p.consumed[(size_t)tile_idx * 2 + 1] += (unsigned long long)used;
    }
#endif

    // :193-197
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t py = py0 + r;
        if (py >= p.height || !okx0) continue;
        if (EARLY_OUT && !DISC) { // T < 0: the pixel took a NaN Gaussian while it accumulated (the builder's 2^60 tables)
            T[r].x = (T[r].x >= 0.0f) ? T[r].x : __builtin_nanf("");
            T[r].y = (T[r].y >= 0.0f) ? T[r].y : __builtin_nanf("");
        }
        const float r0 = cr[r].x + 0.05f * T[r].x, g0 = cg[r].x + 0.05f * T[r].x, b0 = cb[r].x + 0.1f * T[r].x;
        const float r1 = cr[r].y + 0.05f * T[r].y, g1 = cg[r].y + 0.05f * T[r].y, b1 = cb[r].y + 0.1f * T[r].y;
        const size_t o = (size_t)py * p.width + px0;
        const uint32_t q0 = unorm8(r0) | (unorm8(g0) << 8) | (unorm8(b0) << 16) | (255u << 24);
        const uint32_t q1 = unorm8(r1) | (unorm8(g1) << 8) | (unorm8(b1) << 16) | (255u << 24);
        if (p.out_rgba8) {
            if (okx1 && (o & 1) == 0) *reinterpret_cast<uint2 *>(p.out_rgba8 + o) = make_uint2(q0, q1);
            else {
                p.out_rgba8[o] = q0;
                if (okx1) p.out_rgba8[o + 1] = q1;
            }
        }
        if (p.out_rgba32f) {
            p.out_rgba32f[o] = make_float4(r0, g0, b0, 1.0f);
            if (okx1) p.out_rgba32f[o + 1] = make_float4(r1, g1, b1, 1.0f);
        }
        if constexpr (AOV) {
            px_aov_store(p, o, T[r].x, zw[r].x, ws[r].x, idm[r].x);
            if (okx1) px_aov_store(p, o + 1, T[r].y, zw[r].y, ws[r].y, idm[r].y);
        }
    }
}

bool composite_uses_px(const splat_ctx *ctx, uint32_t ntx, uint32_t nty) {
    constexpr uint32_t PX_MIN_TILES = 2048;
    static int s_px = -2; // SPLAT_COMPOSITE=pixel | quadrant: 1 | 0; unset: -1
    if (s_px == -2) {
        const char *e = getenv("SPLAT_COMPOSITE");
        s_px = !e ? -1 : (e[0] == 'p' || e[0] == 'P') ? 1 : (e[0] == 'q' || e[0] == 'Q') ? 0 : -1;
    }
    const int kernel = ctx->opt_composite_kernel >= 0 ? ctx->opt_composite_kernel : s_px;
    return kernel == 1 || (kernel == -1 && ntx * nty >= PX_MIN_TILES);
}

// (read once per process, at the first launch: composite_px_launch)
static bool g_px_order_on = true;   // SPLAT_TILE_ORDER=0: workgroups take their tiles row-major
static bool g_px_predict_on = true; // SPLAT_PX_PREDICT=0: every tile builds and gathers ahead of need without a bound
static int g_px_ahead = 0;          // SPLAT_PX_AHEAD=1 | 2: chunks the builder stays ahead (2: lanes run ahead too); unset: 1 with the early-out, 2 without

// The history of one band of one binner's lists: two cost arrays and two order arrays, alternating.  Launch k over the band
// writes cost[k & 1]; it sizes every tile's look-ahead by cost[(k + 1) & 1] (launch k - 1's), takes its tiles in order[k & 1] —
// which launch k - 1's ordering workgroup derived from cost[k & 1] as launch k - 2 had left it — and derives
// order[(k + 1) & 1] from cost[(k + 1) & 1].  All of it is a hint: any order and any bound give the same image.
// A context keeps PX_HISTORIES of them, found by `key` (the band, the screen, whose lists), least recently used evicted: two
// frames in flight on one context, a band frame next to the whole frame, virtual ranks on one context each keep theirs
// (with ONE slot they reset each other at every launch, and neither the order nor the bound ever engaged: ADVICE r4).
// (p's hint pointers come in as composite_launch initialised them: NULL)
static int px_order_prepare(splat_ctx *ctx, uint32_t band_tiles, uint64_t key, CompositeParams &p) {
    const bool predict_on = ctx->opt_px_predict >= 0 ? ctx->opt_px_predict != 0 : g_px_predict_on;
    if (!g_px_order_on && !predict_on) return SPLAT_OK;
    PxHistory *h = nullptr, *lru = &ctx->px_hist[0];
    for (auto &e : ctx->px_hist) {
        if (e.key == key) h = &e;
        if (e.last_use < lru->last_use) lru = &e;
    }
    if (!h) { // a band this context has not composited lately: the least recently used slot starts over for it
        h = lru;
        h->key = key;
        h->streak = 0;
    }
    h->last_use = ++ctx->px_clock;
    if (band_tiles > h->cap) {
        // (each array padded so that px_make_order's 128 threads read whole 64-byte groups of costs past the last tile)
        const uint32_t cap = (band_tiles + 128u * 16u + 1023u) & ~1023u;
        const int rc = device_reserve(ctx, &h->mem, &h->cap, cap, (size_t)cap * 16, "composite tile order hipMalloc");
        if (rc != SPLAT_OK) {
            if (!h->mem) h->key = 0, h->streak = 0; // (the old arrays are gone: the slot is free)
            return rc;
        }
        h->streak = 0;
        (void)hipMemsetAsync(h->mem, 0, (size_t)cap * 16, ctx->stream);
    }
    uint32_t *cost[2] = {h->mem, h->mem + h->cap}, *order[2] = {h->mem + 2 * (size_t)h->cap, h->mem + 3 * (size_t)h->cap};
    const uint32_t q = h->parity & 1u;
    p.tile_cost = cost[q];
    if (g_px_order_on && h->streak >= 2) p.tile_order = order[q]; // written by the previous launch from the costs of the one before it
    if (h->streak >= 1) {                                          // the previous launch left its costs
        if (predict_on) p.cost_prev = cost[q ^ 1u];
        if (g_px_order_on) { // sort them for the next launch
            p.order_src = cost[q ^ 1u];
            p.order_dst = order[q ^ 1u];
        }
    }
    h->parity ^= 1u;
    if (h->streak < 2) h->streak++;
#ifdef PX_PROFILE
    { // (measuring build only, SPLAT_PX_FREEZE=1: the order found by the first launches is kept and no launch computes another: is the ordering workgroup free?)
        static int freeze = -1;
        static uint32_t *frozen = nullptr;
        if (freeze < 0) freeze = getenv("SPLAT_PX_FREEZE") ? 1 : 0;
        if (freeze) {
            if (frozen && p.tile_order) { p.tile_order = frozen; p.order_src = nullptr; p.order_dst = nullptr; }
            else if (p.tile_order) frozen = const_cast<uint32_t *>(p.tile_order);
        }
    }
#endif
    return SPLAT_OK;
}

int composite_px_launch(splat_ctx *ctx, const splat_composite_cfg *cfg, CompositeParams &p, const TileBand &band, bool *launched) {
    static bool s_env = false;
    if (!s_env) {
        s_env = true;
        const char *o = getenv("SPLAT_TILE_ORDER"); // =0: workgroups take tiles row-major
        g_px_order_on = !(o && o[0] == '0');
        const char *pr = getenv("SPLAT_PX_PREDICT"); // =0: no look-ahead bound from the previous launch's costs
        g_px_predict_on = !(pr && pr[0] == '0');
        const char *ah = getenv("SPLAT_PX_AHEAD");
        g_px_ahead = !ah ? 0 : ah[0] == '1' ? 1 : 2;
    }
#ifdef PX_PROFILE
    p.debug_cap = getenv("SPLAT_PX_CAP") ? (uint32_t)strtoul(getenv("SPLAT_PX_CAP"), nullptr, 10) : 0xffffffffu;
#endif
    const bool eo = cfg->early_out != 0, want_aov = p.aov_depth || p.aov_alpha || p.aov_id;
    // Two chunks ahead with lanes running ahead makes 27 % fewer trips, each four instructions longer, on five waves per
    // SIMD instead of eight (three table buffers): a gain where every list is walked to its end (early-out off: C2 319 ->
    // 298 us), a loss where most tiles stop after a few chunks and a tile's life is mostly latency (50.6 -> 52.8 us):
    // profiles/r04_b_px_ab_C2.txt
    // (the oriented disc keeps eleven numbers per entry instead of tables: a third buffer costs it no resident workgroup)
    const int ahead = ctx->opt_px_ahead > 0 ? ctx->opt_px_ahead : g_px_ahead > 0 ? g_px_ahead : ((eo && !p.disc) ? 1 : 2);
    const uint32_t r0 = band.row0, r1 = band.row1, band_tiles = band.ntx * (r1 - r0);
    // (the band, the screen, and whose lists these are: two binners on one context do not share a history)
    const uint64_t key = (((uint64_t)band.ntx << 40) ^ ((uint64_t)r0 << 20) ^ (uint64_t)r1 ^ ((uint64_t)p.width << 50) ^
                          ((uint64_t)(uintptr_t)p.counts * 0x9E3779B97F4A7C15ull)) | 1u;
    const int orc = px_order_prepare(ctx, band_tiles, key, p);
    if (orc != SPLAT_OK) return orc;
#ifdef SPLAT_TEST_HOOKS
    if (ctx->debug_tile_order) p.tile_order = ctx->debug_tile_order;
#endif
    // one workgroup of two waves (consumer, builder) per tile, behind workgroup 0 (report, next launch's tile order)
    const bool ok = variant_dispatch(
        [&](auto eo_, auto lit, auto cnt, auto ah, auto disc, auto aov, auto ell) {
            if constexpr (composite_px_variant_exists(disc.value, lit.value, ell.value)) {
                launch_kernel(ctx, SPLAT_STAGE_COMPOSITE, k_composite_px<eo_.value, lit.value, cnt.value, ah.value, disc.value, aov.value, ell.value>,
                              dim3(band_tiles + 1u), dim3(128), p, band_tiles);
                return true;
            } else return false;
        },
        eo, p.lit32 && !p.disc, p.consumed != nullptr, OneOf<1, 2>{ahead == 2 ? 2 : 1}, p.disc != 0, want_aov,
        footprint_is_ell(cfg->footprint));
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "k_composite_px: no kernel for this footprint and record format");
    *launched = hipPeekAtLastError() == hipSuccess; // (only a launch that went out carries the frame's report)
    LAUNCH_CHECK(ctx, "k_composite_px");
    return SPLAT_OK;
}

#ifdef SPLAT_TEST_HOOKS // (the test build only: include/splat.h)
extern "C" int splat_debug_set_tile_order(splat_ctx *ctx, const void *order_dptr) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ctx->debug_tile_order = (const uint32_t *)order_dptr;
    return SPLAT_OK;
}
#endif
