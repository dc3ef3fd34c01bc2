// tile_first.hip — the frame path's binner: bin FIRST (in index order), depth-sort each tile's list after.
//
// Reference stages: GPUTileBinner.binSplats (/root/reference/src/GPUTileBinner.ts:190-338) followed by
// PerTileSorter.sort (/root/reference/src/PerTileSorter.ts:66-122, src/shaders/sort-tile-splats.wgsl) — the
// reference's own plan bins and then re-sorts every tile's list by depth.  The result contract is
// unchanged: tile t's list is the stable depth order (key, then splat index) restricted to t, i.e.
// TileBinner.binSorted (src/TileBinner.ts:426-495) applied to the stably sorted order.
//
// Why this order on MI355X: the sort-first path pays a 4-pass global sort of N keys and then gathers
// each splat's tile range in sorted (= random) order, which is bound by every CU's L1 fill rate
// (80 us for 5M splats).  Here nothing is gathered: pairs are expanded from the projector's per-index
// arrays with coalesced reads, each pair carrying its own (depth key, index) as an 8-byte payload
// through the 2-pass tile-id sort, and the depth order is established inside each tile by one
// workgroup sorting a few thousand elements in LDS.
//
//   (projector)     per 1024-splat block: pairs per low tile-id digit (first-pass histogram)
//   k_radix_rowscan digit rows -> block bases, digit totals
//   k_tf_scatter    expansion fused with the first sort pass      N*8 B read, P*9 B written
//   k_tf_upsweep2 / k_radix_rowscan / k_tf_downsweep2
//                   second (high digit) pass, 8-byte payload      P*(1 + 9 + 8) B
//                   + tile offsets from the second pass's scanned histogram (no search, no sorted tile ids): the
//                   downsweep launch's last workgroups (tf_offsets_block)
//   k_tile_sort     per tile: LSD radix on (key - tile min key)    P*8 B read, P*4 B written      (tile_sort.hip)
#include "common.h"
#include "tile_range.h"
#include "block_scan.h"
#include "variant.h"

constexpr uint32_t TF_THREADS = 256, TF_WAVES = TF_THREADS / 64;
constexpr uint32_t TF_STAGE = 4096; // pairs staged per block for contiguous stores
static_assert(TF_BLOCK_LARGE == 1024 && TF_BLOCK_SMALL == 256, "the stage word packs the block-local slot in 10 bits; blocks are 256 x {4, 1}");

// ---------------------------------------------------------------------------------------------
// The pairs are never written in expansion order: a 1024-splat block IS a partition of the tile-id
// sort's first pass.  The projector (project.hip: k_project_hist; frame.hip: k_band_prepare_tf for a
// multi-GPU band) counts the block's pairs per low tile-id digit while the tile rectangle is in
// registers (the upsweep's histogram); k_tf_scatter expands the block into LDS, ranks the pairs by
// that digit and scatters (tile id | depth key, index) to their first-pass positions (the downsweep).
// Saved per frame: the expanded array's write and two reads (12 + 4 + 12 B per pair).
//
// Order inside a block: ascending splat index, then row-major over the splat's tile rectangle; the
// stable passes keep it inside each tile, so equal depth keys still resolve by ascending index.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t TFS_ITEMS = TF_STAGE / TF_THREADS; // 16 staged pairs per thread and round

struct TfScatterShared {
    uint32_t wave_hist[TF_WAVES][256];
    uint32_t digit_base[256];  // round-local start of each digit's run
    uint32_t global_base[256]; // where this block's pairs of each digit start in the output (advances per round)
    uint32_t wave_sums[TF_WAVES];
};

// d_total (out): [0] = pair total of this frame (the sum of the digit totals); [2] = the count the
// later kernels work on: the total, or 0 when it exceeds pair_limit (then nothing is written and
// the overflow flag is raised: the frame is rendered again with room).
// TF_PER_THREAD splats per thread: 4 (1024-splat blocks) or 1 (256-splat blocks of small frames, common.h).
#ifndef TF_SCATTER_WAVES
#define TF_SCATTER_WAVES 5 // (tuning knob of tools/build_variant.sh: 4 and 6 measured, profiles/r03_q_small_knobs_C2.txt)
#endif
// COMPACTED (a multi-GPU band's frame, frame.hip: k_band_prepare_tfc): a workgroup's input is not 1024 consecutive splat
// indices but the splats its band KEEPS of a group of TF_GROUP consecutive records, compacted in index order to the start of
// the group's segment of range32 / depth_keys, their indices beside them (`cidx`), their number in kept[group] — a band of
// an eighth of the screen keeps an eighth of the splats, and what this kernel costs is its workgroups, not its pairs.  The
// histogram has one column per group.  A group that keeps more than 1024 splats goes in rounds of 1024.
constexpr uint32_t TF_GROUP = 4096;
template <bool RANK_ATOMIC, uint32_t TF_PER_THREAD, bool COMPACTED = false>
__global__ __launch_bounds__(TF_THREADS, TF_SCATTER_WAVES) void k_tf_scatter(const uint32_t *__restrict__ range32,
                                                           const uint32_t *__restrict__ depth_keys, uint32_t n, uint32_t ntx,
                                                           uint32_t mask, uint32_t num_parts,
                                                           const uint32_t *__restrict__ scanned_hist,
                                                           const uint32_t *__restrict__ totals, uint32_t *__restrict__ d_total,
                                                           uint32_t pair_limit, uint32_t *__restrict__ overflow,
                                                           uint8_t *__restrict__ out_hi, uint2 *__restrict__ out_val,
                                                           uint32_t lo_bits, uint32_t align_m1, TfRuns runs,
                                                           uint32_t *__restrict__ offsets_out, uint32_t tiles, uint32_t *report,
                                                           uint32_t seq, const uint32_t *__restrict__ cidx,
                                                           const uint32_t *__restrict__ kept, uint32_t xcd_per) {
    static_assert(!COMPACTED || TF_PER_THREAD == 4, "compacted groups are read four splats per thread");
    const uint32_t blk = xcd_block_of(blockIdx.x, xcd_per); // this workgroup's block of splats = its histogram column
    if (blk >= num_parts) return;
    __shared__ TfScatterShared sh;
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t stage[TF_STAGE]; // tile id << 10 | block-local slot
    __shared__ uint32_t s_key[TF_THREADS * TF_PER_THREAD];
    __shared__ uint32_t s_idx[COMPACTED ? TF_THREADS * TF_PER_THREAD : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t first = blk * (COMPACTED ? TF_GROUP : TF_THREADS * TF_PER_THREAD);
    // (COMPACTED: n = this group's kept splats end at first + kept[group]; the loads below stop there)
    if (COMPACTED) n = first + min(kept[blk], TF_GROUP);
    // every global load of the prologue is issued before anything waits on one: the block's ranges and
    // keys, the digit totals, and this block's row of scanned histogram (measured per phase, a workgroup
    // spent 15 % of its life on the totals alone when they were loaded, scanned and waited for first)
    static_assert(TF_PER_THREAD == 4 || TF_PER_THREAD == 1, "uint4 or scalar loads");
    uint32_t i0 = first + tid * TF_PER_THREAD; // thread t owns splats first + 4t .. 4t+3 (one 16-byte load each of ranges and keys)
    uint4 rr = make_uint4(1u, 1u, 1u, 1u), kk = make_uint4(0, 0, 0, 0); // 1 = empty range
    if (TF_PER_THREAD == 1) {
        if (i0 < n) { rr.x = range32[i0]; kk.x = depth_keys[i0]; }
    } else if (i0 + 3 < n) {
        rr = reinterpret_cast<const uint4 *>(range32)[i0 >> 2];
        kk = reinterpret_cast<const uint4 *>(depth_keys)[i0 >> 2];
    } else {
        if (i0 < n) { rr.x = range32[i0]; kk.x = depth_keys[i0]; }
        if (i0 + 1 < n) { rr.y = range32[i0 + 1]; kk.y = depth_keys[i0 + 1]; }
        if (i0 + 2 < n) { rr.z = range32[i0 + 2]; kk.z = depth_keys[i0 + 2]; }
    }
    const uint32_t digit_total = totals[tid];
    const uint32_t row_prefix = tid <= mask ? scanned_hist[(size_t)tid * num_parts + blk] : 0u;

    // digit starts = exclusive scan of the digit totals, each rounded up to whole partitions of the second pass when
    // there is one (align_m1 = TF2_PART - 1: every partition then holds pairs of ONE low digit, see k_tf_downsweep2);
    // the sum of the totals themselves is this frame's pair total
    const uint32_t digit_room = (digit_total + align_m1) & ~align_m1;
    // (the frame's pair total in 64 bits: a sum that wrapped would pass the `fits` test below with a small value and let
    // the scatter write out of bounds; k_radix_rowscan saturates each digit's total at 2^30)
    const auto [gincl, aincl, g64] = wave_inclusive_scan(digit_total, digit_room, (unsigned long long)digit_total);
    __shared__ unsigned long long wsum64[4];
    if (lane == 63) {
        sh.wave_sums[w] = gincl;
        wsum[w] = aincl;
        wsum64[w] = g64;
    }
    __syncthreads(); // (one barrier: wsum is not written again before the next one)
    const uint32_t aprefix = waves_before(wsum, w);
    const unsigned long long all_pairs64 = wsum64[0] + wsum64[1] + wsum64[2] + wsum64[3];
    const uint32_t all_pairs = all_pairs64 > 0xffffffffull ? 0xffffffffu : (uint32_t)all_pairs64; // saturated: it can only fail `fits`
    const uint32_t run_start = aprefix + aincl - digit_room; // where digit tid's pairs start in the output
    if (blk == 0) {
        const bool fits = all_pairs <= pair_limit;
        if (tid == 0) {
            d_total[0] = all_pairs;
            d_total[2] = fits ? all_pairs : 0u;
            d_total[3] = 0u; // (k_tile_sort's first launch counts the tiles beyond its short class here)
            if (!fits) atomicOr(overflow, 1u);
        }
        // the second pass's view of this output: per low digit where its run starts and how many pairs it holds,
        // per partition the digit it belongs to, and the number of partitions (all zero when the pairs do not fit)
        runs.start[tid] = fits ? run_start : 0u;
        runs.total[tid] = fits ? digit_total : 0u;
        if (align_m1 && fits)
            for (uint32_t j = 0, first_part = run_start / (align_m1 + 1u); j < digit_room / (align_m1 + 1u); ++j)
                runs.part_digit[first_part + j] = (uint8_t)tid;
        if (tid == 255) *runs.parts = (align_m1 && fits) ? (run_start + digit_room) / (align_m1 + 1u) : 0u;
        // a screen of at most 256 tiles is sorted by this pass alone and its (dense) runs ARE the tiles: the tile
        // offsets go out from here (tf_offsets_block has nothing to read them from)
        if (offsets_out) {
            if (tid < tiles) offsets_out[tid] = fits ? run_start : 0u;
            if (tid == 0) {
                offsets_out[tiles] = fits ? all_pairs : 0u;
                if (report) tile_report(d_total, report, seq);
            }
        }
    }
    if (all_pairs > pair_limit) return;
    // where this block's pairs of digit tid start: digit start + the earlier blocks' share
    sh.global_base[tid] = run_start + row_prefix;
    for (;;) { // (COMPACTED: rounds of 1024 kept splats; otherwise once)
    __syncthreads(); // wave_sums and wsum are reused below (and the round before has left stage, s_key, s_idx)

    uint32_t r[TF_PER_THREAD], h[TF_PER_THREAD];
    if constexpr (TF_PER_THREAD == 4) {
        reinterpret_cast<uint4 *>(s_key)[tid] = kk;
        r[0] = rr.x; r[1] = rr.y; r[2] = rr.z; r[3] = rr.w;
        if constexpr (COMPACTED) { // the kept splats' own indices (what a pair carries)
            uint4 ii = make_uint4(0, 0, 0, 0);
            if (i0 + 3 < n) ii = reinterpret_cast<const uint4 *>(cidx)[i0 >> 2];
            else {
                if (i0 < n) ii.x = cidx[i0];
                if (i0 + 1 < n) ii.y = cidx[i0 + 1];
                if (i0 + 2 < n) ii.z = cidx[i0 + 2];
            }
            reinterpret_cast<uint4 *>(s_idx)[tid] = ii;
        }
    } else {
        s_key[tid] = kk.x;
        r[0] = rr.x;
    }
#pragma unroll
    for (uint32_t k = 0; k < TF_PER_THREAD; ++k) h[k] = range32_hits(r[k]);
    // offsets of every splat's pairs inside the block, in ascending splat index: one block scan of the
    // per-thread totals, then the thread's own running sum
    uint32_t off[TF_PER_THREAD];
    uint32_t carry;
    {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < TF_PER_THREAD; ++k) mine += h[k];
        off[0] = block_exclusive_scan<false>(mine, wsum, &carry); // (one barrier: the round's next write of wsum is behind others)
#pragma unroll
        for (uint32_t k = 1; k < TF_PER_THREAD; ++k) off[k] = off[k - 1] + h[k - 1];
    }
    const uint32_t total = carry;
    const bool more_splats = COMPACTED && first + TF_THREADS * TF_PER_THREAD < n; // (uniform) another round of this group's kept splats follows
    if (total == 0 && !more_splats) return;
    // rounds of TF_STAGE pairs (one round unless the block's splats are unusually large)
    for (uint32_t c0 = 0; c0 < total; c0 += TF_STAGE) {
        const uint32_t cnt = (total - c0 < TF_STAGE) ? total - c0 : TF_STAGE;
        for (uint32_t i = tid; i < TF_WAVES * 256; i += TF_THREADS) (&sh.wave_hist[0][0])[i] = 0;
#pragma unroll
        for (uint32_t k = 0; k < TF_PER_THREAD; ++k) {
            if (h[k] == 0 || off[k] >= c0 + TF_STAGE || off[k] + h[k] <= c0) continue;
            const TileRect t = unpack_range32(r[k]);
            const uint32_t slot = tid * TF_PER_THREAD + k;
            uint32_t o = off[k] - c0; // may wrap below zero for pairs of an earlier round: the range check rejects them
            for (uint32_t ty = t.ty0; ty <= t.ty1; ++ty)
                for (uint32_t tx = t.tx0; tx <= t.tx1; ++tx) {
                    if (o < TF_STAGE) stage[o] = ((ty * ntx + tx) << 10) | slot;
                    ++o;
                }
        }
        __syncthreads();
        // rank by digit, wave-striped positions (wave, item, lane), items in groups of four
        const uint32_t items = ((cnt + TF_THREADS - 1) / TF_THREADS + 3u) & ~3u;
        const uint32_t wbase = w * items * 64 + lane;
        uint32_t el[TFS_ITEMS], rank[TFS_ITEMS];
#pragma unroll
        for (uint32_t g = 0; g < TFS_ITEMS; g += 4) {
            if (g < items) {
#pragma unroll
                for (uint32_t i = g; i < g + 4; ++i) {
                    const uint32_t p = wbase + i * 64;
                    el[i] = stage[p < cnt ? p : cnt - 1];
                }
#pragma unroll
                for (uint32_t i = g; i < g + 4; ++i) {
                    rank[i] = 0;
                    if (wbase + i * 64 < cnt) rank[i] = wave_rank<RANK_ATOMIC>(sh.wave_hist[w], (el[i] >> 10) & mask);
                }
            }
        }
        __syncthreads();
        const uint32_t dcount = ts_wave_prefixes(sh.wave_hist, tid);
        const uint32_t excl = block_exclusive_scan<true>(dcount, sh.wave_sums);
        sh.digit_base[tid] = excl;
        __syncthreads();
        // reorder in place (every thread holds its elements in registers): digit runs become contiguous
#pragma unroll
        for (uint32_t g = 0; g < TFS_ITEMS; g += 4) {
            if (g < items) {
#pragma unroll
                for (uint32_t i = g; i < g + 4; ++i) {
                    const uint32_t d = (el[i] >> 10) & mask;
                    if (wbase + i * 64 < cnt) stage[sh.digit_base[d] + sh.wave_hist[w][d] + rank[i]] = el[i];
                }
            }
        }
        __syncthreads();
        for (uint32_t pos = tid; pos < cnt; pos += TF_THREADS) {
            const uint32_t e = stage[pos], slot = e & 1023u, d = (e >> 10) & mask;
            const uint32_t g = sh.global_base[d] + (pos - sh.digit_base[d]);
            out_hi[g] = (uint8_t)(e >> (10u + lo_bits)); // (the low digit is the run the pair sits in)
            out_val[g] = make_uint2(s_key[slot], COMPACTED ? s_idx[slot] : first + slot);
        }
        if (c0 + TF_STAGE >= total && !more_splats) break; // (the usual case: one round)
        __syncthreads();
        sh.global_base[tid] += dcount; // the next round's pairs of digit tid follow this round's
        __syncthreads();
    }
    if (!more_splats) return;
    // the group's next 1024 kept splats
    first += TF_THREADS * TF_PER_THREAD;
    {
        const uint32_t j0 = first + tid * TF_PER_THREAD;
        rr = make_uint4(1u, 1u, 1u, 1u);
        kk = make_uint4(0, 0, 0, 0);
        if (j0 + 3 < n) {
            rr = reinterpret_cast<const uint4 *>(range32)[j0 >> 2];
            kk = reinterpret_cast<const uint4 *>(depth_keys)[j0 >> 2];
        } else {
            if (j0 < n) { rr.x = range32[j0]; kk.x = depth_keys[j0]; }
            if (j0 + 1 < n) { rr.y = range32[j0 + 1]; kk.y = depth_keys[j0 + 1]; }
            if (j0 + 2 < n) { rr.z = range32[j0 + 2]; kk.z = depth_keys[j0 + 2]; }
        }
        i0 = j0;
    }
    } // (rounds of kept splats)
}

// ---------------------------------------------------------------------------------------------
// Second pass of the tile-id sort (the high digit), for the layout k_tf_scatter leaves: every low digit's run starts
// on a partition boundary, so a partition holds pairs of ONE low digit and
//   * a pair carries one byte of tile id (the high digit) instead of four,
//   * the pass writes no tile ids at all: with hist[h][p] = pairs of high digit h in partition p, scanned over p by
//     k_radix_rowscan, tile (h, l) starts at  start(h) + scanned[h][first partition of run l]  — every pair with
//     high digit h in an earlier run has a smaller tile id, every one in run l or later does not.  tf_offsets_block reads
//     the tile offsets straight out of the scanned histogram; the 65-ary search over the sorted tile ids (10 us at
//     C2) and the 45 MB of sorted ids it probed are gone, and so are 3 of every 4 key bytes the pass used to move.
// The price is up to TF2_PART - 1 unused slots at the end of each run of the first pass's output (the second pass's
// output is dense again).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t TF2_ITEMS = 16, TF2_PART = TF2_ITEMS * TF_THREADS; // 4096 pairs per partition
static_assert(TF2_PART == TF_RUN_ALIGN, "k_tf_scatter rounds every run up to whole partitions of this pass");

// partition p: which low digit's run it lies in and how many of its TF2_PART slots hold pairs (0: past the end)
__device__ __forceinline__ uint32_t tf2_valid(const TfRuns &runs, uint32_t p) {
    if (p >= *runs.parts) return 0u;
    const uint32_t d = runs.part_digit[p];
    const uint32_t left = runs.start[d] + runs.total[d] - p * TF2_PART;
    return left < TF2_PART ? left : TF2_PART;
}

__global__ __launch_bounds__(TF_THREADS) void k_tf_upsweep2(const uint8_t *__restrict__ hi, TfRuns runs, uint32_t hmask,
                                                           uint32_t num_parts, uint32_t *__restrict__ hist, uint32_t xcd_per) {
    __shared__ uint32_t lh[TF_WAVES][256];
    const uint32_t tid = threadIdx.x, w = tid >> 6, p = xcd_block_of(blockIdx.x, xcd_per);
    if (p >= num_parts) return;
    const uint32_t valid = tf2_valid(runs, p);
    if (valid == 0) { // (uniform) a column of zeros: the row scans run over all num_parts columns
        if (tid <= hmask) hist[(size_t)tid * num_parts + p] = 0;
        return;
    }
    const uint8_t *src = hi + (size_t)p * TF2_PART;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid == TF2_PART) v = reinterpret_cast<const uint4 *>(src)[tid]; // (runs start on 4096-byte boundaries)
    for (uint32_t i = tid; i < TF_WAVES * 256; i += TF_THREADS) (&lh[0][0])[i] = 0;
    __syncthreads();
    if (valid == TF2_PART) {
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = q[j] & 255u, b = (q[j] >> 8) & 255u, c = (q[j] >> 16) & 255u, d = q[j] >> 24;
            if (a == b && b == c && c == d) { // neighbours in the run often share a tile row
                atomicAdd(&lh[w][a], 4u);
            } else {
                atomicAdd(&lh[w][a], 1u);
                atomicAdd(&lh[w][b], 1u);
                atomicAdd(&lh[w][c], 1u);
                atomicAdd(&lh[w][d], 1u);
            }
        }
    } else {
        for (uint32_t i = tid; i < valid; i += TF_THREADS) atomicAdd(&lh[w][src[i]], 1u);
    }
    __syncthreads();
    hist_flush<TF_WAVES>(lh, hist, num_parts, p, hmask);
}

template <uint32_t NW>
struct TfDownsweepShared {
    uint32_t wave_hist[NW][256];
    uint32_t global_base[256]; // (where this partition's pairs of each digit start in the output) - (their local start)
    uint32_t wave_sums[TF_WAVES], wave_gsums[TF_WAVES];
};

// offsets[t] for t = 0 .. tiles (offsets[tiles] = the pair total): tile (h, l) starts at start(h) + scanned[h][first
// partition of run l].  It needs the scanned histogram only, not the second pass's output — so it is not a launch of its own
// (a dependent launch costs ~5 us whatever it does) but the work of k_tf_downsweep2's LAST workgroups, beside the partitions.
// (A screen of at most 256 tiles has no second pass: its dense runs are the tiles, and k_tf_scatter writes the offsets.)
struct TfOffsetsArgs {
    uint32_t tiles, lo_bits;
    uint32_t *offsets;
    const uint32_t *d_total;
};
// (the first 256 threads of the workgroup: one per digit / per tile of the block)
__device__ __forceinline__ void tf_offsets_block(uint32_t block, const TfOffsetsArgs &o, const TfRuns &runs, uint32_t num_parts,
                                                 const uint32_t *__restrict__ scanned, const uint32_t *__restrict__ totals, uint32_t *hstart,
                                                 uint32_t *wsums) {
    const uint32_t tid = threadIdx.x;
    if (tid >= 256u) return; // (whole waves: the barriers below count the waves that are left)
    const uint32_t t = block * 256u + tid;
    const uint32_t total = o.d_total[2];
    // start of every high digit's run in the sorted order: exclusive scan of the second pass's digit totals
    hstart[tid] = block_exclusive_scan<false>(totals[tid], wsums);
    __syncthreads();
    if (t > o.tiles) return;
    if (t == o.tiles) {
        o.offsets[t] = total;
        return;
    }
    const uint32_t h = t >> o.lo_bits, l = t & ((1u << o.lo_bits) - 1u);
    const uint32_t first_part = runs.start[l] / TF2_PART; // (an empty run starts where the next one does)
    o.offsets[t] = hstart[h] + (first_part < num_parts ? scanned[(size_t)h * num_parts + first_part] : totals[h]);
}

// NW waves per workgroup (4: sixteen pairs per thread; 8: eight)
template <bool RANK_ATOMIC, uint32_t NW>
__global__ __launch_bounds__(NW * 64, 4) void k_tf_downsweep2(const uint8_t *__restrict__ hi_in, const uint2 *__restrict__ val_in,
                                                              uint2 *__restrict__ val_out, TfRuns runs, uint32_t hmask,
                                                              uint32_t num_parts, const uint32_t *__restrict__ scanned,
                                                              const uint32_t *__restrict__ totals, TfOffsetsArgs off, uint32_t part_blocks,
                                                              uint32_t xcd_per) {
    constexpr uint32_t THREADS = NW * 64, ITEMS = TF2_PART / THREADS;
    __shared__ TfDownsweepShared<NW> sh;
    __shared__ uint2 s_val[TF2_PART];
    // the reordered pairs' digits live where the waves' counters were (every position is computed before the first digit is
    // stored): 37.9 instead of 42.3 KB, FOUR workgroups per CU instead of three
    static_assert(sizeof(sh.wave_hist) >= TF2_PART, "s_dig aliases the wave counters");
    uint8_t *const s_dig = reinterpret_cast<uint8_t *>(&sh.wave_hist[0][0]);
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (blockIdx.x >= part_blocks) { // (uniform) not a partition: a block of 256 tile offsets
        tf_offsets_block(blockIdx.x - part_blocks, off, runs, num_parts, scanned, totals, sh.global_base, sh.wave_sums);
        return;
    }
    const uint32_t p = xcd_block_of(blockIdx.x, xcd_per);
    if (p >= num_parts) return;
    const uint32_t valid = tf2_valid(runs, p);
    if (valid == 0) return;
    for (uint32_t i = tid; i < NW * 256; i += THREADS) (&sh.wave_hist[0][0])[i] = 0;
    const bool digit_thread = tid < 256u; // thread tid < 256 owns digit tid in the scans below
    const uint32_t row_prefix = (digit_thread && tid <= hmask) ? scanned[(size_t)tid * num_parts + p] : 0u; // digit tid in earlier partitions
    const uint32_t digit_total = digit_thread ? totals[tid] : 0u;                                              // ... and in the whole frame
    // wave-striped: item i of lane l of wave w is element w * ITEMS * 64 + i * 64 + l, the order the ranking preserves.
    // Slots past `valid` read the last pair and rank as digit 255 behind every real one: they end up past `valid`
    // in the reordered partition and are not written.
    const size_t base = (size_t)p * TF2_PART;
    const uint32_t wbase = w * (ITEMS * 64) + lane;
    uint32_t dig[ITEMS];
    uint2 val[ITEMS];
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        const uint32_t q = wbase + i * 64;
        const uint32_t c = q < valid ? q : valid - 1;
        dig[i] = q < valid ? (uint32_t)hi_in[base + c] : 255u;
        val[i] = val_in[base + c];
    }
    // a partition dominated by one digit (a scene bunched up in a few tile rows) ranks faster with ballots: returning
    // LDS atomics that collide on one counter serialise (block_scan.h: ranks_with_atomics)
    bool use_atomic = RANK_ATOMIC;
    if (RANK_ATOMIC) {
        const uint32_t next = (!digit_thread || tid > hmask) ? 0u : (p + 1 < num_parts) ? scanned[(size_t)tid * num_parts + p + 1] : digit_total;
        use_atomic = ranks_with_atomics(next, row_prefix, TF2_PART);
    } else {
        __syncthreads();
    }
    uint32_t rank[ITEMS];
    if (use_atomic) {
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; ++i) rank[i] = wave_rank<true>(sh.wave_hist[w], dig[i]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; ++i) rank[i] = wave_rank<false>(sh.wave_hist[w], dig[i]);
    }
    __syncthreads();
    uint32_t cs[NW];
    uint32_t dcount = 0;
    if (digit_thread) {
#pragma unroll
        for (uint32_t v = 0; v < NW; ++v) {
            cs[v] = sh.wave_hist[v][tid];
            dcount += cs[v];
        }
    }
    // exclusive scans over the 256 digits of the partition's counts (local starts) and, in the same shuffles, of the
    // frame's digit totals (where each digit's run starts in the output)
    // (written out, not block_scan.h's two-value wave_inclusive_scan: with it this kernel's address arithmetic comes out
    // differently and the second pass measured 1.1 - 1.4 % slower at C3, profiles/binner_shared_helpers_refactor.txt)
    uint32_t incl = dcount, gincl = digit_total;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(incl, s), g = __shfl_up(gincl, s);
        if ((int)lane >= s) {
            incl += t;
            gincl += g;
        }
    }
    if (digit_thread && lane == 63) {
        sh.wave_sums[w] = incl;
        sh.wave_gsums[w] = gincl;
    }
    __syncthreads();
    if (digit_thread) {
        const uint32_t wprefix = waves_before(sh.wave_sums, w), gprefix = waves_before(sh.wave_gsums, w);
        const uint32_t local_start = wprefix + incl - dcount;
        uint32_t run = local_start;
#pragma unroll
        for (uint32_t v = 0; v < NW; ++v) {
            sh.wave_hist[v][tid] = run;
            run += cs[v];
        }
        sh.global_base[tid] = gprefix + gincl - digit_total + row_prefix - local_start;
    }
    __syncthreads();
    // reorder inside the partition: same-digit pairs become contiguous, stable
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) rank[i] += sh.wave_hist[w][dig[i]]; // (now the pair's position in the partition)
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        s_val[rank[i]] = val[i];
        s_dig[rank[i]] = (uint8_t)dig[i];
    }
    __syncthreads();
    // consecutive lanes write consecutive addresses inside each digit run
#pragma unroll
    for (uint32_t j = 0; j < ITEMS; ++j) {
        const uint32_t pos = j * THREADS + tid;
        if (pos < valid) val_out[sh.global_base[s_dig[pos]] + pos] = s_val[pos];
    }
}

// The second pass and the tile offsets.  hist: 256 * num_parts + 256 words, num_parts = tf2_parts_bound(pairs bound,
// low digits).  hi_bits == 0: only the offsets (the first pass's output is final).
int tf_second_pass_launch(splat_ctx *ctx, const TfSecondPassArgs &a) {
    const uint32_t num_parts = tf2_parts_bound(a.pairs_bound, a.lo_bits);
    uint32_t *totals = a.hist + (size_t)256 * num_parts;
    if (a.hi_bits > 0) {
        const uint32_t hmask = (1u << a.hi_bits) - 1u;
        // each XCD takes a contiguous eighth of the partitions (common.h: xcd_block_of)
        const uint32_t xcd_per = xcd_grid(num_parts).xcd_per, part_blocks = xcd_grid(num_parts).grid;
        hipLaunchKernelGGL(k_tf_upsweep2, dim3(part_blocks), dim3(TF_THREADS), 0, ctx->stream, a.hi, *a.runs, hmask, num_parts, a.hist, xcd_per);
        LAUNCH_CHECK(ctx, "k_tf_upsweep2");
        int rc = radix_rowscan_launch(ctx, a.hist, num_parts, hmask + 1u);
        if (rc != SPLAT_OK) return rc;
        const TfOffsetsArgs off = {a.tiles, a.lo_bits, a.offsets, a.d_total};
        const dim3 grid(part_blocks + div_up(a.tiles + 1, 256)); // the partitions, then the blocks of tile offsets
        const bool ra = rank_atomic_ok(ctx, true); // (checked: k_tile_sort verifies every list this pass contributes to)
        // (512 threads per partition, eight pairs per thread: measured level with this, profiles/r05_b_second_pass_xcd_C3_C2.txt)
        // Workgroups per CU: four fit (37.9 KB each) and are what a pass of 7-bit digits likes (C1 22.4 -> 21.0 us, C2 level);
        // with 8-bit digits (screens beyond 2^14 tiles: C3, where a partition leaves 128-byte fragments) a fourth resident
        // workgroup LOSES — 135 -> 143 us, and two are worse still (154) —, so there 4 KB of dynamic LDS that nobody uses
        // keep it at three (profiles/r05_x_downsweep2_workgroups_per_cu.txt).
        const uint32_t pad = a.hi_bits >= 8u ? 4096u : 0u;
        variant_dispatch([&](auto ra_) { // (launch_kernel passes no dynamic LDS: this launch carries its pad itself)
            hipLaunchKernelGGL((k_tf_downsweep2<ra_.value, TF_WAVES>), grid, dim3(TF_THREADS), pad, ctx->stream, a.hi, a.val_in, a.val_out, *a.runs, hmask,
                               num_parts, a.hist, totals, off, part_blocks, xcd_per);
        }, ra);
        LAUNCH_CHECK(ctx, "k_tf_downsweep2");
    }
    return SPLAT_OK; // (hi_bits == 0: k_tf_scatter wrote the offsets itself)
}

// hist: the digit histogram the projector (k_project_hist) or the band prepare kernel counted, after
// radix_rowscan_launch (rows scanned in place, digit totals behind them)
int tf_scatter_launch(splat_ctx *ctx, const TfScatterArgs &a) {
    const uint32_t parts = div_up(a.n, a.block_splats);
    // each XCD takes a contiguous eighth of the blocks (common.h: xcd_block_of; C3: this kernel 112 -> 97 us and the second
    // pass's downsweep 145 -> 135, C2 48.5 -> 47.0 / 44.1 -> 42.6: profiles/r05_c_first_pass_projector_xcd_C3_C2.txt)
    const XcdGrid xg = xcd_grid(parts);
    if (a.cidx && a.block_splats != TF_GROUP) return ctx_fail(ctx, SPLAT_ERR_INVALID, "tf_scatter_launch: compacted input comes in groups of 4096 records");
    const uint32_t *totals = a.hist + (size_t)256 * parts;
    {
        int prc = ctx_resolve_rank_mode(ctx); // (probe of the LDS atomics' lane order, once per context)
        if (prc != SPLAT_OK) return prc;
    }
    const bool ra = rank_atomic_ok(ctx, true); // (checked: k_tile_sort verifies every list this pass contributes to)
    // splats per thread: 4, or 1 for the 256-splat blocks of small frames; compacted input (a multi-GPU band's kept splats, per
    // group of TF_GROUP records) is read four per thread
    const bool ok = variant_dispatch(
        [&](auto ra_, auto per, auto compacted) {
            if constexpr (!compacted.value || per.value == 4) {
                launch_kernel(ctx, NO_STAGE, k_tf_scatter<ra_.value, (uint32_t)per.value, compacted.value>, dim3(xg.grid), dim3(TF_THREADS), a.range32,
                              a.depth_keys, a.n, a.ntx, a.mask, parts, a.hist, totals, a.d_total, a.pair_limit, a.overflow, a.out_hi, a.out_val,
                              a.lo_bits, a.second_pass ? TF_RUN_ALIGN - 1u : 0u, *a.runs, a.second_pass ? nullptr : a.offsets_if_final, a.tiles,
                              a.report, a.seq, a.cidx, a.kept, xg.xcd_per);
                return true;
            } else return false;
        },
        ra, OneOf<4, 1>{a.block_splats == TF_BLOCK_SMALL ? 1 : 4}, a.cidx != nullptr);
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "k_tf_scatter: no kernel for this input");
    LAUNCH_CHECK(ctx, "k_tf_scatter");
    return SPLAT_OK;
}
