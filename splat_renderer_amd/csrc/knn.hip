// knn.hip — initialisation from a point cloud: per point the mean of the squared distances to its three nearest neighbours, what
// 3DGS sets a new splat's scale from (simple_knn's distCUDA2; an extension, no reference counterpart).  include/splat.h,
// "Initialisation from a point cloud", states the contract in binary32 operation by operation; tests/knn_ref.py restates it as
// brute force.  The search prunes with boxes that are true bounds of their members, so it visits fewer pairs than brute force and
// returns the same bits.
//
// splat_knn_mean_sq   k_knn_bbox (the box of the finite points: integer atomic min / max of order-preserving codes of the floats)
//                     -> k_knn_codes (63-bit Morton code per point, 21 bits per axis; a point with a non-finite coordinate gets the
//                     largest code) -> splat_sort_run on the low 32 bits, k_knn_gather_high, splat_sort_run on the high 31 (both
//                     stable: a 63-bit sort) -> k_knn_blocks (the sorted points with their indices as float4s, 64 per block, and
//                     every block's box by fminf / fmaxf) -> k_knn_groups (the box of every 64 blocks) -> k_knn_search (one wave
//                     per block of 64 queries).
// k_knn_search        A lane is a query and keeps its three smallest distances in registers.  The own block is scanned first, then
//                     the 64 blocks on either side outward in sorted order, so that the third distances shrink early, then every
//                     other block by groups.  Candidates are taken 64 at a time, one per lane, first groups and then the blocks
//                     of a group that is left: one whose box is farther from the QUERY BLOCK's box than the largest third distance
//                     of the wave is dropped there; a block that is left is tested per lane against the lane's own third distance,
//                     and scanned when the ballot of the lanes that need it is not empty.  A candidate block is one float4 per
//                     lane, broadcast with v_readlane.
// All bounds round the way d(i, j) does (the header says why that makes them lower bounds), a skip wants lb > b2 strictly, and a
// NaN bound compares false and is visited.  Nothing depends on the codes but the order of the visits.
// No kernel waits on another workgroup, every loop is bounded by the block count, no floating-point atomic, no compare-and-swap.
#include "common.h"

namespace {

constexpr uint32_t KT = 256;            // threads per workgroup of the streaming kernels
constexpr uint32_t KB = 64;             // points per block: one wave's queries, one float4 per lane as candidates
constexpr uint32_t KG = 64;             // blocks per group: the coarser level of boxes, one block per lane
constexpr uint32_t KNN_NEAR = 64;       // blocks on either side of the query block that are taken outward, before the groups
constexpr uint32_t KNN_MAX_POINTS = 1u << 30;
constexpr uint32_t KNN_AXIS_BITS = 21;  // Morton bits per axis
constexpr uint32_t KNN_SEARCH_WAVES = 4; // query blocks per workgroup of k_knn_search (they share nothing)

size_t plane_bytes(uint64_t bytes) { return (size_t)((bytes + 255) & ~(uint64_t)255); }
uint32_t knn_blocks(uint32_t n) { return div_up(n, KB); }

// order-preserving code of a float that is not a NaN: a < b  <=>  code(a) < code(b)
__device__ __forceinline__ uint32_t ordered_code(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_decode(uint32_t c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7fffffffu) : ~c); }

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; // (false for a NaN)
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// box[0..3) = codes of the minima, box[3..6) = of the maxima, over the points whose three coordinates are finite (the caller
// fills box with 0xffffffff x 3, 0 x 3).  min and max do not depend on the order: any schedule gives the same words.
__global__ __launch_bounds__(KT) void k_knn_bbox(const float *__restrict__ points, uint32_t stride, uint32_t n, uint32_t *__restrict__ box) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * KT + threadIdx.x; i < n; i += gridDim.x * KT) {
        const float *p = points + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2];
        if (finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min(lo[a]), h = wave_max(hi[a]);
        if ((threadIdx.x & 63) == 0 && l <= h) { // (a wave that saw no finite point has nothing to say)
            atomicMin(&box[a], ordered_code(l));
            atomicMax(&box[3 + a], ordered_code(h));
        }
    }
}

// bit k of v -> bit 3 k (v < 2^21)
__device__ __forceinline__ uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// keys[i] = the code's low 32 bits, payload[i] = i, high[i] = its high 31.  The codes only order the visits: any rounding here is
// as good as another, as long as it is the same on every run (it is: plain binary32 operations on the same words).
__global__ __launch_bounds__(KT) void k_knn_codes(const float *__restrict__ points, uint32_t stride, uint32_t n, const uint32_t *__restrict__ box,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ payload, uint32_t *__restrict__ high) {
    const uint32_t i = blockIdx.x * KT + threadIdx.x;
    if (i >= n) return;
    const float *p = points + (size_t)i * stride;
    const float c[3] = {p[0], p[1], p[2]};
    uint64_t code = 0x7fffffffffffffffull;
    if (finite3(c[0], c[1], c[2])) {
        code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = ordered_decode(box[a]), hi = ordered_decode(box[3 + a]);
            // (in binary64: hi - lo of two finite floats cannot overflow there)
            const double ext = (double)hi - (double)lo;
            constexpr double cells = (double)(1u << KNN_AXIS_BITS);
            double t = ext > 0.0 ? ((double)c[a] - (double)lo) / ext * cells : 0.0;
            t = t < 0.0 ? 0.0 : t > cells - 1.0 ? cells - 1.0 : t;
            code |= spread3((uint32_t)t) << a;
        }
    }
    keys[i] = (uint32_t)code;
    payload[i] = i;
    high[i] = (uint32_t)(code >> 32);
}

// between the two sort passes: the high words follow the payload.  (in and out may be the same arrays: a thread reads its own
// element before it writes it.)
__global__ __launch_bounds__(KT) void k_knn_gather_high(const uint32_t *sorted_payload, const uint32_t *__restrict__ high, uint32_t n, uint32_t *keys,
                                                        uint32_t *payload) {
    const uint32_t i = blockIdx.x * KT + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = sorted_payload[i];
    const uint32_t h = p < n ? high[p] : 0x7fffffffu;
    keys[i] = h;
    payload[i] = p;
}

// One wave per block: sorted[pos] = (x, y, z, original index).  A point with a non-finite coordinate is stored as three NaNs: every
// distance to or from it is non-finite whatever its other coordinates are, so it is no candidate and its own row is +inf either
// way.  The slots past n in the last block are NaNs with index 0xffffffff.  boxes[2 b], boxes[2 b + 1] = the block's minima and
// maxima by fminf / fmaxf, which pass over NaNs: true bounds of every member that can be a candidate (+inf / -inf when none can).
__global__ __launch_bounds__(KT) void k_knn_blocks(const float *__restrict__ points, uint32_t stride, uint32_t n, const uint32_t *__restrict__ order,
                                                   float4 *__restrict__ sorted, float4 *__restrict__ boxes) {
    const uint32_t pos = blockIdx.x * KT + threadIdx.x; // (the grid covers whole blocks: pos < blocks * KB or the wave is idle)
    const uint32_t blocks = (n + KB - 1u) / KB, b = pos / KB;
    if (b >= blocks) return; // (a whole wave)
    const float nan = __uint_as_float(0x7fc00000u);
    float x = nan, y = nan, z = nan;
    uint32_t idx = 0xffffffffu;
    if (pos < n) {
        idx = order[pos];
        if (idx < n) { // (the sorter's payload is a permutation of 0..n-1; nothing is read out of bounds if it ever were not)
            const float *p = points + (size_t)idx * stride;
            const float px = p[0], py = p[1], pz = p[2];
            if (finite3(px, py, pz)) x = px, y = py, z = pz;
        }
    }
    sorted[pos] = make_float4(x, y, z, __uint_as_float(idx));
    const float lx = wave_min(x), ly = wave_min(y), lz = wave_min(z); // (fminf(NaN, v) = v; all NaN: NaN ...)
    const float hx = wave_max(x), hy = wave_max(y), hz = wave_max(z);
    if ((threadIdx.x & 63) == 0) {
        const bool any = lx == lx; // (... which is stored as the empty box)
        boxes[2 * (size_t)b] = any ? make_float4(lx, ly, lz, 0.0f) : make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
        boxes[2 * (size_t)b + 1] = any ? make_float4(hx, hy, hz, 0.0f) : make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    }
}

// One wave per group of KG consecutive blocks: groups[2 g], groups[2 g + 1] = the box of their boxes (a true bound of every member of
// every block of the group; empty boxes change nothing).
__global__ __launch_bounds__(KT) void k_knn_groups(const float4 *__restrict__ boxes, uint32_t blocks, float4 *__restrict__ groups) {
    const uint32_t b = blockIdx.x * KT + threadIdx.x, g = b / KG;
    if (g >= (blocks + KG - 1u) / KG) return; // (a whole wave)
    const bool have = b < blocks;
    const float4 lo = have ? boxes[2 * (size_t)b] : make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
    const float4 hi = have ? boxes[2 * (size_t)b + 1] : make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    const float lx = wave_min(lo.x), ly = wave_min(lo.y), lz = wave_min(lo.z);
    const float hx = wave_max(hi.x), hy = wave_max(hi.y), hz = wave_max(hi.z);
    if ((threadIdx.x & 63) == 0) {
        groups[2 * (size_t)g] = make_float4(lx, ly, lz, 0.0f);
        groups[2 * (size_t)g + 1] = make_float4(hx, hy, hz, 0.0f);
    }
}

__device__ __forceinline__ float bcast(float v, uint32_t lane) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane)); }

// the three smallest of {b0, b1, b2, d}: d enters only when d < b2 (never for a NaN or +inf), then two compare-exchanges
__device__ __forceinline__ void knn_insert(float d, float &b0, float &b1, float &b2) {
    const float t = d < b2 ? d : b2;
    const float m1 = fminf(b1, t);
    b2 = fmaxf(b1, t);
    b1 = fmaxf(b0, m1);
    b0 = fminf(b0, m1);
}

// every member of the candidate block c against every lane's query; self: the own block, whose slot `lane` is the query itself
template <bool SELF>
__device__ __forceinline__ void knn_scan_block(const float4 *__restrict__ sorted, uint32_t c, uint32_t members, uint32_t lane, float x, float y, float z,
                                               float &b0, float &b1, float &b2) {
#pragma clang fp contract(off)
    const float4 cand = sorted[(size_t)c * KB + lane];
    auto one = [&](uint32_t j) {
        const float dx = x - bcast(cand.x, j), dy = y - bcast(cand.y, j), dz = z - bcast(cand.z, j);
        float d = (dx * dx + dy * dy) + dz * dz;
        if (SELF) d = j == lane ? INFINITY : d;
        knn_insert(d, b0, b1, b2);
    };
    if (members == KB) { // (every block but the last: a constant trip count unrolls)
#pragma unroll 8
        for (uint32_t j = 0; j < KB; ++j) one(j);
    } else {
        for (uint32_t j = 0; j < members; ++j) one(j);
    }
}

// lower bound of d(i, j) over the members j of a box, in d's own operation order
__device__ __forceinline__ float knn_box_bound(float x, float y, float z, float4 lo, float4 hi) {
#pragma clang fp contract(off)
    const float gx = fmaxf(fmaxf(lo.x - x, x - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - y, y - hi.y), 0.0f), gz = fmaxf(fmaxf(lo.z - z, z - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}
// ... and over the queries of box q as well: lo - x >= lo - q.hi and x - hi >= q.lo - hi for every x in q, and rounding is monotone
__device__ __forceinline__ float knn_box_box_bound(float4 qlo, float4 qhi, float4 lo, float4 hi) {
#pragma clang fp contract(off)
    const float gx = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.0f),
                gz = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__global__ __launch_bounds__(KB * KNN_SEARCH_WAVES) void k_knn_search(const float4 *__restrict__ sorted, const float4 *__restrict__ boxes,
                                                                      const float4 *__restrict__ groups, uint32_t n, uint32_t blocks,
                                                                      float *__restrict__ mean_sq,
                                                                      unsigned long long *__restrict__ evaluations) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qb = blockIdx.x * KNN_SEARCH_WAVES + (threadIdx.x >> 6);
    if (qb >= blocks) return; // (a whole wave)
    const uint32_t pos = qb * KB + lane;
    const float4 me = sorted[pos];
    const float x = me.x, y = me.y, z = me.z;
    const uint32_t idx = __float_as_uint(me.w);
    // a query that is not finite has no candidate (its row is +inf) and asks for no block; a slot past n is nobody
    const bool query = x == x;
    const uint32_t lanes_here = min(KB, n - qb * KB); // the wave's lanes that are points: all of them run every scan in lockstep
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    unsigned long long evals = 0;

    knn_scan_block<true>(sorted, qb, lanes_here, lane, x, y, z, b0, b1, b2);
    evals += (unsigned long long)lanes_here * lanes_here;
    float b2max = wave_max(query ? b2 : -INFINITY); // (no query in the wave: -inf, and every block is dropped)

    const float4 qlo = boxes[2 * (size_t)qb], qhi = boxes[2 * (size_t)qb + 1];
    // the candidates `mine` (one block per lane, `valid` where there is one) that the wave's bound does not drop, nearest lane first
    auto visit = [&](uint32_t mine, bool valid) {
        const float lbw = knn_box_box_bound(qlo, qhi, boxes[2 * (size_t)mine], boxes[2 * (size_t)mine + 1]);
        unsigned long long todo = __ballot(valid && !(lbw > b2max));
        while (todo) { // (at most 64 rounds: a bit is cleared in each)
            const uint32_t src = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)src);
            const float lb = knn_box_bound(x, y, z, boxes[2 * (size_t)c], boxes[2 * (size_t)c + 1]);
            if (__ballot(query && !(lb > b2)) == 0ull) continue;
            const uint32_t members = min(KB, n - c * KB);
            knn_scan_block<false>(sorted, c, members, lane, x, y, z, b0, b1, b2);
            evals += (unsigned long long)lanes_here * members;
            b2max = wave_max(query ? b2 : -INFINITY);
        }
    };
    // near: candidate t = 0, 1, 2, ...: the blocks qb - 1, qb + 1, qb - 2, qb + 2, ... up to KNN_NEAR on either side, so that b2 shrinks early
    const uint32_t reach = min(max(qb, blocks - 1u - qb), KNN_NEAR);
    for (uint32_t t0 = 0; t0 < 2u * reach; t0 += 64u) {
        const uint32_t t = t0 + lane, off = (t >> 1) + 1u;
        const bool up = t & 1u;
        const bool valid = off <= KNN_NEAR && (up ? off <= blocks - 1u - qb : off <= qb);
        visit(valid ? (up ? qb + off : qb - off) : qb, valid);
    }
    // far: every other block, by groups of KG: a group whose box the wave's bound drops costs one lane of one round
    const uint32_t n_groups = (blocks + KG - 1u) / KG;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += 64u) {
        const uint32_t g = g0 + lane;
        const bool gvalid = g < n_groups;
        const uint32_t gi = gvalid ? g : 0u;
        const float lbg = knn_box_box_bound(qlo, qhi, groups[2 * (size_t)gi], groups[2 * (size_t)gi + 1]);
        unsigned long long gtodo = __ballot(gvalid && !(lbg > b2max));
        while (gtodo) { // (at most 64 rounds)
            const uint32_t gs = g0 + (uint32_t)__builtin_ctzll(gtodo);
            gtodo &= gtodo - 1ull;
            const uint32_t c = gs * KG + lane;
            const uint32_t dist = c > qb ? c - qb : qb - c;
            const bool valid = c < blocks && dist > KNN_NEAR; // (the near blocks and the own one are done)
            visit(valid ? c : qb, valid);
        }
    }
    if (pos < n && idx < n) mean_sq[idx] = ((b0 + b1) + b2) / 3.0f;
    if (evaluations && lane == 0) atomicAdd(evaluations, evals);
}

} // namespace

extern "C" uint64_t splat_knn_workspace_bytes(uint32_t n) {
    const uint64_t blocks = knn_blocks(n);
    // the codes' high words, the sorted float4 plane (whole blocks), two float4 per block and per group of blocks, the cloud's box
    return (uint64_t)plane_bytes((uint64_t)n * 4) + plane_bytes(blocks * KB * 16) + plane_bytes(blocks * 32) + plane_bytes(div_up64(blocks, KG) * 32) + 256;
}

extern "C" int splat_knn_mean_sq(splat_ctx *ctx, splat_sorter *sorter, const void *points, uint32_t stride_floats, uint32_t n, void *workspace,
                                 uint64_t workspace_bytes, void *mean_sq, void *evaluations) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    if (n >= KNN_MAX_POINTS) return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_knn_mean_sq: n must be below 2^30");
    ARG_CHECK(ctx, stride_floats >= 3);
    ARG_CHECK(ctx, ((uintptr_t)evaluations & 7) == 0);
    if (n == 0) return SPLAT_OK;
    ARG_CHECK(ctx, sorter && sorter->ctx == ctx && points && mean_sq && workspace);
    ARG_CHECK(ctx, (((uintptr_t)points | (uintptr_t)mean_sq) & 3) == 0 && ((uintptr_t)workspace & 15) == 0);
    if (workspace_bytes < splat_knn_workspace_bytes(n))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_knn_mean_sq: the workspace is smaller than splat_knn_workspace_bytes(n)");
    if (n > sorter->capacity) return ctx_fail(ctx, SPLAT_ERR_CAPACITY, "splat_knn_mean_sq: n exceeds the sorter's capacity");
    const uint32_t blocks = knn_blocks(n);
    char *w = (char *)workspace;
    uint32_t *high = (uint32_t *)w;
    float4 *sorted = (float4 *)(w + plane_bytes((uint64_t)n * 4));
    float4 *boxes = (float4 *)((char *)sorted + plane_bytes((uint64_t)blocks * KB * 16));
    float4 *groups = (float4 *)((char *)boxes + plane_bytes((uint64_t)blocks * 32));
    uint32_t *box = (uint32_t *)((char *)groups + plane_bytes(div_up64(blocks, KG) * 32));
    const float *pts = (const float *)points;
    const dim3 block(KT), grid(div_up(n, KT));
    if (evaluations) HIP_TRY(ctx, hipMemsetAsync(evaluations, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(box, 0xff, 12, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(box + 3, 0, 12, ctx->stream));
    hipLaunchKernelGGL(k_knn_bbox, dim3(grid.x < 1024u ? grid.x : 1024u), block, 0, ctx->stream, pts, stride_floats, n, box);
    LAUNCH_CHECK(ctx, "k_knn_bbox");
    hipLaunchKernelGGL(k_knn_codes, grid, block, 0, ctx->stream, pts, stride_floats, n, box, sorter->keys, sorter->payload, high);
    LAUNCH_CHECK(ctx, "k_knn_codes");
    int rc = splat_sort_run(sorter, n, 0, 32);
    if (rc != SPLAT_OK) return rc;
    hipLaunchKernelGGL(k_knn_gather_high, grid, block, 0, ctx->stream, (const uint32_t *)splat_sort_sorted_payload(sorter), high, n, sorter->keys,
                       sorter->payload);
    LAUNCH_CHECK(ctx, "k_knn_gather_high");
    if ((rc = splat_sort_run(sorter, n, 0, 31)) != SPLAT_OK) return rc;
    hipLaunchKernelGGL(k_knn_blocks, dim3(div_up(blocks * KB, KT)), block, 0, ctx->stream, pts, stride_floats, n,
                       (const uint32_t *)splat_sort_sorted_payload(sorter), sorted, boxes);
    LAUNCH_CHECK(ctx, "k_knn_blocks");
    hipLaunchKernelGGL(k_knn_groups, dim3(div_up(div_up(blocks, KG) * KG, KT)), block, 0, ctx->stream, boxes, blocks, groups);
    LAUNCH_CHECK(ctx, "k_knn_groups");
    hipLaunchKernelGGL(k_knn_search, dim3(div_up(blocks, KNN_SEARCH_WAVES)), dim3(KB * KNN_SEARCH_WAVES), 0, ctx->stream, sorted, boxes, groups, n, blocks,
                       (float *)mean_sq, (unsigned long long *)evaluations);
    LAUNCH_CHECK(ctx, "k_knn_search");
    return SPLAT_OK;
}
