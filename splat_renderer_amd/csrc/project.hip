// project.hip — SplatProjector + DepthKeyExtractor + SplatPropertyManager update as CDNA4 kernels.
//
// Reference: /root/reference/src/SplatProjector.ts:64-132 (K1), src/shaders/extract-depth-keys.wgsl:37-63
// (K2), src/SplatPropertyManager.ts:82-107 (K12).
//
// Roofline: HBM.  Algorithmic bytes per splat: 16 (pos,radius) in + 32 (ProjectedSplat) + 4 (key)
// + 4 (payload) out = 56 B.  One lane per splat, 16-byte vector load, two 16-byte stores per lane
// that together fill a 32-byte record, 4-byte coalesced key/payload stores.
//
// This file is compiled with -ffp-contract=off: every float op below is one IEEE binary32 op in
// the order written, identical to oracle/oracle.c, so records and keys are bit-exact.
#include "common.h"
#include "variant.h"
#include "tile_range.h"
#include "block_scan.h"
#include "disc.h"
#include "ellipsoid.h"
#include "surfel.h"
#include "shade.h"

struct FrameUniforms {
    float m[16];   // VP, column-major
    float eye[3];
    float time;
    float w, h;
};

__device__ __forceinline__ void to_screen(const FrameUniforms &u, float x, float y, float z, float &sx, float &sy) {
    float cx = ((u.m[0] * x + u.m[4] * y) + u.m[8] * z) + u.m[12];
    float cy = ((u.m[1] * x + u.m[5] * y) + u.m[9] * z) + u.m[13];
    float cw = ((u.m[3] * x + u.m[7] * y) + u.m[11] * z) + u.m[15];
    float nx = cx / cw, ny = cy / cw;
    sx = ((nx + 1.0f) * 0.5f) * u.w;
    sy = ((1.0f - ny) * 0.5f) * u.h;
}

__device__ __forceinline__ uint32_t depth_key(float depth) {
    uint32_t bits = __float_as_uint(depth);
    uint32_t mask = ((bits >> 31) == 1u) ? 0xffffffffu : 0x80000000u; // extract-depth-keys.wgsl:57-58
    return bits ^ mask;
}

// The projector up to the point where the record is formed: screen centre, screen radius, depth.
__device__ __forceinline__ float4 project_centre(const FrameUniforms &u, float4 pr) {
    float x = pr.x, y = pr.y, z = pr.z, radius = pr.w;
    float dx = x - u.eye[0], dy = y - u.eye[1], dz = z - u.eye[2];
    float depth = sqrtf((dx * dx + dy * dy) + dz * dz); // SplatProjector.ts:77
    float scx, scy;
    to_screen(u, x, y, z, scx, scy);
    // max_k sqrt(d2_k) == sqrt(max_k d2_k) bit for bit: a correctly rounded square root is monotone, d2 >= +0,
    // and fmaxf drops a NaN operand either way — one square root per splat instead of six (the kernel is
    // VALU-bound: SQ counters show the vector ALUs 89 % busy, IEEE divides and square roots being most of it)
    float max_d2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) { // :93-113, same offset order as the shader
        float ox = (k == 0) ? radius : (k == 1) ? -radius : 0.0f;
        float oy = (k == 2) ? radius : (k == 3) ? -radius : 0.0f;
        float oz = (k == 4) ? radius : (k == 5) ? -radius : 0.0f;
        float sx, sy;
        to_screen(u, x + ox, y + oy, z + oz, sx, sy);
        float ex = scx - sx, ey = scy - sy;
        max_d2 = fmaxf(max_d2, ex * ex + ey * ey);
    }
    const float max_r = sqrtf(max_d2);
    return make_float4(scx, scy, max_r, depth);
}

// The oriented-disc projector's second input and output (disc.h): normals in, 32-byte disc records out.
struct DiscIO {
    const float4 *normals;
    uint32_t normal_stride;
    float4 *discs;
    uint32_t disc_stride; // float4s per record: 2, or 3 when the frame asks for LIT disc records (the splat's lit colour behind the record)
    EllIO ell;            // ELL (the anisotropic Gaussian, ellipsoid.h): its planes instead of the normals
};

// Band frames without an exchange (every rank projects all splats): most splats cannot reach the rank's
// tile rows, and the six offset projections that give the screen radius (12 IEEE divides) are what the projector
// costs.  This is a cheap, provably conservative test: with a_i = radius * VP[:, i] the screen displacement of the
// offset along axis i is W/2 * (a_x - ndc_x * a_w) / (c_w + a_w) (and likewise in y), so
//     |dx| <= W/2 * (max_i |a_x| + |ndc_x| * max_i |a_w|) / (c_w - max_i |a_w|)
// bounds the radius, hence the padded box; 0.1 % and one pixel of slack cover the rounding of the bound itself, and
// two pixels more on either side the rounding of the centre (below).  A splat it rejects has an empty clamped
// tile range in the exact path too (its record is not written: no list of the band can contain it); anything
// doubtful (w <= 0, NaN) goes through the exact path.
// BALL (the oriented disc): the offsets are not along the axes but anywhere in a ball of radius `r` (the disc p +
// r (t u + b v), |t| = 1, |b| = |n|, lies in the ball of radius r * max(1, |n|)), so the row NORMS of VP bound the
// clip-space displacement instead of the largest entry of each row.
template <bool BALL>
__device__ __forceinline__ bool cannot_reach_band(const FrameUniforms &u, float4 pr, float r, const BinParams &bp) {
    const float *m = u.m;
    const float cx = ((m[0] * pr.x + m[4] * pr.y) + m[8] * pr.z) + m[12];
    const float cy = ((m[1] * pr.x + m[5] * pr.y) + m[9] * pr.z) + m[13];
    const float cw = ((m[3] * pr.x + m[7] * pr.y) + m[11] * pr.z) + m[15];
    const float ax = r * (BALL ? 1.001f * __builtin_amdgcn_sqrtf((m[0] * m[0] + m[4] * m[4]) + m[8] * m[8])
                               : fmaxf(fmaxf(fabsf(m[0]), fabsf(m[4])), fabsf(m[8])));
    const float ay = r * (BALL ? 1.001f * __builtin_amdgcn_sqrtf((m[1] * m[1] + m[5] * m[5]) + m[9] * m[9])
                               : fmaxf(fmaxf(fabsf(m[1]), fabsf(m[5])), fabsf(m[9])));
    const float aw = r * (BALL ? 1.001f * __builtin_amdgcn_sqrtf((m[3] * m[3] + m[7] * m[7]) + m[11] * m[11])
                               : fmaxf(fmaxf(fabsf(m[3]), fabsf(m[7])), fabsf(m[11])));
    const float den = cw - aw;
    if (!(cw > 0.0f) || !(den > 0.0f)) return false;
    // (hardware reciprocal and square root, 1 ulp: the slack below is a thousand times that, and this test runs for
    // every splat of the scene on every rank)
    const float icw = __builtin_amdgcn_rcpf(cw), iden = __builtin_amdgcn_rcpf(den);
    const float ndx = cx * icw, ndy = cy * icw;
    const float bx = (0.5f * u.w) * (ax + fabsf(ndx) * aw) * iden, by = (0.5f * u.h) * (ay + fabsf(ndy) * aw) * iden;
    const float reach = __builtin_amdgcn_sqrtf(bx * bx + by * by) * (1.5f * 1.001f) + 1.0f; // >= the padded radius of SplatProjector.ts:119
    const float scy = ((1.0f - ndy) * 0.5f) * u.h;
    const float ts = (float)bp.tile;
    // The exact path bins the splat into the band iff max_y >= 16 row0 and min_y < 16 row1 (tile_range: floor, clamp): with reach
    // >= the padded radius + 1 px and this centre within 1e-3 px of the exact one, two more pixels on either side are slack
    // enough — a whole tile row (rounds 2-4) let 40 % more splats through to the exact projection than the band keeps.
    return (scy + reach < (float)bp.row0 * ts - 2.0f) || (scy - reach > (float)bp.row1 * ts + 2.0f); // (NaN: false)
}

// One splat: record, key, payload, packed tile range.  Returns the packed range (1 = empty).
// DISC: the footprint is SequentialRenderer's oriented disc — the ProjectedSplat's bounds are the disc's exact
// screen extent, screenRadius half the larger one, and the disc record goes to dio.discs.
// LIT (isotropic frames): the 32-byte composite record {centre, radius, depth | lit colour} goes to lio.records
// (shade.h) — everything the composite reads of a splat, in one line; the ProjectedSplat is then optional.
// Everything the projector reads of one splat.  Kernels that project several splats per thread load all of them
// before the first one's arithmetic (fourteen IEEE divides and two square roots deep) and stores: left to the
// compiler the loads stay behind the previous splat's stores — the output pointers may alias the inputs for all it
// knows — and every wave sits out two memory round trips per splat.
struct SplatIn {
    float4 pr, col, nrm, scl, rot;
};
// ELL (with DISC): the anisotropic Gaussian (ellipsoid.h) — scale and rotation instead of the normal, written as a disc record
template <bool DISC, bool LIT, bool ELL = false>
__device__ __forceinline__ SplatIn load_splat(const float4 *__restrict__ pos_radius, uint32_t stride_vec4, uint32_t i, const DiscIO &dio,
                                              const LitIO &lio) {
    SplatIn s;
    s.pr = pos_radius[(size_t)i * stride_vec4];
    s.col = s.nrm = s.scl = s.rot = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ELL) {
        s.scl = dio.ell.scales[(size_t)i * dio.ell.scale_stride];
        s.rot = dio.ell.rotations[(size_t)i * dio.ell.rot_stride];
    } else if (DISC) s.nrm = dio.normals[(size_t)i * dio.normal_stride];
    if (LIT) {
        s.col = lio.color[(size_t)i * lio.color_stride];
        if (!lio.prelit) s.nrm = lio.normals[(size_t)i * lio.normal_stride];
    }
    return s;
}

// WIDE (screens beyond 256 x 256 tiles): the range goes to range32 as an 8-byte pack_range_wide (range32 then points at
// uint2s); the return value is then not a range.
template <bool WITH_KEYS, bool WITH_RANGE, bool DISC, bool LIT = false, bool WIDE = false, bool ELL = false>
__device__ __forceinline__ uint32_t project_one(const FrameUniforms &u, const SplatIn &in, uint32_t i, uint32_t index_base,
                                                float4 *__restrict__ projected, uint32_t *__restrict__ keys,
                                                uint32_t *__restrict__ payload, uint32_t *__restrict__ range32, const BinParams &bp,
                                                const DiscIO &dio, const LitIO &lio = LitIO{}, uint32_t kslot = 0xffffffffu) {
    const uint32_t ks = kslot == 0xffffffffu ? i : kslot; // where the key and the packed range go (k_project_hist_bandc: a compacted slot)
    float4 a, b;
    float depth;
    if (DISC) {
        const float4 pr = in.pr;
        const DiscRecord d = ELL ? ellipsoid_record(u.m, u.w, u.h, pr, in.scl, in.rot) : disc_record(u.m, u.w, u.h, pr, in.nrm);
        dio.discs[(size_t)i * dio.disc_stride] = d.a;
        dio.discs[(size_t)i * dio.disc_stride + 1] = d.b;
        // LIT: the lit colour rides behind the record (48 bytes per splat): the disc frame's composite then gathers this one
        // record per staged list entry instead of record + colour + normal — the gathers are what a staged entry costs
        // (C2: 168 -> 124 us for one line less, profiles/r04_d_disc_composite_C2.txt)
        const float dx = pr.x - u.eye[0], dy = pr.y - u.eye[1], dz = pr.z - u.eye[2];
        depth = sqrtf((dx * dx + dy * dy) + dz * dz); // SplatProjector.ts:77: the sort key does not depend on the footprint
        // (the fourth word, the opacity the composite never reads, carries the depth instead: the auxiliary outputs' splat_aov)
        if (LIT) {
            const float4 lc = (ELL || lio.prelit) ? in.col : lit_color(in.col, in.nrm); // (an ellipsoid's colour is final: prelit)
            dio.discs[(size_t)i * dio.disc_stride + 2] = make_float4(lc.x, lc.y, lc.z, depth);
        }
        disc_bounds(d, a);
        b = make_float4(depth, 0.5f * fmaxf(a.z - a.x, a.w - a.y), __uint_as_float(index_base + i), 0.0f);
    } else {
        const float4 c = project_centre(u, in.pr);
        const float scx = c.x, scy = c.y, max_r = c.z;
        depth = c.w;
        float padded = max_r * 1.5f; // :119
        a = make_float4(scx - padded, scy - padded, scx + padded, scy + padded);
        b = make_float4(depth, max_r, __uint_as_float(index_base + i), 0.0f); // :128 originalIndex
        if (LIT) {
            lio.records[(size_t)i * 2] = c;
            lio.records[(size_t)i * 2 + 1] = lio.prelit ? in.col : lit_color(in.col, in.nrm);
        }
    }
    if ((!DISC && !LIT) || projected) { // (a disc or lit frame's composite reads its own records: the ProjectedSplat is optional there)
        projected[(size_t)i * 2] = a;
        projected[(size_t)i * 2 + 1] = b;
    }
    if (WITH_KEYS) {
        keys[ks] = depth_key(depth);
        if (payload) payload[ks] = index_base + i; // (frame path: the sort's first pass synthesises it)
    }
    uint32_t packed = 1u;
    if (WITH_RANGE) { // the binner's clamped tile range while the bounds are still in registers
        uint32_t tx0, tx1, ty0, ty1;
        const bool ok = tile_range(a, bp.width, bp.height, bp.tile, bp.ntx, bp.nty, bp.row0, bp.row1, tx0, tx1, ty0, ty1);
        if (WIDE) {
            reinterpret_cast<uint2 *>(range32)[ks] = pack_range_wide(ok, tx0, tx1, ty0, ty1);
        } else {
            packed = pack_range32(ok, tx0, tx1, ty0, ty1);
            range32[ks] = packed;
        }
    }
    return packed;
}

// Multi-GPU exchange records (no reference counterpart): 16 bytes per splat, float4 {screen
// centre x, y, screen radius, depth}.  The 32-byte ProjectedSplat is a pure function of it (bounds =
// centre -/+ radius * 1.5 in this file's operation order, originalIndex = position in the gathered
// array), so the ranks exchange half the bytes and rebuild records bit-exactly where they need them.
__global__ __launch_bounds__(256) void k_project_compact(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                         uint32_t n, float4 *__restrict__ records16) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) records16[i] = project_centre(u, pos_radius[(size_t)i * stride_vec4]);
}

// The same for the oriented-disc footprint: 48 bytes per splat {disc record, depth, 0, 0, 0} (the disc's bounds are a
// pure function of its record: disc_bounds).
__global__ __launch_bounds__(256) void k_project_disc48(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                        const float4 *__restrict__ normals, uint32_t normal_stride, uint32_t n,
                                                        float4 *__restrict__ records48) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 pr = pos_radius[(size_t)i * stride_vec4];
    const DiscRecord d = disc_record(u.m, u.w, u.h, pr, normals[(size_t)i * normal_stride]);
    const float dx = pr.x - u.eye[0], dy = pr.y - u.eye[1], dz = pr.z - u.eye[2];
    records48[(size_t)i * 3] = d.a;
    records48[(size_t)i * 3 + 1] = d.b;
    records48[(size_t)i * 3 + 2] = make_float4(sqrtf((dx * dx + dy * dy) + dz * dz), 0.0f, 0.0f, 0.0f); // SplatProjector.ts:77
}

__global__ __launch_bounds__(256) void k_expand_compact(const float4 *__restrict__ records16, uint32_t n, uint32_t index_base,
                                                        float4 *__restrict__ projected) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 c = records16[i];
    const float padded = c.z * 1.5f;
    projected[(size_t)i * 2] = make_float4(c.x - padded, c.y - padded, c.x + padded, c.y + padded);
    projected[(size_t)i * 2 + 1] = make_float4(c.w, c.z, __uint_as_float(index_base + i), 0.0f);
}

template <bool WITH_KEYS, bool WITH_RANGE, bool DISC, bool LIT = false, bool ELL = false>
__global__ __launch_bounds__(256) void k_project(FrameUniforms u, const float4 *__restrict__ pos_radius,
                                                 uint32_t stride_vec4, uint32_t n, uint32_t n_padded, uint32_t index_base,
                                                 float4 *__restrict__ projected, uint32_t *__restrict__ keys,
                                                 uint32_t *__restrict__ payload, uint32_t *__restrict__ range32, BinParams bp,
                                                 DiscIO dio, LitIO lio) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        if (WITH_KEYS && i < n_padded) { // extract-depth-keys.wgsl:46-50
            keys[i] = 0xffffffffu;
            if (payload) payload[i] = 0xffffffffu;
        }
        return;
    }
    const SplatIn in = load_splat<DISC, LIT, ELL>(pos_radius, stride_vec4, i, dio, lio);
    project_one<WITH_KEYS, WITH_RANGE, DISC, LIT, false, ELL>(u, in, i, index_base, projected, keys, payload, range32, bp, dio, lio);
}

// The frame's projector on screens beyond 256 x 256 tiles (sort-first only): k_project<true, true, DISC, LIT> with the
// 8-byte wide range per splat index instead of range32 (no payload: the sort's first pass synthesises it).
template <bool DISC, bool LIT, bool ELL = false>
__global__ __launch_bounds__(256) void k_project_wide(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                      uint32_t n, uint32_t n_padded, float4 *__restrict__ projected,
                                                      uint32_t *__restrict__ keys, uint2 *__restrict__ range_wide, BinParams bp,
                                                      DiscIO dio, LitIO lio) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        if (i < n_padded) keys[i] = 0xffffffffu;
        return;
    }
    const SplatIn in = load_splat<DISC, LIT, ELL>(pos_radius, stride_vec4, i, dio, lio);
    project_one<true, true, DISC, LIT, true, ELL>(u, in, i, 0, projected, keys, nullptr, reinterpret_cast<uint32_t *>(range_wide), bp, dio,
                                                  lio);
}

// Tile-first frame path: 1024 splats per workgroup (the binner's block), and while each splat's tile
// rectangle is in registers the block's pairs are counted per low tile-id digit — the histogram the
// first pass of the tile-id sort needs (tile_first.hip; k_band_prepare_tf in frame.hip does the same for
// the gathered records of a multi-GPU band).  The kernel is HBM-bound; the LDS counting hides under the stores.
template <bool DISC, bool LIT, uint32_t PER, uint32_t AHEAD = 1, bool ELL = false>
__global__ __launch_bounds__(256) void k_project_hist(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                      uint32_t n, uint32_t n_padded, float4 *__restrict__ projected,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ range32, BinParams bp,
                                                      TfHistOut ho, DiscIO dio, LitIO lio) {
    __shared__ uint32_t lh[4][256];
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, w = tid >> 6;
    const uint32_t blk = xcd_block_of(blockIdx.x, ho.xcd_per); // (blocks past the grid's last: nothing to project, no key to pad)
    if (blk * (PER * 256u) >= n_padded) return;
    SplatIn in[PER]; // (unrolled: a splat's registers are live from its load to its last use only)
#pragma unroll
    for (uint32_t k = 0; k < AHEAD; ++k) { // AHEAD splats' loads in flight before the first dependent instruction
        const uint32_t i = blk * (PER * 256u) + k * 256u + tid;
        if (i < n) in[k] = load_splat<DISC, LIT, ELL>(pos_radius, stride_vec4, i, dio, lio);
    }
    if (blk == 0 && tid == 0) *ho.overflow_flag = 0;
    for (uint32_t j = tid; j < 4 * 256; j += 256) (&lh[0][0])[j] = 0;
    __syncthreads();
    uint32_t local = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) { // (PER * 256 splats per workgroup: the binner's block)
        if (k + AHEAD < PER) { // ... and AHEAD of them in flight from then on
            const uint32_t i = blk * (PER * 256u) + (k + AHEAD) * 256u + tid;
            if (i < n) in[k + AHEAD] = load_splat<DISC, LIT, ELL>(pos_radius, stride_vec4, i, dio, lio);
        }
        const uint32_t i = blk * (PER * 256u) + k * 256u + tid;
        if (i >= n) {
            if (i < n_padded) keys[i] = 0xffffffffu;
            continue;
        }
        const uint32_t r = project_one<true, true, DISC, LIT, false, ELL>(u, in[k], i, 0, projected, keys, nullptr, range32, bp, dio, lio);
        const TileRect t = unpack_range32(r);
        if (t.empty()) continue;
        local += hist_add_rect(lh[w], t, bp.ntx, ho.mask);
    }
    local = wave_sum(local);
    if ((tid & 63) == 0) wsum[w] = local;
    __syncthreads();
    if (blk < ho.num_parts) { // (blocks that only pad keys past n have no histogram column)
        hist_flush<4>(lh, ho.hist, ho.num_parts, blk, ho.mask);
        if (tid == 0) ho.blocksums[blk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// The same kernel for a strict band of tile rows (bp.skip_outside): a cheap conservative test first, for all 1024
// splats of the block; the survivors — about 1/G of them, scattered at random over the lanes — are compacted through
// LDS so that the full projection runs on dense waves (left in place, every wave would still execute it for its few
// surviving lanes).  Same records, keys, ranges and histogram for every splat that can reach the band; the others get
// an all-ones key, an empty range and no record.
template <bool DISC, bool LIT>
__global__ __launch_bounds__(256) void k_project_hist_band(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                           uint32_t n, uint32_t n_padded, float4 *__restrict__ projected,
                                                           uint32_t *__restrict__ keys, uint32_t *__restrict__ range32, BinParams bp,
                                                           TfHistOut ho, DiscIO dio, LitIO lio) {
    __shared__ uint32_t lh[4][256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t s_list[1024];
    __shared__ uint32_t s_count;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    if (blockIdx.x == 0 && tid == 0) *ho.overflow_flag = 0;
    if (tid == 0) s_count = 0;
    for (uint32_t j = tid; j < 4 * 256; j += 256) (&lh[0][0])[j] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t i = blockIdx.x * 1024u + k * 256u + tid;
        bool keep = false;
        if (i < n) {
            const float4 pr = pos_radius[(size_t)i * stride_vec4];
            float r = fabsf(pr.w);
            if (DISC) {
                const float4 nr = dio.normals[(size_t)i * dio.normal_stride];
                r *= fmaxf(1.0f, 1.001f * __builtin_amdgcn_sqrtf((nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z));
            }
            keep = !cannot_reach_band<DISC>(u, pr, r, bp); // (NaN radius or normal: kept, the exact path decides)
            if (!keep) {
                keys[i] = 0xffffffffu; // (never read: a splat without pairs contributes no key; written so that the array is defined)
                range32[i] = 1u;       // pack_range32's empty range
            }
        } else if (i < n_padded) {
            keys[i] = 0xffffffffu;
        }
        const unsigned long long m = __ballot(keep);
        uint32_t base = 0;
        if (lane == 0 && m) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0);
        if (keep) s_list[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] = i;
    }
    __syncthreads();
    const uint32_t kept = s_count;
    uint32_t local = 0;
    for (uint32_t j = tid; j < kept; j += 256) {
        const uint32_t i = s_list[j];
        const SplatIn in = load_splat<DISC, LIT>(pos_radius, stride_vec4, i, dio, lio);
        const uint32_t r = project_one<true, true, DISC, LIT>(u, in, i, 0, projected, keys, nullptr, range32, bp, dio, lio);
        const TileRect t = unpack_range32(r);
        if (t.empty()) continue;
        local += hist_add_rect(lh[w], t, bp.ntx, ho.mask);
    }
    local = wave_sum(local);
    if (lane == 0) wsum[w] = local;
    __syncthreads();
    if (blockIdx.x < ho.num_parts) {
        hist_flush<4>(lh, ho.hist, ho.num_parts, blockIdx.x, ho.mask);
        if (tid == 0) ho.blocksums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// The strict band's projector for bands of a fraction of the screen (the exchange-free multi-GPU cut: every rank projects all
// splats for its own tile rows): groups of 4096 splats, the conservative test for all of them (every position load of a thread in
// flight at once), the survivors compacted through LDS, their full projection on DENSE lanes, and what the binner's first pass
// reads of them — packed tile range, depth key, splat index — left compacted at the front of the group's segment
// (ho.cidx / ho.kept_groups): k_tf_scatter<COMPACTED> then runs one workgroup per group over the survivors only, as it does after
// k_band_prepare_tfc for gathered records.  Same records, keys, ranges, histogram and lists as k_project_hist_band.
// (256 threads x 16 splats — every group of a 5 M-splat frame resident at once instead of two rounds — measured the same: 51 us at
// C2 on eight ranks.  20 us of that are the test of all splats, at the copy rate; the survivors' exact projection — ~550
// instructions a splat with its fourteen IEEE divides, behind a gather — is the rest: VALU 0.34 busy, waves waiting 0.55 of their
// cycles: profiles/r05_r_exchange_free_band_projector.txt)
constexpr uint32_t PBC_THREADS = 512, PBC_WAVES = PBC_THREADS / 64, PBC_PER = 8, PBC_GROUP = PBC_THREADS * PBC_PER;
static_assert(PBC_GROUP == 4096 && PBC_PER * PBC_WAVES == 64, "a group is 4096 splats = 64 (row, wave) cells of 64 splats");
template <bool DISC, bool LIT>
__global__ __launch_bounds__(PBC_THREADS) void k_project_hist_bandc(FrameUniforms u, const float4 *__restrict__ pos_radius, uint32_t stride_vec4,
                                                                    uint32_t n, float4 *__restrict__ projected, uint32_t *__restrict__ keys_c,
                                                                    uint32_t *__restrict__ range_c, BinParams bp, TfHistOut ho, DiscIO dio, LitIO lio) {
    __shared__ uint32_t lh[PBC_WAVES][256];
    __shared__ uint32_t rowcnt[64];
    __shared__ uint32_t wsum[PBC_WAVES];
    __shared__ uint32_t s_list[PBC_GROUP];
    __shared__ uint32_t s_kept;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t blk = xcd_block_of(blockIdx.x, ho.xcd_per);
    if (blk >= ho.num_parts) return;
    if (blk == 0 && tid == 0) *ho.overflow_flag = 0;
    for (uint32_t j = tid; j < PBC_WAVES * 256; j += PBC_THREADS) (&lh[0][0])[j] = 0;
    const uint32_t g0 = blk * PBC_GROUP;
    uint32_t okbits = 0;
#pragma unroll
    for (uint32_t k0 = 0; k0 < PBC_PER; k0 += 8) {
        float4 pr[8], nr[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t i = g0 + (k0 + k) * PBC_THREADS + tid;
            pr[k] = nr[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < n) {
                pr[k] = pos_radius[(size_t)i * stride_vec4];
                if (DISC) nr[k] = dio.normals[(size_t)i * dio.normal_stride];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t i = g0 + (k0 + k) * PBC_THREADS + tid;
            bool keep = false;
            if (i < n) {
                float r = fabsf(pr[k].w);
                if (DISC) r *= fmaxf(1.0f, 1.001f * __builtin_amdgcn_sqrtf((nr[k].x * nr[k].x + nr[k].y * nr[k].y) + nr[k].z * nr[k].z));
                keep = !cannot_reach_band<DISC>(u, pr[k], r, bp); // (NaN radius or normal: kept, the exact path decides)
            }
            const unsigned long long m = __ballot(keep);
            okbits |= keep ? (1u << (k0 + k)) : 0u;
            if (lane == 0) rowcnt[(k0 + k) * PBC_WAVES + w] = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    if (w == 0) { // the cells in (row, wave) order = ascending splat index
        const uint32_t mine = rowcnt[lane], incl = wave_inclusive_scan(mine);
        rowcnt[lane] = incl - mine;
        if (lane == 63) {
            ho.kept_groups[blk] = incl;
            s_kept = incl;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < PBC_PER; ++k) {
        const bool keep = (okbits >> k) & 1u;
        const unsigned long long m = __ballot(keep);
        if (keep) s_list[rowcnt[k * PBC_WAVES + w] + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] = g0 + k * PBC_THREADS + tid;
    }
    __syncthreads();
    const uint32_t kept = s_kept;
    uint32_t local = 0;
    for (uint32_t j = tid; j < kept; j += PBC_THREADS) {
        const uint32_t i = s_list[j];
        const SplatIn in = load_splat<DISC, LIT>(pos_radius, stride_vec4, i, dio, lio);
        // (the record goes to the splat's own index — the composite gathers it by that —, key and range to the compacted slot)
        const uint32_t r = project_one<true, true, DISC, LIT>(u, in, i, 0, projected, keys_c, nullptr, range_c, bp, dio, lio, g0 + j);
        ho.cidx[g0 + j] = i;
        const TileRect t = unpack_range32(r);
        if (t.empty()) continue; // (passed the conservative test, reaches no tile of the band: an empty range in the list)
        local += hist_add_rect(lh[w], t, bp.ntx, ho.mask);
    }
    local = wave_sum(local);
    if (lane == 0) wsum[w] = local;
    __syncthreads();
    hist_flush<PBC_WAVES>(lh, ho.hist, ho.num_parts, blk, ho.mask);
    if (tid == 0) {
        uint32_t ps = 0;
#pragma unroll
        for (uint32_t v = 0; v < PBC_WAVES; ++v) ps += wsum[v];
        ho.blocksums[blk] = ps;
    }
}

// The antialiased ellipsoid projector (splat_project_ellipsoid_aa): k_project<WITH_KEYS, false, true, false, true>'s outputs, from
// the same functions in the same order, and beside them the 2D Mip filter's factor rho (ellipsoid.h: <RHO>) and the colour
// plane with its opacity compensated, fl32(opacity * rho).  Every output is optional here (the whole antialiased frame asks for
// the colour plane alone); one thread per splat.
struct AaIO {
    float *rho;              // n floats, or NULL
    const float4 *color;     // (r, g, b, opacity), color_stride float4s apart; read only with color_out
    uint32_t color_stride;
    float4 *color_out;       // n x float4 (r, g, b, fl32(opacity * rho)), or NULL
};
__global__ __launch_bounds__(256) void k_project_ellipsoid_aa(FrameUniforms u, const float4 *__restrict__ pos, uint32_t stride_vec4, uint32_t n,
                                                              uint32_t n_padded, float4 *__restrict__ projected, float4 *__restrict__ records,
                                                              uint32_t *__restrict__ keys, uint32_t *__restrict__ payload, EllIO ell, AaIO aa) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        if (keys && i < n_padded) { // extract-depth-keys.wgsl:46-50
            keys[i] = 0xffffffffu;
            payload[i] = 0xffffffffu;
        }
        return;
    }
    const float4 pr = pos[(size_t)i * stride_vec4];
    const float4 scl = ell.scales[(size_t)i * ell.scale_stride], rot = ell.rotations[(size_t)i * ell.rot_stride];
    float4 col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (aa.color_out) col = aa.color[(size_t)i * aa.color_stride];
    float rho;
    const DiscRecord d = ellipsoid_record<true>(u.m, u.w, u.h, pr, scl, rot, &rho);
    if (records) {
        records[(size_t)i * 2] = d.a;
        records[(size_t)i * 2 + 1] = d.b;
    }
    if (projected || keys) { // project_one's DISC branch
        const float dx = pr.x - u.eye[0], dy = pr.y - u.eye[1], dz = pr.z - u.eye[2];
        const float depth = sqrtf((dx * dx + dy * dy) + dz * dz); // SplatProjector.ts:77
        if (projected) {
            float4 a;
            disc_bounds(d, a);
            projected[(size_t)i * 2] = a;
            projected[(size_t)i * 2 + 1] = make_float4(depth, 0.5f * fmaxf(a.z - a.x, a.w - a.y), __uint_as_float(i), 0.0f);
        }
        if (keys) {
            keys[i] = depth_key(depth);
            payload[i] = i;
        }
    }
    if (aa.rho) aa.rho[i] = rho;
    if (aa.color_out) aa.color_out[i] = make_float4(col.x, col.y, col.z, col.w * rho);
}

// The surfel projector (splat_project_surfel; surfel.h): project_one's DISC branch over surfel_record — the record, the
// ProjectedSplat (disc_bounds, depth |p - eye|, half the larger extent), key and payload — and beside them the centre's clip w
// (the z_i of the intersection-depth map; 0 for a culled surfel).  One thread per splat.
__global__ __launch_bounds__(256) void k_project_surfel(FrameUniforms u, const float4 *__restrict__ pos, uint32_t stride_vec4, uint32_t n,
                                                        uint32_t n_padded, float4 *__restrict__ projected, float4 *__restrict__ records,
                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ payload, EllIO ell,
                                                        float *__restrict__ clip_w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        if (keys && i < n_padded) { // extract-depth-keys.wgsl:46-50
            keys[i] = 0xffffffffu;
            payload[i] = 0xffffffffu;
        }
        return;
    }
    const float4 pr = pos[(size_t)i * stride_vec4];
    const float4 scl = ell.scales[(size_t)i * ell.scale_stride], rot = ell.rotations[(size_t)i * ell.rot_stride];
    float cw;
    const DiscRecord d = surfel_record(u.m, u.w, u.h, pr, scl, rot, &cw);
    records[(size_t)i * 2] = d.a;
    records[(size_t)i * 2 + 1] = d.b;
    const float dx = pr.x - u.eye[0], dy = pr.y - u.eye[1], dz = pr.z - u.eye[2];
    const float depth = sqrtf((dx * dx + dy * dy) + dz * dz); // SplatProjector.ts:77: surfels sort by centre distance, as 2DGS does
    float4 a;
    disc_bounds(d, a);
    projected[(size_t)i * 2] = a;
    projected[(size_t)i * 2 + 1] = make_float4(depth, 0.5f * fmaxf(a.z - a.x, a.w - a.y), __uint_as_float(i), 0.0f);
    if (keys) {
        keys[i] = depth_key(depth);
        payload[i] = i;
    }
    if (clip_w) clip_w[i] = cw;
}

// splat_sampling_rate_max: one thread per splat, no atomics.  c = VP [p; 1] and the screen centre exactly as to_screen();
// a splat in front of `near` and inside the screen widened by `margin` of its size on every side raises its rate to
// focal_px / c.w (Mip-Splatting's compute_3D_filter, one camera per call).  A NaN anywhere fails a comparison: unchanged.
__global__ __launch_bounds__(256) void k_sampling_rate_max(FrameUniforms u, float focal_px, float near, float margin, const float4 *__restrict__ pos,
                                                           uint32_t stride_vec4, uint32_t n, float *__restrict__ rate) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = pos[(size_t)i * stride_vec4];
    const float cw = ((u.m[3] * p.x + u.m[7] * p.y) + u.m[11] * p.z) + u.m[15]; // to_screen()'s own c.w
    float scx, scy;
    to_screen(u, p.x, p.y, p.z, scx, scy);
    const float lo_x = (-margin) * u.w, hi_x = (1.0f + margin) * u.w, lo_y = (-margin) * u.h, hi_y = (1.0f + margin) * u.h;
    if (cw > near && scx >= lo_x && scx <= hi_x && scy >= lo_y && scy <= hi_y) rate[i] = fmaxf(rate[i], focal_px / cw);
}

__global__ __launch_bounds__(256) void k_extract_keys(const float4 *__restrict__ projected, uint32_t n, uint32_t n_padded,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ payload) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_padded) return;
    if (i >= n) {
        keys[i] = 0xffffffffu;
        payload[i] = 0xffffffffu;
        return;
    }
    float depth = reinterpret_cast<const float *>(projected)[(size_t)i * 8 + 4];
    keys[i] = depth_key(depth);
    payload[i] = i;
}

__global__ __launch_bounds__(256) void k_update_props(const float4 *__restrict__ positions, const float4 *__restrict__ curvature,
                                                      uint32_t n, float4 *__restrict__ props) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 p = positions[i], c = curvature[i];
    props[(size_t)i * 2] = make_float4(p.x, p.y, p.z, 0.04f);                                                   // :94
    props[(size_t)i * 2 + 1] = make_float4(fabsf(c.x) * 0.8f + 0.2f, fabsf(c.y) * 0.8f + 0.2f, fabsf(c.z) * 0.8f + 0.2f, 1.0f); // :97-101
}

// the same update into two planes (the projector reads the first, the composite gathers from the second)
__global__ __launch_bounds__(256) void k_update_props_planes(const float4 *__restrict__ positions,
                                                             const float4 *__restrict__ curvature, uint32_t n,
                                                             float4 *__restrict__ pos_radius, float4 *__restrict__ color_opacity) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 p = positions[i], c = curvature[i];
    pos_radius[i] = make_float4(p.x, p.y, p.z, 0.04f);                                                                    // :94
    color_opacity[i] = make_float4(fabsf(c.x) * 0.8f + 0.2f, fabsf(c.y) * 0.8f + 0.2f, fabsf(c.z) * 0.8f + 0.2f, 1.0f); // :97-101
}

__global__ __launch_bounds__(256) void k_props_to_planes(const float4 *__restrict__ props, uint32_t n,
                                                         float4 *__restrict__ pos_radius, float4 *__restrict__ color_opacity) {
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    pos_radius[i] = props[(size_t)i * 2];
    color_opacity[i] = props[(size_t)i * 2 + 1];
}

static void load_uniforms(FrameUniforms &u, const float *uniforms) {
    for (int i = 0; i < 16; ++i) u.m[i] = uniforms[i];
    u.eye[0] = uniforms[16]; u.eye[1] = uniforms[17]; u.eye[2] = uniforms[18];
    u.time = uniforms[19]; u.w = uniforms[20]; u.h = uniforms[21];
}

int project_launch(splat_ctx *ctx, const ProjectArgs &a) {
    const uint32_t pr_stride_vec4 = a.pr_stride_vec4, n = a.n, index_base = a.index_base, n_padded = a.n_padded;
    const uint32_t normal_stride_vec4 = a.normal_stride_vec4;
    void *const projected = a.projected, *const keys = a.keys, *const payload = a.payload, *const discs = a.discs;
    uint32_t *const range32 = a.range32;
    uint2 *const range_wide = a.range_wide;
    const BinParams *const bp = a.bp;
    const TfHistOut *const hist_out = a.hist_out;
    const LitIO *const lit = a.lit;
    const EllIO *const ell = a.ell;
    FrameUniforms u;
    load_uniforms(u, a.uniforms);
    const uint32_t work = keys ? n_padded : n;
    if (work == 0) return SPLAT_OK;
    BinParams none = {0, 0, 1, 0, 0, 0, 0};
    const float4 *src = (const float4 *)a.pos_radius + (size_t)index_base * pr_stride_vec4;
    const bool disc = discs != nullptr; // the oriented-disc footprint (disc.h): normals in, disc records out
    // ... or the anisotropic Gaussian's (ellipsoid.h): scales and rotations in, disc records out (not on the band paths)
    const bool el = disc && ell != nullptr;
    if (el && hist_out && bp && bp->skip_outside)
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "project_launch: the ellipsoid footprint has no band projector");
    // lit composite records (shade.h) of an isotropic frame, written next to the keys and tile ranges; a disc frame's lit
    // colours go behind its disc records (lit->records = discs there: 48-byte records)
    const bool with_lit = lit && lit->records && !disc, disc_lit = lit && lit->records && disc;
    if ((with_lit || disc_lit) && !(keys && (range32 || range_wide) && !payload && index_base == 0))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "project_launch: lit records are written by the frame's projector only");
    DiscIO dio = {(disc && !el) ? (const float4 *)a.normals + (size_t)index_base * normal_stride_vec4 : nullptr, normal_stride_vec4,
                  (float4 *)discs, disc_lit ? 3u : 2u, EllIO{}};
    if (el) {
        dio.ell = *ell;
        dio.ell.scales += (size_t)index_base * ell->scale_stride;
        dio.ell.rotations += (size_t)index_base * ell->rot_stride;
    }
    const LitIO lio = (with_lit || disc_lit) ? *lit : LitIO{};
    stage_begin(ctx, SPLAT_STAGE_PROJECT);
    const dim3 block(256);
    const bool lit_out = with_lit || disc_lit;
    const bool frame_keys = keys && !payload && index_base == 0; // the frame's projector: keys in splat order, the payload implied
    // Every projector kernel takes the footprint as <DISC, ..., ELL> (the ellipsoid's records are disc records: no ELL without
    // DISC) and LIT: whether it writes lit colours as well.
    bool ok = false;
    if (hist_out && frame_keys && range32 && bp->skip_outside) {
        // a strict band (no ellipsoid: refused above), in 1024-splat blocks only: the caller keeps hist_out->block at TF_BLOCK_LARGE for it
        TfHistOut ho = *hist_out;
        if (hist_out->cidx) { // ... of a fraction of the screen: groups of 4096 splats, the survivors left compacted (num_parts = groups)
            const XcdGrid xg = xcd_grid(ho.num_parts);
            ho.xcd_per = xg.xcd_per;
            const dim3 grid(xg.grid);
            ok = variant_dispatch(
                [&](auto d, auto l) {
                    launch_kernel(ctx, NO_STAGE, k_project_hist_bandc<d.value, l.value>, grid, dim3(PBC_THREADS), u, src, pr_stride_vec4, n,
                                  (float4 *)projected, (uint32_t *)keys, range32, *bp, ho, dio, lio);
                    return true;
                },
                disc, lit_out);
        } else {
            ok = variant_dispatch(
                [&](auto d, auto l) {
                    launch_kernel(ctx, NO_STAGE, k_project_hist_band<d.value, l.value>, dim3(div_up(work, 1024)), block, u, src, pr_stride_vec4, n,
                                  n_padded, (float4 *)projected, (uint32_t *)keys, range32, *bp, ho, dio, lio);
                    return true;
                },
                disc, lit_out);
        }
    } else if (hist_out && frame_keys && range32) {
        TfHistOut ho = *hist_out;
        const bool small = hist_out->block == TF_BLOCK_SMALL;
        const uint32_t blocks = div_up(work, small ? 256u : 1024u);
        const XcdGrid xg = xcd_grid(blocks); // the blocks dealt as k_tf_scatter's are (common.h: xcd_block_of)
        ho.xcd_per = xg.xcd_per;
        const dim3 grid(xg.grid);
        ok = variant_dispatch(
            [&](auto d, auto l, auto per, auto e) {
                if constexpr (d.value || !e.value) {
                    launch_kernel(ctx, NO_STAGE, k_project_hist<d.value, l.value, per.value, 1, e.value>, grid, block, u, src, pr_stride_vec4, n,
                                  n_padded, (float4 *)projected, (uint32_t *)keys, range32, *bp, ho, dio, lio);
                    return true;
                } else return false;
            },
            disc, lit_out, OneOf<1, 4>{small ? 1 : 4}, el);
    } else if (frame_keys && range_wide) {
        ok = variant_dispatch(
            [&](auto d, auto l, auto e) {
                if constexpr (d.value || !e.value) {
                    launch_kernel(ctx, NO_STAGE, k_project_wide<d.value, l.value, e.value>, dim3(div_up(work, 256)), block, u, src, pr_stride_vec4, n,
                                  n_padded, (float4 *)projected, (uint32_t *)keys, range_wide, *bp, dio, lio);
                    return true;
                } else return false;
            },
            disc, lit_out, el);
    } else {
        // the staged projector: <WITH_KEYS, WITH_RANGE, ...>; tile ranges go with keys, lit colours with tile ranges
        const bool with_keys = keys != nullptr, with_range = keys && range32;
        ok = variant_dispatch(
            [&](auto k, auto r, auto d, auto l, auto e) {
                if constexpr ((k.value || !r.value) && (r.value || !l.value) && (d.value || !e.value)) {
                    launch_kernel(ctx, NO_STAGE, k_project<k.value, r.value, d.value, l.value, e.value>, dim3(div_up(work, 256)), block, u, src,
                                  pr_stride_vec4, n, with_keys ? n_padded : n, index_base, (float4 *)projected, (uint32_t *)keys,
                                  (uint32_t *)payload, with_range ? range32 : nullptr, with_range ? *bp : none, dio, lio);
                    return true;
                } else return false;
            },
            with_keys, with_range, disc, with_range && lit_out, el);
    }
    if (!ok) return ctx_fail(ctx, SPLAT_ERR_INVALID, "project_launch: no kernel for this footprint and these outputs");
    LAUNCH_CHECK(ctx, "k_project");
    stage_end(ctx, SPLAT_STAGE_PROJECT);
    return SPLAT_OK;
}

// The antialiased projector's launch, for splat_project_ellipsoid_aa and for the antialiased frame (frame.hip), which asks
// for the compensated colour plane only.  timed: the launch is a SPLAT_STAGE_PROJECT interval of its own (the staged entry point);
// the frame passes false, so that a timed antialiased frame still records one PROJECT interval, its projector's: the
// compensation pass runs before it and outside every stage.
int project_ellipsoid_aa_launch(splat_ctx *ctx, const ProjectAaArgs &a) {
    const uint32_t work = a.keys ? a.n_padded : a.n;
    if (work == 0) return SPLAT_OK;
    FrameUniforms u;
    load_uniforms(u, a.uniforms);
    const AaIO aa = {a.rho_out, (const float4 *)a.color_opacity, a.color_stride_vec4, (float4 *)a.color_opacity_out};
    if (a.timed) stage_begin(ctx, SPLAT_STAGE_PROJECT);
    hipLaunchKernelGGL(k_project_ellipsoid_aa, dim3(div_up(work, 256)), dim3(256), 0, ctx->stream, u, (const float4 *)a.positions, a.pos_stride_vec4,
                       a.n, work, (float4 *)a.projected, (float4 *)a.records, (uint32_t *)a.keys, (uint32_t *)a.payload, *a.ell, aa);
    LAUNCH_CHECK(ctx, "k_project_ellipsoid_aa");
    if (a.timed) stage_end(ctx, SPLAT_STAGE_PROJECT);
    return SPLAT_OK;
}

extern "C" {

int splat_project(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4, uint32_t n,
                  void *projected, void *keys, void *payload, uint32_t n_padded) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (pos_radius && projected)));
    ARG_CHECK(ctx, pr_stride_vec4 >= 1);
    ARG_CHECK(ctx, (keys == nullptr) == (payload == nullptr));
    ARG_CHECK(ctx, keys == nullptr || n_padded >= n);
    ARG_CHECK(ctx, (((uintptr_t)pos_radius | (uintptr_t)projected) & 15) == 0);
    ProjectArgs a;
    a.uniforms = uniforms, a.pos_radius = pos_radius, a.pr_stride_vec4 = pr_stride_vec4, a.n = n;
    a.projected = projected, a.keys = keys, a.payload = payload, a.n_padded = n_padded;
    return project_launch(ctx, a);
}

int splat_project_disc(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4, const void *normals,
                       uint32_t normal_stride_vec4, uint32_t n, void *projected, void *discs, void *keys, void *payload,
                       uint32_t n_padded) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (pos_radius && normals && projected && discs)));
    ARG_CHECK(ctx, pr_stride_vec4 >= 1 && normal_stride_vec4 >= 1);
    ARG_CHECK(ctx, (keys == nullptr) == (payload == nullptr));
    ARG_CHECK(ctx, keys == nullptr || n_padded >= n);
    ARG_CHECK(ctx, (((uintptr_t)pos_radius | (uintptr_t)normals | (uintptr_t)projected | (uintptr_t)discs) & 15) == 0);
    // (n == 0 with keys only pads them, which either footprint's kernel does)
    ProjectArgs a;
    a.uniforms = uniforms, a.pos_radius = pos_radius, a.pr_stride_vec4 = pr_stride_vec4, a.n = n;
    a.projected = projected, a.keys = keys, a.payload = payload, a.n_padded = n_padded;
    a.normals = normals, a.normal_stride_vec4 = normal_stride_vec4, a.discs = n ? discs : nullptr;
    return project_launch(ctx, a);
}

int splat_project_ellipsoid(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4, const void *scales,
                            uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4, uint32_t n, void *projected,
                            void *records, void *keys, void *payload, uint32_t n_padded) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (positions && scales && rotations && projected && records)));
    ARG_CHECK(ctx, pos_stride_vec4 >= 1 && scale_stride_vec4 >= 1 && rot_stride_vec4 >= 1);
    ARG_CHECK(ctx, (keys == nullptr) == (payload == nullptr));
    ARG_CHECK(ctx, keys == nullptr || n_padded >= n);
    ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)scales | (uintptr_t)rotations | (uintptr_t)projected | (uintptr_t)records) & 15) == 0);
    const EllIO ell = {(const float4 *)scales, scale_stride_vec4, (const float4 *)rotations, rot_stride_vec4};
    ProjectArgs a;
    a.uniforms = uniforms, a.pos_radius = positions, a.pr_stride_vec4 = pos_stride_vec4, a.n = n;
    a.projected = projected, a.keys = keys, a.payload = payload, a.n_padded = n_padded;
    a.discs = n ? records : nullptr, a.ell = &ell;
    return project_launch(ctx, a);
}

int splat_project_ellipsoid_aa(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4, const void *scales,
                               uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4, uint32_t n, void *projected,
                               void *records, void *keys, void *payload, uint32_t n_padded, void *rho_out, const void *color_opacity,
                               uint32_t color_stride_vec4, void *color_opacity_out) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (positions && scales && rotations && projected && records)));
    ARG_CHECK(ctx, pos_stride_vec4 >= 1 && scale_stride_vec4 >= 1 && rot_stride_vec4 >= 1);
    ARG_CHECK(ctx, (keys == nullptr) == (payload == nullptr));
    ARG_CHECK(ctx, keys == nullptr || n_padded >= n);
    ARG_CHECK(ctx, color_opacity_out == nullptr || (color_opacity && color_stride_vec4 >= 1));
    ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)scales | (uintptr_t)rotations | (uintptr_t)projected | (uintptr_t)records |
                     (uintptr_t)color_opacity | (uintptr_t)color_opacity_out) & 15) == 0 && ((uintptr_t)rho_out & 3) == 0);
    const EllIO ell = {(const float4 *)scales, scale_stride_vec4, (const float4 *)rotations, rot_stride_vec4};
    ProjectAaArgs a;
    a.uniforms = uniforms, a.positions = positions, a.pos_stride_vec4 = pos_stride_vec4, a.ell = &ell, a.n = n;
    a.projected = projected, a.records = records, a.keys = keys, a.payload = payload, a.n_padded = n_padded;
    a.rho_out = (float *)rho_out, a.color_opacity = color_opacity, a.color_stride_vec4 = color_stride_vec4;
    a.color_opacity_out = color_opacity_out, a.timed = true;
    return project_ellipsoid_aa_launch(ctx, a);
}

int splat_project_surfel(splat_ctx *ctx, const float *uniforms, const void *positions, uint32_t pos_stride_vec4, const void *scales,
                         uint32_t scale_stride_vec4, const void *rotations, uint32_t rot_stride_vec4, uint32_t n, void *projected, void *records,
                         void *keys, void *payload, uint32_t n_padded, void *clip_w_out) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (positions && scales && rotations && projected && records)));
    ARG_CHECK(ctx, pos_stride_vec4 >= 1 && scale_stride_vec4 >= 1 && rot_stride_vec4 >= 1);
    ARG_CHECK(ctx, (keys == nullptr) == (payload == nullptr));
    ARG_CHECK(ctx, keys == nullptr || n_padded >= n);
    ARG_CHECK(ctx, (((uintptr_t)positions | (uintptr_t)scales | (uintptr_t)rotations | (uintptr_t)projected | (uintptr_t)records) & 15) == 0 &&
                       ((uintptr_t)clip_w_out & 3) == 0);
    const uint32_t work = keys ? n_padded : n; // (n == 0 with keys only pads them)
    if (work == 0) return SPLAT_OK;
    FrameUniforms u;
    load_uniforms(u, uniforms);
    const EllIO ell = {(const float4 *)scales, scale_stride_vec4, (const float4 *)rotations, rot_stride_vec4};
    stage_begin(ctx, SPLAT_STAGE_PROJECT);
    hipLaunchKernelGGL(k_project_surfel, dim3(div_up(work, 256)), dim3(256), 0, ctx->stream, u, (const float4 *)positions, pos_stride_vec4, n, work,
                       (float4 *)projected, (float4 *)records, (uint32_t *)keys, (uint32_t *)payload, ell, (float *)clip_w_out);
    LAUNCH_CHECK(ctx, "k_project_surfel");
    stage_end(ctx, SPLAT_STAGE_PROJECT);
    return SPLAT_OK;
}

int splat_sampling_rate_max(splat_ctx *ctx, const float *uniforms, float focal_px, float near, float margin, const void *positions,
                            uint32_t pos_stride_vec4, uint32_t n, void *rate_inout) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (n == 0 || (positions && rate_inout)) && pos_stride_vec4 >= 1);
    ARG_CHECK(ctx, ((uintptr_t)positions & 15) == 0 && ((uintptr_t)rate_inout & 3) == 0);
    if (n == 0) return SPLAT_OK;
    FrameUniforms u;
    load_uniforms(u, uniforms);
    hipLaunchKernelGGL(k_sampling_rate_max, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, u, focal_px, near, margin, (const float4 *)positions,
                       pos_stride_vec4, n, (float *)rate_inout);
    LAUNCH_CHECK(ctx, "k_sampling_rate_max");
    return SPLAT_OK;
}

int splat_project_slice(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4, uint32_t first,
                        uint32_t count, void *projected_slice) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (count == 0 || (pos_radius && projected_slice)) && pr_stride_vec4 >= 1);
    ARG_CHECK(ctx, (((uintptr_t)pos_radius | (uintptr_t)projected_slice) & 15) == 0);
    ProjectArgs a;
    a.uniforms = uniforms, a.pos_radius = pos_radius, a.pr_stride_vec4 = pr_stride_vec4, a.n = count, a.index_base = first;
    a.projected = projected_slice;
    return project_launch(ctx, a);
}


int splat_project_slice_compact(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4,
                                uint32_t first, uint32_t count, void *records16_slice) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (count == 0 || (pos_radius && records16_slice)) && pr_stride_vec4 >= 1);
    ARG_CHECK(ctx, (((uintptr_t)pos_radius | (uintptr_t)records16_slice) & 15) == 0);
    if (count == 0) return SPLAT_OK;
    FrameUniforms u;
    load_uniforms(u, uniforms);
    stage_begin(ctx, SPLAT_STAGE_PROJECT);
    hipLaunchKernelGGL(k_project_compact, dim3(div_up(count, 256)), dim3(256), 0, ctx->stream, u,
                       (const float4 *)pos_radius + (size_t)first * pr_stride_vec4, pr_stride_vec4, count, (float4 *)records16_slice);
    LAUNCH_CHECK(ctx, "k_project_compact");
    stage_end(ctx, SPLAT_STAGE_PROJECT);
    return SPLAT_OK;
}

int splat_project_slice_disc(splat_ctx *ctx, const float *uniforms, const void *pos_radius, uint32_t pr_stride_vec4, const void *normals,
                             uint32_t normal_stride_vec4, uint32_t first, uint32_t count, void *records48_slice) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, uniforms && (count == 0 || (pos_radius && normals && records48_slice)) && pr_stride_vec4 >= 1 && normal_stride_vec4 >= 1);
    ARG_CHECK(ctx, (((uintptr_t)pos_radius | (uintptr_t)normals | (uintptr_t)records48_slice) & 15) == 0);
    if (count == 0) return SPLAT_OK;
    FrameUniforms u;
    load_uniforms(u, uniforms);
    stage_begin(ctx, SPLAT_STAGE_PROJECT);
    hipLaunchKernelGGL(k_project_disc48, dim3(div_up(count, 256)), dim3(256), 0, ctx->stream, u,
                       (const float4 *)pos_radius + (size_t)first * pr_stride_vec4, pr_stride_vec4,
                       (const float4 *)normals + (size_t)first * normal_stride_vec4, normal_stride_vec4, count, (float4 *)records48_slice);
    LAUNCH_CHECK(ctx, "k_project_disc48");
    stage_end(ctx, SPLAT_STAGE_PROJECT);
    return SPLAT_OK;
}

int splat_expand_compact(splat_ctx *ctx, const void *records16, uint32_t n, uint32_t index_base, void *projected) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, n == 0 || (records16 && projected));
    ARG_CHECK(ctx, (((uintptr_t)records16 | (uintptr_t)projected) & 15) == 0);
    if (n == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_expand_compact, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const float4 *)records16, n, index_base,
                       (float4 *)projected);
    LAUNCH_CHECK(ctx, "k_expand_compact");
    return SPLAT_OK;
}

int splat_extract_keys(splat_ctx *ctx, const void *projected, uint32_t n, uint32_t n_padded, void *keys, void *payload) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, keys && payload && (n == 0 || projected) && n_padded >= n);
    if (n_padded == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_extract_keys, dim3(div_up(n_padded, 256)), dim3(256), 0, ctx->stream, (const float4 *)projected, n,
                       n_padded, (uint32_t *)keys, (uint32_t *)payload);
    LAUNCH_CHECK(ctx, "k_extract_keys");
    return SPLAT_OK;
}

int splat_update_props(splat_ctx *ctx, const void *positions, const void *curvature, uint32_t n, void *props) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, n == 0 || (positions && curvature && props));
    if (n == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_update_props, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const float4 *)positions,
                       (const float4 *)curvature, n, (float4 *)props);
    LAUNCH_CHECK(ctx, "k_update_props");
    return SPLAT_OK;
}

int splat_update_props_planes(splat_ctx *ctx, const void *positions, const void *curvature, uint32_t n, void *pos_radius,
                              void *color_opacity) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, n == 0 || (positions && curvature && pos_radius && color_opacity));
    if (n == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_update_props_planes, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const float4 *)positions,
                       (const float4 *)curvature, n, (float4 *)pos_radius, (float4 *)color_opacity);
    LAUNCH_CHECK(ctx, "k_update_props_planes");
    return SPLAT_OK;
}

int splat_props_to_planes(splat_ctx *ctx, const void *props, uint32_t n, void *pos_radius, void *color_opacity) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, n == 0 || (props && pos_radius && color_opacity));
    ARG_CHECK(ctx, (((uintptr_t)props | (uintptr_t)pos_radius | (uintptr_t)color_opacity) & 15) == 0);
    if (n == 0) return SPLAT_OK;
    hipLaunchKernelGGL(k_props_to_planes, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, (const float4 *)props, n, (float4 *)pos_radius,
                       (float4 *)color_opacity);
    LAUNCH_CHECK(ctx, "k_props_to_planes");
    return SPLAT_OK;
}

} // extern "C"
