// mcmc.hip — 3DGS-MCMC for a fit (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", 2024; an extension, no
// reference counterpart): dead splats teleported onto live ones drawn in proportion to opacity, growth to an exact budget, and
// the per-step noise on the means (include/splat.h, "MCMC relocation", states the rules; tests/mcmc_ref.py restates them).
//
// splat_mcmc_sample   k_mcmc_weights (binary64 sigmoid -> 24-bit integer weight, dead flag) -> the dead flags' exclusive scan
//                     (scan.hip's kernels) and the weights' INCLUSIVE scan in uint64 (k_scan64_reduce, one k_scan64_sums
//                     workgroup over the block sums, k_scan64_apply: wave64 shuffles of the two halves, LDS for the four wave
//                     totals) -> k_mcmc_draw: one Philox draw per thread, a binary search over the scan, counts by unsigned
//                     integer atomic adds (their result does not depend on the order: the same inputs give the same bits).
// splat_mcmc_apply    k_mcmc_rows (one thread per float of a moved row: copies, zeroed moments), k_mcmc_values (one thread per
//                     draw: the corrected opacity and scales in binary64), k_mcmc_sources (one thread per splat: a drawn
//                     source's own correction and zeroed moments), in that order on the stream.
// splat_mcmc_noise    k_mcmc_noise<VEC>: one pass, 44 B read and 12 B written per splat; VEC: four splats per thread, every plane
//                     in float4s (3 + 3 + 4 + 1 loads, 3 stores; the up to three splats past the last four take the scalar form in
//                     the same launch).  Both forms call noise_one(): the same bits.
// No floating-point atomics anywhere.
#include "common.h"
#include "philox.h"

namespace {

constexpr uint32_t MT = 256;               // threads per workgroup, every kernel here
constexpr uint32_t S64_UNIT = MT * 4;      // one uint4 of weights per thread
constexpr uint32_t S64_TILE = S64_UNIT * 2; // weights per workgroup of the 64-bit scan
constexpr uint32_t MCMC_MAX_SPLATS = 1u << 30;
constexpr uint32_t MCMC_NMAX = 51;          // the relocation's ratio is capped at N = 51 (the table below)

struct McmcWords { // the device words the host reads back
    uint64_t total; // T: the sum of the weights
    uint32_t dead, pad;
};

// ---- the 64-bit scan ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// exclusive scan of one value per thread over the workgroup; wave_sums: 4 uint64 of LDS
__device__ __forceinline__ uint64_t block_exclusive_scan_u64(uint64_t v, uint64_t *wave_sums, uint64_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = shfl_up_u64(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wave_sums[w] = incl;
    __syncthreads();
    const uint64_t s0 = wave_sums[0], s1 = wave_sums[1], s2 = wave_sums[2], s3 = wave_sums[3];
    __syncthreads(); // (the next unit rewrites wave_sums)
    total = s0 + s1 + s2 + s3;
    return (w > 0 ? s0 : 0ull) + (w > 1 ? s1 : 0ull) + (w > 2 ? s2 : 0ull) + incl - v;
}

__device__ __forceinline__ uint4 load_weights(const uint32_t *in, uint32_t base, uint32_t n) {
    const uint32_t i = base + threadIdx.x * 4;
    if (i + 4 <= n) return *reinterpret_cast<const uint4 *>(in + i);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < n) v.x = in[i];
    if (i + 1 < n) v.y = in[i + 1];
    if (i + 2 < n) v.z = in[i + 2];
    return v;
}

__global__ __launch_bounds__(MT) void k_scan64_reduce(const uint32_t *__restrict__ w, uint32_t n, uint64_t *__restrict__ sums) {
    __shared__ uint64_t wave_sums[4];
    const uint32_t elem0 = blockIdx.x * S64_TILE;
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < S64_TILE / S64_UNIT; ++k) {
        const uint32_t base = elem0 + k * S64_UNIT;
        if (base < n) {
            const uint4 v = load_weights(w, base, n);
            acc += ((uint64_t)v.x + v.y) + ((uint64_t)v.z + v.w);
        }
    }
    uint64_t total;
    block_exclusive_scan_u64(acc, wave_sums, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the block sums -> their exclusive prefixes, in place; words->total = T
__global__ __launch_bounds__(MT) void k_scan64_sums(uint64_t *__restrict__ sums, uint32_t blocks, McmcWords *__restrict__ words) {
    __shared__ uint64_t wave_sums[4];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < blocks; base += MT) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < blocks ? sums[i] : 0ull;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan_u64(v, wave_sums, total) + carry;
        if (i < blocks) sums[i] = ex;
        carry += total;
    }
    if (threadIdx.x == 0) words->total = carry;
}

__global__ __launch_bounds__(MT) void k_scan64_apply(const uint32_t *__restrict__ w, uint32_t n, const uint64_t *__restrict__ sums,
                                                     uint64_t *__restrict__ incl) {
    __shared__ uint64_t wave_sums[4];
    const uint32_t elem0 = blockIdx.x * S64_TILE;
    uint64_t carry = sums[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < S64_TILE / S64_UNIT; ++k) {
        const uint32_t base = elem0 + k * S64_UNIT;
        if (base >= n) break; // (uniform over the workgroup)
        const uint4 v = load_weights(w, base, n);
        uint64_t total;
        const uint64_t ex = block_exclusive_scan_u64(((uint64_t)v.x + v.y) + ((uint64_t)v.z + v.w), wave_sums, total) + carry;
        const uint64_t c0 = ex + v.x, c1 = c0 + v.y, c2 = c1 + v.z, c3 = c2 + v.w;
        const uint32_t i = base + threadIdx.x * 4;
        if (i + 4 <= n) {
            reinterpret_cast<ulonglong2 *>(incl + i)[0] = make_ulonglong2(c0, c1);
            reinterpret_cast<ulonglong2 *>(incl + i)[1] = make_ulonglong2(c2, c3);
        } else {
            if (i < n) incl[i] = c0;
            if (i + 1 < n) incl[i + 1] = c1;
            if (i + 2 < n) incl[i + 2] = c2;
        }
        carry += total;
    }
}

// ---- sample -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MT) void k_mcmc_weights(const float *__restrict__ logits, uint32_t n, uint32_t q_min, uint32_t *__restrict__ weight,
                                                     uint32_t *__restrict__ dead) {
    const uint32_t i = blockIdx.x * MT + threadIdx.x;
    if (i >= n) return;
    const float l = logits[i];
    const double o = 1.0 / (1.0 + exp(-(double)l));
    const uint32_t q = l != l ? 0u : (uint32_t)floor(o * 16777216.0);
    const bool d = q < q_min;
    weight[i] = d ? 0u : q;
    dead[i] = d ? 1u : 0u;
}

// relocate (one thread per splat): dead splat i is target dead_rank[i]; thread j < the number of dead makes draw j.
// add (one thread per draw): target n + j.
__global__ __launch_bounds__(MT) void k_mcmc_draw(uint32_t mode, uint32_t n, uint32_t n_draws, const McmcWords *__restrict__ words,
                                                  const uint64_t *__restrict__ incl, const uint32_t *__restrict__ dead,
                                                  const uint32_t *__restrict__ dead_rank, uint2 key, uint32_t *__restrict__ targets,
                                                  uint32_t *__restrict__ sources, uint32_t *__restrict__ counts) {
    const uint32_t j = blockIdx.x * MT + threadIdx.x;
    const uint64_t total = words->total;
    if (total == 0ull) return; // nobody alive: nothing is drawn
    uint32_t draws = n_draws;
    if (mode == SPLAT_MCMC_RELOCATE) {
        draws = words->dead;
        if (j < n && dead[j]) targets[dead_rank[j]] = j;
    } else if (j < n_draws) {
        targets[j] = n + j;
    }
    if (j >= draws) return;
    const uint4 x = philox4x32_10(make_uint4(j, 0u, mode, 0u), key);
    const uint64_t r = (uint64_t)x.x | ((uint64_t)x.y << 32);
    const uint64_t t = __umul64hi(r, total); // floor(r T / 2^64) < T
    uint32_t lo = 0, hi = n - 1;             // the smallest i with incl[i] > t (incl[n - 1] = T > t)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (incl[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    sources[j] = lo;
    atomicAdd(&counts[lo], 1u);
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------

// binom[a][k] = C(a, k), a, k <= 50: Pascal's triangle in double on the host (every entry is below 2^53: exact)
struct BinomTable {
    double b[MCMC_NMAX][MCMC_NMAX];
    constexpr BinomTable() : b() {
        for (uint32_t a = 0; a < MCMC_NMAX; ++a) {
            b[a][0] = 1.0;
            for (uint32_t k = 1; k <= a; ++k) b[a][k] = b[a - 1][k - 1] + (k < a ? b[a - 1][k] : 0.0);
        }
    }
};
__device__ const BinomTable BINOM = BinomTable();

// The correction of a source drawn c times, from its old logit, in binary64: the new logit (rounded once) and log(o / D), what
// every log-scale gains.
__device__ void mcmc_relocated(float logit, uint32_t c, double min_opacity, float &new_logit, double &log_ratio) {
    const double o = 1.0 / (1.0 + exp(-(double)logit));
    const uint32_t N = c + 1u < MCMC_NMAX ? c + 1u : MCMC_NMAX;
    const double on = 1.0 - pow(1.0 - o, 1.0 / (double)N);
    double term[MCMC_NMAX]; // (-1)^k o'^(k + 1) / sqrt(k + 1)
    double p = on;
    for (uint32_t k = 0; k < N; ++k) {
        term[k] = ((k & 1u) ? -p : p) / sqrt((double)(k + 1u));
        p *= on;
    }
    double D = 0.0;
    for (uint32_t a = 1; a <= N; ++a) {
        double s = 0.0;
        for (uint32_t k = 0; k < a; ++k) s += BINOM.b[a - 1][k] * term[k];
        D += s;
    }
    const double hi = 1.0 - 0x1p-23;
    const double oc = on < min_opacity ? min_opacity : on > hi ? hi : on;
    new_logit = (float)(log(oc) - log(1.0 - oc));
    log_ratio = log(o / D);
}

struct McmcPlanes {
    float *p[5], *m[5], *v[5];
    uint32_t width[5], first[6]; // floats per row of each plane; first[k] = the floats of the planes before k
};

// one thread per float of a moved row: means, rotations and sh copied bit for bit; every moment of the target row zeroed
__global__ __launch_bounds__(MT) void k_mcmc_rows(McmcPlanes pl, const uint32_t *__restrict__ targets, const uint32_t *__restrict__ sources,
                                                  uint32_t total, uint32_t n, uint32_t rows) {
    const uint32_t e = blockIdx.x * MT + threadIdx.x;
    if (e >= total) return;
    const uint32_t per = pl.first[5], j = e / per, c = e - j * per;
    const uint32_t t = targets[j], s = sources[j];
    if (t >= rows || s >= n) return; // (not a sample's output: nothing is written out of bounds)
    uint32_t k = 0;
    while (c >= pl.first[k + 1]) ++k;
    const uint32_t w = pl.width[k], col = c - pl.first[k];
    const size_t dst = (size_t)t * w + col;
    if (k == 0 || k == 2 || k == 4) pl.p[k][dst] = pl.p[k][(size_t)s * w + col];
    if (pl.m[k]) pl.m[k][dst] = 0.0f;
    if (pl.v[k]) pl.v[k][dst] = 0.0f;
}

__global__ __launch_bounds__(MT) void k_mcmc_values(McmcPlanes pl, const uint32_t *__restrict__ targets, const uint32_t *__restrict__ sources,
                                                    const uint32_t *__restrict__ counts, uint32_t n_draws, uint32_t n, uint32_t rows,
                                                    double min_opacity) {
    const uint32_t j = blockIdx.x * MT + threadIdx.x;
    if (j >= n_draws) return;
    const uint32_t t = targets[j], s = sources[j];
    if (t >= rows || s >= n) return;
    float nl;
    double lr;
    mcmc_relocated(pl.p[3][s], counts[s], min_opacity, nl, lr);
    pl.p[3][t] = nl;
#pragma unroll
    for (int a = 0; a < 3; ++a) pl.p[1][3 * (size_t)t + a] = (float)((double)pl.p[1][3 * (size_t)s + a] + lr);
}

__global__ __launch_bounds__(MT) void k_mcmc_sources(McmcPlanes pl, const uint32_t *__restrict__ counts, uint32_t n, double min_opacity) {
    const uint32_t i = blockIdx.x * MT + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = counts[i];
    if (c == 0u) return;
    float nl;
    double lr;
    mcmc_relocated(pl.p[3][i], c, min_opacity, nl, lr);
    pl.p[3][i] = nl;
#pragma unroll
    for (int a = 0; a < 3; ++a) pl.p[1][3 * (size_t)i + a] = (float)((double)pl.p[1][3 * (size_t)i + a] + lr);
    for (int k = 0; k < 5; ++k) {
        const uint32_t w = pl.width[k];
        for (uint32_t col = 0; col < w; ++col) {
            if (pl.m[k]) pl.m[k][(size_t)i * w + col] = 0.0f;
            if (pl.v[k]) pl.v[k][(size_t)i * w + col] = 0.0f;
        }
    }
}

// ---- noise ------------------------------------------------------------------------------------------------------------------------

// means += Sigma xi g scale for one splat, binary32, one rounding per operation as written
__device__ __forceinline__ void noise_one(uint32_t i, uint32_t step, uint2 key, float scale, float logit, float l0, float l1, float l2, float4 q,
                                          float &mx, float &my, float &mz) {
#pragma clang fp contract(off)
    const float o = 1.0f / (1.0f + expf(-logit));
    const float g = 1.0f / (1.0f + expf(-100.0f * (0.005f - o)));
    const float3 xi = philox_normals3(philox4x32_10(make_uint4(i, step, 3u, 0u), key));
    const float k = 1.0f / sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w); // (w, x, y, z), normalised as ellipsoid_record() does
    const float qr = q.x * k, qx = q.y * k, qy = q.z * k, qz = q.w * k;
    const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r01 = 2.0f * (qx * qy - qr * qz), r02 = 2.0f * (qx * qz + qr * qy);
    const float r10 = 2.0f * (qx * qy + qr * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r12 = 2.0f * (qy * qz - qr * qx);
    const float r20 = 2.0f * (qx * qz - qr * qy), r21 = 2.0f * (qy * qz + qr * qx), r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
    // Sigma xi = R diag(exp(2 l)) R^T xi
    const float v0 = ((r00 * xi.x + r10 * xi.y) + r20 * xi.z) * expf(2.0f * l0);
    const float v1 = ((r01 * xi.x + r11 * xi.y) + r21 * xi.z) * expf(2.0f * l1);
    const float v2 = ((r02 * xi.x + r12 * xi.y) + r22 * xi.z) * expf(2.0f * l2);
    const float gs = g * scale;
    mx += ((r00 * v0 + r01 * v1) + r02 * v2) * gs;
    my += ((r10 * v0 + r11 * v1) + r12 * v2) * gs;
    mz += ((r20 * v0 + r21 * v1) + r22 * v2) * gs;
}

template <bool VEC>
__global__ __launch_bounds__(MT) void k_mcmc_noise(float *__restrict__ means, const float *__restrict__ log_scales, const float *__restrict__ rotations,
                                                   const float *__restrict__ logits, uint32_t n, uint32_t step, uint2 key, float scale) {
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    uint32_t i = t;
    if constexpr (VEC) {
        const uint32_t quads = n >> 2;
        if (t < quads) {
            float4 *mu = reinterpret_cast<float4 *>(means) + 3 * (size_t)t;
            const float4 *ls = reinterpret_cast<const float4 *>(log_scales) + 3 * (size_t)t;
            float4 m0 = mu[0], m1 = mu[1], m2 = mu[2];
            const float4 s0 = ls[0], s1 = ls[1], s2 = ls[2];
            const float4 lg = reinterpret_cast<const float4 *>(logits)[t];
            const float4 *rot = reinterpret_cast<const float4 *>(rotations) + 4 * (size_t)t;
            const float4 q0 = rot[0], q1 = rot[1], q2 = rot[2], q3 = rot[3];
            const uint32_t b = t << 2;
            noise_one(b, step, key, scale, lg.x, s0.x, s0.y, s0.z, q0, m0.x, m0.y, m0.z);
            noise_one(b + 1, step, key, scale, lg.y, s0.w, s1.x, s1.y, q1, m0.w, m1.x, m1.y);
            noise_one(b + 2, step, key, scale, lg.z, s1.z, s1.w, s2.x, q2, m1.z, m1.w, m2.x);
            noise_one(b + 3, step, key, scale, lg.w, s2.y, s2.z, s2.w, q3, m2.y, m2.z, m2.w);
            mu[0] = m0;
            mu[1] = m1;
            mu[2] = m2;
            return;
        }
        i = (n & ~3u) + (t - quads); // the splats past the last whole four
    }
    if (i >= n) return;
    const size_t e = 3 * (size_t)i;
    float mx = means[e], my = means[e + 1], mz = means[e + 2];
    const float *q = rotations + 4 * (size_t)i;
    noise_one(i, step, key, scale, logits[i], log_scales[e], log_scales[e + 1], log_scales[e + 2], make_float4(q[0], q[1], q[2], q[3]), mx, my, mz);
    means[e] = mx;
    means[e + 1] = my;
    means[e + 2] = mz;
}

size_t plane_bytes(uint64_t bytes) { return (size_t)((bytes + 255) & ~(uint64_t)255); }
uint32_t scan64_blocks(uint32_t n) { return div_up(n, S64_TILE); }

} // namespace

extern "C" uint64_t splat_mcmc_sample_workspace_bytes(uint32_t n) {
    return 3 * (uint64_t)plane_bytes((uint64_t)n * 4) + plane_bytes((uint64_t)n * 8) + plane_bytes((uint64_t)scan64_blocks(n) * 8) + 256;
}

extern "C" int splat_mcmc_sample(splat_ctx *ctx, const void *opacity_logits, uint32_t n, uint32_t mode, uint32_t n_draws, double min_opacity,
                                 uint64_t seed, void *workspace, uint64_t workspace_bytes, void *targets, void *sources, void *counts,
                                 uint32_t *counts3_host) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    ARG_CHECK(ctx, counts3_host && (mode == SPLAT_MCMC_RELOCATE || mode == SPLAT_MCMC_ADD));
    if (n >= MCMC_MAX_SPLATS) return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_mcmc_sample: n must be below 2^30");
    counts3_host[0] = counts3_host[1] = counts3_host[2] = 0;
    if (n == 0) return SPLAT_OK;
    if (mode == SPLAT_MCMC_RELOCATE) n_draws = n; // (at most: the dead)
    ARG_CHECK(ctx, n_draws < MCMC_MAX_SPLATS && (uint64_t)n + (mode == SPLAT_MCMC_ADD ? n_draws : 0u) <= MCMC_MAX_SPLATS);
    ARG_CHECK(ctx, min_opacity >= 0.0 && min_opacity <= 1.0); // (false for a NaN)
    ARG_CHECK(ctx, opacity_logits && counts && workspace && (n_draws == 0 || (targets && sources)));
    ARG_CHECK(ctx, (((uintptr_t)opacity_logits | (uintptr_t)targets | (uintptr_t)sources | (uintptr_t)counts) & 3) == 0 &&
                       ((uintptr_t)workspace & 15) == 0);
    if (workspace_bytes < splat_mcmc_sample_workspace_bytes(n))
        return ctx_fail(ctx, SPLAT_ERR_INVALID, "splat_mcmc_sample: the workspace is smaller than splat_mcmc_sample_workspace_bytes(n)");
    const size_t p4 = plane_bytes((uint64_t)n * 4), p8 = plane_bytes((uint64_t)n * 8);
    const uint32_t blocks = scan64_blocks(n);
    char *w = (char *)workspace;
    uint32_t *weight = (uint32_t *)w, *dead = (uint32_t *)(w + p4), *rank = (uint32_t *)(w + 2 * p4);
    uint64_t *incl = (uint64_t *)(w + 3 * p4), *sums = (uint64_t *)(w + 3 * p4 + p8);
    McmcWords *words = (McmcWords *)(w + 3 * p4 + p8 + plane_bytes((uint64_t)blocks * 8));
    int rc = ctx_ensure_pinned(ctx, sizeof(McmcWords));
    if (rc != SPLAT_OK) return rc;
    const uint32_t q_min = (uint32_t)ceil(min_opacity * 16777216.0);
    const dim3 grid(div_up(n, MT)), block(MT);
    HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)n * 4, ctx->stream));
    hipLaunchKernelGGL(k_mcmc_weights, grid, block, 0, ctx->stream, (const float *)opacity_logits, n, q_min, weight, dead);
    LAUNCH_CHECK(ctx, "k_mcmc_weights");
    if ((rc = scan_exclusive_u32(ctx, dead, rank, n, &words->dead)) != SPLAT_OK) return rc;
    hipLaunchKernelGGL(k_scan64_reduce, dim3(blocks), block, 0, ctx->stream, weight, n, sums);
    LAUNCH_CHECK(ctx, "k_scan64_reduce");
    hipLaunchKernelGGL(k_scan64_sums, dim3(1), block, 0, ctx->stream, sums, blocks, words);
    LAUNCH_CHECK(ctx, "k_scan64_sums");
    hipLaunchKernelGGL(k_scan64_apply, dim3(blocks), block, 0, ctx->stream, weight, n, sums, incl);
    LAUNCH_CHECK(ctx, "k_scan64_apply");
    if (n_draws != 0) {
        hipLaunchKernelGGL(k_mcmc_draw, dim3(div_up(n_draws, MT)), block, 0, ctx->stream, mode, n, n_draws, words, incl, dead, rank,
                           make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), (uint32_t *)targets, (uint32_t *)sources, (uint32_t *)counts);
        LAUNCH_CHECK(ctx, "k_mcmc_draw");
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, words, sizeof(McmcWords), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const McmcWords *h = (const McmcWords *)ctx->pinned;
    counts3_host[0] = h->dead;
    counts3_host[1] = n - h->dead;
    counts3_host[2] = h->total == 0ull ? 0u : mode == SPLAT_MCMC_RELOCATE ? h->dead : n_draws;
    return SPLAT_OK;
}

extern "C" int splat_mcmc_apply(splat_ctx *ctx, const void *targets, const void *sources, const void *counts, uint32_t n, uint32_t n_draws,
                                uint32_t rows, double min_opacity, const splat_mcmc_planes *planes) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    if (n_draws == 0 || n == 0) return SPLAT_OK;
    ARG_CHECK(ctx, planes && targets && sources && counts && n < MCMC_MAX_SPLATS && rows >= n && rows <= MCMC_MAX_SPLATS && n_draws <= rows);
    ARG_CHECK(ctx, min_opacity >= 0.0 && min_opacity <= 1.0);
    ARG_CHECK(ctx, planes->sh_floats >= 1 && planes->sh_floats <= 48);
    ARG_CHECK(ctx, (((uintptr_t)targets | (uintptr_t)sources | (uintptr_t)counts) & 3) == 0);
    McmcPlanes pl;
    const uint32_t width[5] = {3, 3, 4, 1, planes->sh_floats};
    pl.first[0] = 0;
    for (int k = 0; k < 5; ++k) {
        ARG_CHECK(ctx, planes->param[k] && (((uintptr_t)planes->param[k] | (uintptr_t)planes->m[k] | (uintptr_t)planes->v[k]) & 3) == 0);
        pl.p[k] = (float *)planes->param[k];
        pl.m[k] = (float *)planes->m[k];
        pl.v[k] = (float *)planes->v[k];
        pl.width[k] = width[k];
        pl.first[k + 1] = pl.first[k] + width[k];
    }
    const uint64_t total = (uint64_t)n_draws * pl.first[5];
    ARG_CHECK(ctx, total <= 0xffffffffull - MT);
    const dim3 block(MT);
    hipLaunchKernelGGL(k_mcmc_rows, dim3(div_up((uint32_t)total, MT)), block, 0, ctx->stream, pl, (const uint32_t *)targets, (const uint32_t *)sources,
                       (uint32_t)total, n, rows);
    LAUNCH_CHECK(ctx, "k_mcmc_rows");
    hipLaunchKernelGGL(k_mcmc_values, dim3(div_up(n_draws, MT)), block, 0, ctx->stream, pl, (const uint32_t *)targets, (const uint32_t *)sources,
                       (const uint32_t *)counts, n_draws, n, rows, min_opacity);
    LAUNCH_CHECK(ctx, "k_mcmc_values");
    hipLaunchKernelGGL(k_mcmc_sources, dim3(div_up(n, MT)), block, 0, ctx->stream, pl, (const uint32_t *)counts, n, min_opacity);
    LAUNCH_CHECK(ctx, "k_mcmc_sources");
    return SPLAT_OK;
}

extern "C" int splat_mcmc_noise(splat_ctx *ctx, void *means, const void *log_scales, const void *rotations, const void *opacity_logits, uint32_t n,
                                double scale, uint32_t step, uint64_t seed) {
    if (!ctx) return ctx_fail(nullptr, SPLAT_ERR_INVALID, "ctx is NULL");
    if (n == 0) return SPLAT_OK;
    ARG_CHECK(ctx, means && log_scales && rotations && opacity_logits && n < MCMC_MAX_SPLATS);
    const uintptr_t all = (uintptr_t)means | (uintptr_t)log_scales | (uintptr_t)rotations | (uintptr_t)opacity_logits;
    ARG_CHECK(ctx, (all & 3) == 0);
    const bool vec = (all & 15) == 0 && n >= 4;
    const uint32_t threads = vec ? (n >> 2) + (n & 3u) : n;
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    if (vec)
        hipLaunchKernelGGL(k_mcmc_noise<true>, dim3(div_up(threads, MT)), dim3(MT), 0, ctx->stream, (float *)means, (const float *)log_scales,
                           (const float *)rotations, (const float *)opacity_logits, n, step, key, (float)scale);
    else
        hipLaunchKernelGGL(k_mcmc_noise<false>, dim3(div_up(threads, MT)), dim3(MT), 0, ctx->stream, (float *)means, (const float *)log_scales,
                           (const float *)rotations, (const float *)opacity_logits, n, step, key, (float)scale);
    LAUNCH_CHECK(ctx, "k_mcmc_noise");
    return SPLAT_OK;
}
