// block_scan.h — the wave and workgroup idioms of the binner and the sorts, each written once.
//
//   wave_inclusive_scan(v)            inclusive sum over the lanes of a wave (six __shfl_up steps); (a, b) and (a, b, c): two or
//                                     three values riding in the same six steps
//   waves_before(wave_sums, w)        sum of the totals of the waves before wave w of a four-wave workgroup
//   block_exclusive_scan<SYNC_AFTER>  exclusive sum of one value per thread over 256 threads, and the workgroup's total
//   wave_sum(v), block_sum(v, wsum)   the xor butterfly (every lane holds the sum) and the four-wave sum on top of it
//   match_same_digit(d, active)       the lanes of this wave that hold the same 8-bit digit (eight ballots)
//   wave_rank<RANK_ATOMIC>            stable rank of a lane's element within its digit, counted in the wave's histogram
//   ts_wave_prefixes                  per digit: the four waves' counts -> exclusive wave prefixes, returns their total
//   ranks_with_atomics                the radix downsweeps' vote.  (Their epilogue — digit starts, local and global — stays in
//                                     each downsweep, built from the scans above: see k_tf_downsweep2 in tile_first.hip)
//   hist_flush<NW>                    per-wave LDS histograms -> one column of the digit-major global histogram
#pragma once
#include "common.h"

__device__ __forceinline__ uint64_t lanemask_lt() {
    const uint32_t lane = threadIdx.x & 63;
    return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T t = __shfl_up(v, s);
        if (lane >= s) v += t;
    }
    return v;
}
// (two or three values in the same six steps: `auto [x, y] = wave_inclusive_scan(a, b)`.  By value, not through references:
// the compiler keeps the adds as selects only when it sees plain values here)
template <class A, class B>
struct Scanned2 {
    A a;
    B b;
};
template <class A, class B, class C>
struct Scanned3 {
    A a;
    B b;
    C c;
};
template <class A, class B>
__device__ __forceinline__ Scanned2<A, B> wave_inclusive_scan(A a, B b) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const A ta = __shfl_up(a, s);
        const B tb = __shfl_up(b, s);
        if (lane >= s) {
            a += ta;
            b += tb;
        }
    }
    return {a, b};
}
template <class A, class B, class C>
__device__ __forceinline__ Scanned3<A, B, C> wave_inclusive_scan(A a, B b, C c) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const A ta = __shfl_up(a, s);
        const B tb = __shfl_up(b, s);
        const C tc = __shfl_up(c, s);
        if (lane >= s) {
            a += ta;
            b += tb;
            c += tc;
        }
    }
    return {a, b, c};
}

__device__ __forceinline__ uint32_t waves_before(const uint32_t *wave_sums, uint32_t w) {
    return (w > 0 ? wave_sums[0] : 0u) + (w > 1 ? wave_sums[1] : 0u) + (w > 2 ? wave_sums[2] : 0u);
}

// Exclusive scan of one value per thread over the 256 threads of a workgroup; wave_sums: 4 words of LDS.  One barrier, and with
// SYNC_AFTER a second one behind the reads of wave_sums: for a caller that writes wave_sums again before its next barrier.
template <bool SYNC_AFTER>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t *total = nullptr) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v);
    if (lane == 63) wave_sums[w] = incl;
    __syncthreads();
    const uint32_t s0 = wave_sums[0], s1 = wave_sums[1], s2 = wave_sums[2];
    if (total) *total = s0 + s1 + s2 + wave_sums[3];
    if (SYNC_AFTER) __syncthreads();
    return (w > 0 ? s0 : 0u) + (w > 1 ? s1 : 0u) + (w > 2 ? s2 : 0u) + incl - v;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// sum over a 256-thread workgroup, in every thread (one barrier; wsum: 4 words of LDS)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *wsum) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// The lanes of `active` that hold this lane's 8-bit digit: 8 ballots, each folded in with one v_bitop3 per mask half
// (peers &= ~(ballot ^ mybit)).
struct LanePeers {
    uint32_t lo, hi;
    __device__ __forceinline__ uint32_t below() const { return __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0)); } // peers in lower lanes
    __device__ __forceinline__ uint32_t leader() const { return lo ? (uint32_t)__builtin_ctz(lo) : 32u + (uint32_t)__builtin_ctz(hi); }
    __device__ __forceinline__ uint32_t count() const { return (uint32_t)(__popc(lo) + __popc(hi)); }
};
__device__ __forceinline__ LanePeers match_same_digit(uint32_t d, uint64_t active = ~0ull) {
    LanePeers p = {(uint32_t)active, (uint32_t)(active >> 32)};
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const uint32_t m = (uint32_t)(((int32_t)(d << (31 - b))) >> 31); // all ones if bit b of d is set
        const uint64_t bal = __ballot(m != 0);
        p.lo = __builtin_amdgcn_bitop3_b32(p.lo, (uint32_t)bal, m, 0x90); // lo & ~(bal ^ m)
        p.hi = __builtin_amdgcn_bitop3_b32(p.hi, (uint32_t)(bal >> 32), m, 0x90);
    }
    return p;
}

// rank of this lane's element among the elements of the same digit seen so far by this wave
// (earlier instructions, then lower lanes), adding it to the wave's digit counter
template <bool RANK_ATOMIC>
__device__ __forceinline__ uint32_t wave_rank(uint32_t *wave_hist, uint32_t d) {
    if (RANK_ATOMIC) return atomicAdd(&wave_hist[d], 1u); // lane-ordered returning LDS atomic (probed per context)
    const LanePeers p = match_same_digit(d, __ballot(true)); // callers rank under `if (p < n)`: peers are active lanes only
    const uint32_t below = p.below();
    uint32_t prev = 0;
    if (below == 0) prev = atomicAdd(&wave_hist[d], p.count());
    return (uint32_t)__shfl((int)prev, (int)p.leader()) + below;
}

// thread d: turns the four waves' counts of digit d into exclusive wave prefixes (in place) and returns
// the total; then digit_base[d] = exclusive scan of the totals over the digits (+ nothing else)
__device__ __forceinline__ uint32_t ts_wave_prefixes(uint32_t (*wave_hist)[256], uint32_t tid) {
    const uint32_t c0 = wave_hist[0][tid], c1 = wave_hist[1][tid], c2 = wave_hist[2][tid], c3 = wave_hist[3][tid];
    wave_hist[0][tid] = 0;
    wave_hist[1][tid] = c0;
    wave_hist[2][tid] = c0 + c1;
    wave_hist[3][tid] = c0 + c1 + c2;
    return c0 + c1 + c2 + c3;
}

// The downsweeps' vote (a barrier): may this partition rank with returning LDS atomics?  Those serialise when they collide on
// one counter, so not when some digit holds more than a quarter of the partition.  next - row_prefix: this thread's digit's
// count in the partition, known from the scanned histogram before the partition is read.
__device__ __forceinline__ bool ranks_with_atomics(uint32_t next, uint32_t row_prefix, uint32_t part_keys) {
    return !__syncthreads_or((next - row_prefix) > part_keys / 4);
}

// hist[d * num_parts + col] = the workgroup's count of digit d, summed over its NW per-wave histograms, for the digits that can
// occur (rows above the mask are never read: a 4-byte store per row is a 64-byte line at the memory side)
template <uint32_t NW>
__device__ __forceinline__ void hist_flush(const uint32_t (*lh)[256], uint32_t *__restrict__ hist, uint32_t num_parts, uint32_t col, uint32_t mask) {
    const uint32_t tid = threadIdx.x;
    if (tid <= mask) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < NW; ++v) s += lh[v][tid];
        hist[(size_t)tid * num_parts + col] = s;
    }
}
