// wave_reduce.h — a value combined over the 64 lanes of a wave with DPP moves, the result valid in lane 63.
//
//   wave_reduce63(v, op)   six steps v = op(v, v moved): quad swaps, rotations by 4 and 8 in each row of 16 lanes, then the
//                          row broadcasts 15 and 31 into rows 1, 3 and 2, 3.  A lane a row mask leaves out of a move reads
//                          0, so op needs 0 as its neutral element; the order of the combinations is fixed, so a float sum
//                          is the same bits on every run.  A double moves as its two words.
//   wave_sum63(float), wave_sum63_f64(double), wave_add63_u32, wave_max63_u32   the instances the gradient kernels use.
#pragma once
#include "common.h"

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_move(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_move(uint32_t v) {
    return (uint32_t)dpp_move<CTRL, ROW_MASK>((int)v);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(dpp_move<CTRL, ROW_MASK>(__float_as_int(v)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = dpp_move<CTRL, ROW_MASK>(__double2loint(v));
    const int hi = dpp_move<CTRL, ROW_MASK>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce63(T v, Op op) {
    v = op(v, dpp_move<0xb1, 0xf>(v));  // quad_perm [1,0,3,2]
    v = op(v, dpp_move<0x4e, 0xf>(v));  // quad_perm [2,3,0,1]
    v = op(v, dpp_move<0x124, 0xf>(v)); // row_ror:4
    v = op(v, dpp_move<0x128, 0xf>(v)); // row_ror:8
    v = op(v, dpp_move<0x142, 0xa>(v)); // row_bcast:15
    v = op(v, dpp_move<0x143, 0xc>(v)); // row_bcast:31
    return v;
}

__device__ __forceinline__ float wave_sum63(float v) {
    return wave_reduce63(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ double wave_sum63_f64(double v) {
    return wave_reduce63(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ uint32_t wave_add63_u32(uint32_t v) {
    return wave_reduce63(v, [](uint32_t a, uint32_t b) { return a + b; });
}
__device__ __forceinline__ uint32_t wave_max63_u32(uint32_t v) {
    return wave_reduce63(v, [](uint32_t a, uint32_t b) { return max(a, b); });
}
