// transpose_sum.hpp — the transposing wave64 reduction of the replay kernels that send per-record sums to a splat's row
// (features.hip: k_feature_grad_quad; distortion.hip: k_distortion_grad_quad).  CP registers per lane in, one out: lane
// c < CP ends with the sum over the wave of p[c], through permlane32_swap, permlane16_swap, DPP row rotates and one
// ds_bpermute (the crossbar only, no LDS memory), so that one atomic instruction with CP lanes active can send the sums
// to consecutive words.  T is float (the association differs from lane to lane) or uint32_t (exact).
#pragma once
#include "common.hpp"

namespace brush {
namespace {

__device__ __forceinline__ uint32_t bits_of(float v) { return __float_as_uint(v); }
__device__ __forceinline__ uint32_t bits_of(uint32_t v) { return v; }
template <typename T>
__device__ __forceinline__ T from_bits(uint32_t u);
template <>
__device__ __forceinline__ float from_bits<float>(uint32_t u) { return __uint_as_float(u); }
template <>
__device__ __forceinline__ uint32_t from_bits<uint32_t>(uint32_t u) { return u; }
// lanes 0-31 <- a[l] + a[l+32], lanes 32-63 <- b[l-32] + b[l]
template <typename T>
__device__ __forceinline__ T fold32(T a, T b) {
    const auto r = __builtin_amdgcn_permlane32_swap(bits_of(a), bits_of(b), false, false);
    return from_bits<T>(r[0]) + from_bits<T>(r[1]);
}
// even rows of 16 <- a[row] + a[row+1], odd rows <- b[row-1] + b[row]
template <typename T>
__device__ __forceinline__ T fold16(T a, T b) {
    const auto r = __builtin_amdgcn_permlane16_swap(bits_of(a), bits_of(b), false, false);
    return from_bits<T>(r[0]) + from_bits<T>(r[1]);
}
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_rot_add(T v) {
    return v + from_bits<T>((uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits_of(v), CTRL, 0xf, 0xf, true));
}
// Sum of a row of 16 lanes, in every lane of the row.
template <typename T>
__device__ __forceinline__ T row_all_sum(T v) {
    v = dpp_rot_add<0x128>(v);  // row_ror:8
    v = dpp_rot_add<0x124>(v);  // row_ror:4
    v = dpp_rot_add<0x122>(v);  // row_ror:2
    v = dpp_rot_add<0x121>(v);  // row_ror:1
    return v;
}
template <int CP, typename T>
__device__ __forceinline__ T transpose_sum(const T (&p)[CP], uint32_t lane) {
    constexpr int R = CP / 4;  // registers left after the two swaps: row r of register k holds channel k + r R
    T x[CP / 2], y[R];
#pragma unroll
    for (int k = 0; k < CP / 2; k++) x[k] = fold32(p[k], p[k + CP / 2]);
#pragma unroll
    for (int k = 0; k < R; k++) y[k] = row_all_sum(fold16(x[k], x[k + R]));
    T val = y[0];
#pragma unroll
    for (int k = 1; k < R; k++) val = (lane & (uint32_t)(R - 1)) == (uint32_t)k ? y[k] : val;
    // lane 16 r + j (j < R) holds channel r R + j; lane c fetches channel c (the crossbar of ds_bpermute, no LDS memory)
    const uint32_t src = (16u * (lane / (uint32_t)R) + (lane % (uint32_t)R)) & 63u;
    return from_bits<T>((uint32_t)__builtin_amdgcn_ds_bpermute((int)(src * 4u), (int)bits_of(val)));
}

}  // namespace
}  // namespace brush
