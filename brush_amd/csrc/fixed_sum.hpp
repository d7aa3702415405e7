// fixed_sum.hpp — the fixed-order sums behind the promise that the same inputs give the same bits on every call: the
// pose gradient, exposure compensation, the depth loss, the eval metrics and the image loss all reduce through the
// pieces here.  A workgroup of these reductions is kSumWaves waves of 64 lanes.  Three steps, each with one order that
// is part of the results' bits:
//   tree_sum : inside a wave, the xor-shuffle tree (offsets 32, 16, ... 1; every lane ends with the sum).  Not the DPP
//       scan behind wave_sum(uint32_t) of common.hpp: that one is integer-only, and a floating-point scan associates as
//       a running prefix where the tree folds halves onto each other, so swapping one for the other changes low bits.
//       The uint32 valid count of k_depth_loss goes through the tree as well, beside its float64 twin.
//   across the waves : lane 0 of each wave puts its sum into LDS; behind a __syncthreads() the four are added
//         sum_waves_in_order  ((r0 + r1) + r2) + r3 : k_view_grad, k_view_grad_finalize (pose_grad.hip),
//             k_exposure_backward, k_exposure_finalize (exposure.hip), k_depth_loss, k_depth_loss_finalize
//             (depth_loss.hip), k_bilagrid_backward (bilagrid.hip, 48 words); block_sum_words is this order
//         sum_waves_pairwise  (r0 + r1) + (r2 + r3) : k_eval_finalize (eval.hip), block_sum of k_l1_backward
//             (train_step.hip)
//       Neither is better.  Each kernel keeps the order it was written with, because its output is held to the bit;
//       a new kernel picks one and is listed here.
//   block_sum_rows : a finalize kernel's thread t first adds the workgroup rows t, t + 256, ... in that order.
// Compiled under -ffp-contract=off and =fast alike: there is no multiply here to contract.
#pragma once
#include "common.hpp"

namespace brush {

constexpr uint32_t kSumThreads = 256;
constexpr uint32_t kSumWaves = kSumThreads / kWave;

template <typename T>  // double, float, uint32_t
__device__ __forceinline__ T tree_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The four staged wave sums red[0], red[stride], red[2 stride], red[3 stride].
template <typename T>
__device__ __forceinline__ T sum_waves_in_order(const T *red, uint32_t stride = 1) {
    return ((red[0] + red[stride]) + red[2 * stride]) + red[3 * stride];
}
template <typename T>
__device__ __forceinline__ T sum_waves_pairwise(const T *red, uint32_t stride = 1) {
    return (red[0] + red[stride]) + (red[2 * stride] + red[3 * stride]);
}

// Sum of W words over the workgroup, waves in order: thread t < W receives word t as f(t, sum).  A functor, not a
// returned value: a sum handed back at a clamped index costs the finalize kernels a v_cndmask and their schedule.
template <uint32_t W, typename F>
__device__ __forceinline__ void block_sum_words(double (&acc)[W], F &&f) {
    __shared__ double red[kSumWaves][W];
#pragma unroll
    for (uint32_t i = 0; i < W; i++) acc[i] = tree_sum(acc[i]);
    if (lane_id() == 0) {
#pragma unroll
        for (uint32_t i = 0; i < W; i++) red[threadIdx.x / kWave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < W) f(threadIdx.x, sum_waves_in_order(&red[0][threadIdx.x], W));
}

// The same over nrows rows of W words written by as many workgroups: thread t first adds rows t, t + kSumThreads, ...
// in that order.  One function with block_sum_words, not a loop helper in front of it: with the accumulators handed
// from one helper to the next the finalize kernels zero their registers in another order.
template <uint32_t W, typename F>
__device__ __forceinline__ void block_sum_rows(const double *__restrict__ rows, uint32_t nrows, F &&f) {
    double acc[W];
#pragma unroll
    for (uint32_t i = 0; i < W; i++) acc[i] = 0.0;
    for (uint32_t r = threadIdx.x; r < nrows; r += kSumThreads) {
#pragma unroll
        for (uint32_t i = 0; i < W; i++) acc[i] += rows[(size_t)r * W + i];
    }
    block_sum_words(acc, f);
}

}  // namespace brush
