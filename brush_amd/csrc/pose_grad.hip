// pose_grad.hip — the gradient of a render with respect to its camera: v_viewmat[3][4] = d L / d [W | t] of the
// world-to-camera transform p = W mean + t (brush_render_backward_pose, brush_render_backward_adam_pose).
//
// The last link of the backward's chain.  For a visible splat, splat_projection_vjp (splat_vjp.hpp, shared with the
// parameter backward) already forms v_p, the gradient at p, and v_T, the gradient at T = J W; then
//   v_t_view = sum_i v_p(i)                      v_W = sum_i ( v_p(i) mean(i)^T + J(i)^T v_T(i) )
// Inherited conventions: J at the unclamped p_view; no gradient through the SH view direction (as for
// v_means), so above SH degree 0 this is the gradient with the colours held fixed; culling and tile decisions are
// piecewise constant.
//
//   k_view_grad<AA>      : one lane per visible splat in compact order, grid-stride; 12 float64 accumulators per lane,
//       added in loop order; then block_sum_words (fixed_sum.hpp): a fixed shuffle tree per wave, the four waves of a
//       workgroup through LDS in wave order; one row of 12 doubles per workgroup.  Reads the compact-order sums the way
//       the parameter VJP does (det_sums.hpp), so the atomic and the deterministic layout both work.  ~100 B gathered
//       per visible splat.
//   k_view_grad_finalize : one workgroup sums the rows in a fixed order and writes the 12 words as f32, zeros included.
// No atomics, no counters to reset, no allocation, no synchronisation: graph-capturable, and the same inputs give the
// same bits on every call.  The grid is a function of n alone.  Compiled with -ffp-contract=off like the parameter VJP.
#include "det_sums.hpp"
#include "fixed_sum.hpp"
#include "splat_vjp.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = kSumThreads;
constexpr uint32_t kPoseWords = 12;      // row-major 3x4: [v_W row r | v_t_view[r]]
constexpr uint32_t kMaxPoseRows = 2048;  // workgroups of k_view_grad

template <bool AA>
__global__ __launch_bounds__(kThreads) void k_view_grad(
    const ViewParams vp, const float *__restrict__ means, const float *__restrict__ log_scales,
    const float *__restrict__ quats, const float *__restrict__ raw_opac, const uint32_t *__restrict__ num_visible,
    uint32_t n, const uint32_t *__restrict__ global_from_compact, const float *__restrict__ v_compact, const DetSums det,
    uint32_t has_depth, double *__restrict__ rows) {
    const uint32_t V = min(*num_visible, n);
    double acc[kPoseWords];
#pragma unroll
    for (uint32_t i = 0; i < kPoseWords; i++) acc[i] = 0.0;
    for (uint32_t c = blockIdx.x * kThreads + threadIdx.x; c < V; c += gridDim.x * kThreads) {
        float4 r0, r1, r2;
        load_compact_sums(v_compact, det, c, r0, r1, r2);
        const uint32_t g = global_from_compact[c];
        float mean[3], scale[3], quat[4];
        load_splat(means, log_scales, quats, g, mean, scale, quat);
        const float vxy[2] = {r0.x, r0.y};
        const float vconic[3] = {r0.z, r0.w, r1.x};
        float o_mean[3], o_scale[3], o_quat[4];
        PoseTerms pt;
        if constexpr (AA) {  // v_comp = v_alpha sigmoid(raw), as visible_splat_vjp
            float comp;
            splat_projection_vjp<true, PoseTerms>(vp, mean, scale, quat, vxy, vconic, o_mean, o_scale, o_quat,
                                                  r2.x * det_sigmoid(raw_opac[g]), &comp, &pt);
        } else {
            splat_projection_vjp<false, PoseTerms>(vp, mean, scale, quat, vxy, vconic, o_mean, o_scale, o_quat, 0.0f,
                                                   nullptr, &pt);
        }
        if (has_depth) pt.v_p[2] = pt.v_p[2] + load_compact_depth(v_compact, det, c);  // z = p[2]
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++)
                acc[a * 4 + b] += (double)(pt.v_p[a] * mean[b] + (pt.J[0][a] * pt.v_T[0][b] + pt.J[1][a] * pt.v_T[1][b]));
            acc[a * 4 + 3] += (double)pt.v_p[a];
        }
    }
    block_sum_words(acc, [&](uint32_t t, double sum) { rows[(size_t)blockIdx.x * kPoseWords + t] = sum; });
}

// block_sum_rows: fixed per-thread strides over the rows, the fixed shuffle tree, the four waves in order: all 12 words
// every call.
__global__ __launch_bounds__(kThreads) void k_view_grad_finalize(const double *__restrict__ rows, uint32_t nrows,
                                                                 float *__restrict__ v_viewmat) {
    block_sum_rows<kPoseWords>(rows, nrows, [&](uint32_t t, double sum) { v_viewmat[t] = (float)sum; });
}

}  // namespace

uint32_t pose_grad_rows(uint32_t n) { return capped_rows(n, kThreads, kMaxPoseRows); }

size_t pose_grad_workspace_bytes(uint32_t n) { return row_bytes(max(pose_grad_rows(n), 1u), kPoseWords); }

hipError_t launch_view_grad(const ViewParams &vp, const float *means, const float *log_scales, const float *quats,
                            const float *raw_opac, const uint32_t *num_visible, uint32_t n,
                            const uint32_t *global_from_compact, const float *v_compact, const DetSumsArgs &dargs,
                            bool has_depth, bool antialiased, void *pose_ws, float *v_viewmat, hipStream_t s) {
    double *rows = static_cast<double *>(pose_ws);
    const uint32_t nrows = pose_grad_rows(n);  // 0 for an empty cloud: the finalize alone writes the twelve zeros
    if (nrows) {
        const DetSums det = make_det_sums(dargs);
        auto k = antialiased ? k_view_grad<true> : k_view_grad<false>;
        hipLaunchKernelGGL(k, dim3(nrows), dim3(kThreads), 0, s, vp, means, log_scales, quats, raw_opac, num_visible, n,
                           global_from_compact, v_compact, det, has_depth ? 1u : 0u, rows);
    }
    hipLaunchKernelGGL(k_view_grad_finalize, dim3(1), dim3(kThreads), 0, s, rows, nrows, v_viewmat);
    return hipGetLastError();
}

}  // namespace brush
