// exposure.hip — per-view exposure compensation: a 3x4 affine colour map E = [A | b] (row-major, 12 floats) applied to a
// rendered image before the loss, its two gradients, and the Adam step of E (brush_exposure_forward, _backward,
// _backward_adam).  For a premultiplied pixel p = (r, g, b, alpha):
//   out_c = A[c][0] r + A[c][1] g + A[c][2] b + alpha b_c      out_alpha = alpha
// i.e. A c + b on the un-premultiplied colour, premultiplied again: an empty pixel stays empty.  With v' = d L / d out:
//   v_p[k] = sum_c A[c][k] v'_c     v_alpha = v'_alpha + sum_c b_c v'_c     v_E[c][k] = sum_pixels v'_c p_k  (p_3 = alpha)
//
//   k_exposure_forward      : one pixel per lane, one 16-byte load and one 16-byte store; E is 12 wave-uniform words.
//   k_exposure_backward     : one pixel per lane, grid-stride; writes v_pred (may alias v_out: a lane reads its pixel
//       before it writes it) and carries 12 float64 accumulators, each product (double) v' * (double) p exact, added in
//       loop order; then block_sum_words (fixed_sum.hpp): a fixed shuffle tree per wave, the four waves through LDS in
//       wave order, one row of 12 doubles per workgroup with ordinary stores.
//   k_exposure_finalize<ADAM>: one workgroup sums the rows at fixed strides through the same tree (block_sum_rows) and
//       writes the 12 words as f32, zeros included; with ADAM it then adds the penalty reg (E - [I|0]) and steps m1, m2
//       and E of the view in place, in float64 from the stored f32 words, each stored word rounded once.
// No atomics, no counters, no allocation, no synchronisation: graph-capturable, and the same inputs give the same bits
// on every call.  The grids are functions of w h alone.  Compiled with -ffp-contract=off.
// Roofline: HBM streams (forward 16 B read + 16 B written per pixel; backward 32 B read + 16 B written).
#include <cmath>

#include "fixed_sum.hpp"
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = kSumThreads;
constexpr uint32_t kExpWords = 12;       // row-major 3x4: [A row c | b_c]
// Workgroups of k_exposure_backward: two per CU.  The wave reduction behind the loop is 144 LDS-crossbar shuffles per
// wave whatever the image, so more workgroups cost more than they hide (1080p: 24.6 us at 2048, 21.3 at 1024, 18.2 at
// 512, 19.4 at 256).
constexpr uint32_t kMaxExpRows = 512;

__global__ __launch_bounds__(kThreads) void k_exposure_forward(const float4 *__restrict__ pred,
                                                               const float *__restrict__ E, uint32_t npix,
                                                               float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const float4 p = pred[i];
    float4 o;
    o.x = ((E[0] * p.x + E[1] * p.y) + E[2] * p.z) + p.w * E[3];
    o.y = ((E[4] * p.x + E[5] * p.y) + E[6] * p.z) + p.w * E[7];
    o.z = ((E[8] * p.x + E[9] * p.y) + E[10] * p.z) + p.w * E[11];
    o.w = p.w;
    out[i] = o;
}

// v_out and v_pred may be the same array: neither is __restrict__.
__global__ __launch_bounds__(kThreads) void k_exposure_backward(const float4 *__restrict__ pred, const float4 *v_out,
                                                                const float *__restrict__ E, uint32_t npix,
                                                                float4 *v_pred, double *__restrict__ rows) {
    float e[kExpWords];
#pragma unroll
    for (uint32_t i = 0; i < kExpWords; i++) e[i] = E[i];
    double acc[kExpWords];
#pragma unroll
    for (uint32_t i = 0; i < kExpWords; i++) acc[i] = 0.0;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < npix; i += gridDim.x * kThreads) {
        const float4 p = pred[i];
        const float4 v = v_out[i];
        float4 o;
        o.x = (e[0] * v.x + e[4] * v.y) + e[8] * v.z;
        o.y = (e[1] * v.x + e[5] * v.y) + e[9] * v.z;
        o.z = (e[2] * v.x + e[6] * v.y) + e[10] * v.z;
        o.w = v.w + ((e[3] * v.x + e[7] * v.y) + e[11] * v.z);
        v_pred[i] = o;
        const double pk[4] = {(double)p.x, (double)p.y, (double)p.z, (double)p.w};
        const double vc[3] = {(double)v.x, (double)v.y, (double)v.z};
#pragma unroll
        for (int c = 0; c < 3; c++) {
#pragma unroll
            for (int k = 0; k < 4; k++) acc[c * 4 + k] += vc[c] * pk[k];
        }
    }
    block_sum_words(acc, [&](uint32_t t, double sum) { rows[(size_t)blockIdx.x * kExpWords + t] = sum; });
}

struct ExposureAdam {
    float *E, *m1, *m2;  // this view's 12 words each, updated in place
    double lr, beta1, beta2, eps, reg, bc1, bc2;  // bc = 1 - beta^time
};

// block_sum_rows: fixed per-thread strides over the rows, the fixed shuffle tree, the four waves in order: all 12 words
// every call.
template <bool ADAM>
__global__ __launch_bounds__(kThreads) void k_exposure_finalize(const double *__restrict__ rows, uint32_t nrows,
                                                                float *__restrict__ v_exposure, const ExposureAdam a) {
    block_sum_rows<kExpWords>(rows, nrows, [&](uint32_t t, double sum) {
        v_exposure[t] = (float)sum;
        if constexpr (ADAM) {
            const double x = (double)a.E[t];
            const double ident = (t == 0 || t == 5 || t == 10) ? 1.0 : 0.0;
            const double g = sum + a.reg * (x - ident);
            const double m = a.beta1 * (double)a.m1[t] + (1.0 - a.beta1) * g;
            const double v = a.beta2 * (double)a.m2[t] + (1.0 - a.beta2) * (g * g);
            a.m1[t] = (float)m;
            a.m2[t] = (float)v;
            a.E[t] = (float)(x - a.lr * (m / a.bc1) / (sqrt(v / a.bc2) + a.eps));
        }
    });
}

uint32_t exposure_rows(uint32_t npix) { return capped_rows(npix, kThreads, kMaxExpRows); }
size_t exposure_workspace_bytes(uint32_t npix) { return row_bytes(exposure_rows(npix), kExpWords); }

int backward_common(const float *pred, const float *v_out, const float *exposure, uint32_t w, uint32_t h, float *v_pred,
                    float *v_exposure, void *workspace, size_t workspace_bytes, const ExposureAdam *adam,
                    brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !pred || !v_out || !exposure || !v_pred || !v_exposure || !workspace) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(v_out, 16) || misaligned(v_pred, 16) || misaligned(exposure, 4) ||
        misaligned(v_exposure, 4) || misaligned(workspace, 8) || v_pred == pred)
        return BRUSH_ERR_INVALID_ARG;
    if (workspace_bytes < exposure_workspace_bytes(npix)) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *rows = static_cast<double *>(workspace);
    const uint32_t nrows = exposure_rows(npix);
    hipLaunchKernelGGL(k_exposure_backward, dim3(nrows), dim3(kThreads), 0, s, reinterpret_cast<const float4 *>(pred),
                       reinterpret_cast<const float4 *>(v_out), exposure, npix, reinterpret_cast<float4 *>(v_pred), rows);
    if (adam)
        hipLaunchKernelGGL(k_exposure_finalize<true>, dim3(1), dim3(kThreads), 0, s, rows, nrows, v_exposure, *adam);
    else
        hipLaunchKernelGGL(k_exposure_finalize<false>, dim3(1), dim3(kThreads), 0, s, rows, nrows, v_exposure,
                           ExposureAdam{});
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_exposure_workspace_size(uint32_t w, uint32_t h, size_t *bytes) {
    const uint32_t npix = checked_pixels(w, h);
    if (!bytes || !npix) return BRUSH_ERR_INVALID_ARG;
    *bytes = exposure_workspace_bytes(npix);
    return BRUSH_OK;
}

extern "C" int brush_exposure_forward(const float *pred, const float *exposure, uint32_t w, uint32_t h, float *out,
                                      brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !pred || !exposure || !out || out == pred) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(out, 16) || misaligned(exposure, 4)) return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_exposure_forward, dim3(ceil_div(npix, kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const float4 *>(pred), exposure, npix,
                       reinterpret_cast<float4 *>(out));
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_exposure_backward(const float *pred, const float *v_out, const float *exposure, uint32_t w,
                                       uint32_t h, float *v_pred, float *v_exposure, void *workspace,
                                       size_t workspace_bytes, brush_stream_t stream) {
    return backward_common(pred, v_out, exposure, w, h, v_pred, v_exposure, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int brush_exposure_backward_adam(const float *pred, const float *v_out, const BrushExposureAdam *cfg,
                                            uint32_t w, uint32_t h, float *v_pred, float *exposure, float *moment1,
                                            float *moment2, float *v_exposure, void *workspace, size_t workspace_bytes,
                                            brush_stream_t stream) {
    if (!cfg || cfg->time == 0 || !moment1 || !moment2 || misaligned(moment1, 4) || misaligned(moment2, 4))
        return BRUSH_ERR_INVALID_ARG;
    ExposureAdam a;
    a.E = exposure, a.m1 = moment1, a.m2 = moment2;
    a.lr = (double)cfg->lr, a.beta1 = (double)cfg->beta1, a.beta2 = (double)cfg->beta2;
    a.eps = (double)cfg->epsilon, a.reg = (double)cfg->reg;
    a.bc1 = 1.0 - std::pow(a.beta1, (double)cfg->time);
    a.bc2 = 1.0 - std::pow(a.beta2, (double)cfg->time);
    return backward_common(pred, v_out, exposure, w, h, v_pred, v_exposure, workspace, workspace_bytes, &a, stream);
}
