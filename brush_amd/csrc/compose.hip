// compose.hip — background colour and loss mask in front of the colour loss (brush_compose_forward, _backward): the
// premultiplied render is composed over a background colour, a straight-alpha target over the same colour, and both are
// zeroed where a mask says "leave this pixel out".  With a = pred.w, b the background, G the target, G_a its alpha:
//   out_pred.c = pred.c + (1 - a) b_c     out_pred.w = a
//   out_gt.c   = G_c G_a + (1 - G_a) b_c  (4-channel target; a 3-channel one is copied)
// and with v = d L / d out_pred:  v_pred.c = v.c,  v_pred.w = v.w - ((b_0 v_0 + b_1 v_1) + b_2 v_2).
// A pixel is kept when there is no mask or mask[p] != 0; every word of a pixel that is not kept is +0.0f, chosen by
// selection (v_cndmask), never by multiplication: a NaN under the mask stays there.
//
//   k_compose_forward<GT, CG, BG, MASK>: one pixel per lane over the whole grid, no stride loop (w h < 2^28 fits one):
//       one 16-byte load and one 16-byte store of the f32 pixel; the target is read as CG elements (u8 through ld_gt's
//       IEEE division) and written as 3 (BG) or CG f32 words; the background is 3 wave-uniform words.
//   k_compose_backward<BG, MASK>       : the same shape; v_pred may alias v_out (a lane reads its pixel before it
//       writes it).
// No LDS, no atomics, no allocation, no synchronisation: graph-capturable, and the same inputs give the same bits on
// every call.  Compiled with -ffp-contract=off: every operation above is one f32 operation rounded on its own.
// Roofline: HBM streams (forward 16 + CG sizeof(GT) + 1 B read, 16 + 4 (3 | CG) B written per pixel; backward 16 + 1 B
// read, 16 B written).
#include "internal.hpp"
#include "ssim_dev.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;

template <typename GT, int CG, bool BG, bool MASK>
__global__ __launch_bounds__(kThreads) void k_compose_forward(const float4 *__restrict__ pred,
                                                              const GT *__restrict__ gt,
                                                              const uint8_t *__restrict__ mask,
                                                              const float *__restrict__ background, uint32_t npix,
                                                              float4 *__restrict__ out_pred,
                                                              float *__restrict__ out_gt) {
    constexpr int CO = BG ? 3 : CG;  // channels of out_gt
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const float4 p = pred[i];
    float g[CG];
#pragma unroll
    for (int k = 0; k < CG; k++) g[k] = ld_gt(gt, i * (uint32_t)CG + (uint32_t)k);
    bool keep = true;
    if constexpr (MASK) keep = mask[i] != 0;
    float4 o = p;
    float t[CO];
    if constexpr (BG) {
        const float b[3] = {background[0], background[1], background[2]};
        const float tr = 1.0f - p.w;
        o.x = p.x + tr * b[0];
        o.y = p.y + tr * b[1];
        o.z = p.z + tr * b[2];
        if constexpr (CG == 4) {
            const float s = 1.0f - g[3];
#pragma unroll
            for (int c = 0; c < 3; c++) t[c] = g[c] * g[3] + s * b[c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) t[c] = g[c];
        }
    } else {
#pragma unroll
        for (int k = 0; k < CG; k++) t[k] = g[k];
    }
    if constexpr (MASK) {
        o.x = keep ? o.x : 0.0f;
        o.y = keep ? o.y : 0.0f;
        o.z = keep ? o.z : 0.0f;
        o.w = keep ? o.w : 0.0f;
#pragma unroll
        for (int k = 0; k < CO; k++) t[k] = keep ? t[k] : 0.0f;
    }
    out_pred[i] = o;
    if constexpr (CO == 4) {
        reinterpret_cast<float4 *>(out_gt)[i] = make_float4(t[0], t[1], t[2], t[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) out_gt[(size_t)i * 3 + k] = t[k];
    }
}

// v_out and v_pred may be the same array: neither is __restrict__.
template <bool BG, bool MASK>
__global__ __launch_bounds__(kThreads) void k_compose_backward(const float4 *v_out, const uint8_t *__restrict__ mask,
                                                               const float *__restrict__ background, uint32_t npix,
                                                               float4 *v_pred) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const float4 v = v_out[i];
    float4 o = v;
    if constexpr (BG) o.w = v.w - ((background[0] * v.x + background[1] * v.y) + background[2] * v.z);
    if constexpr (MASK) {
        const bool keep = mask[i] != 0;
        o.x = keep ? o.x : 0.0f;
        o.y = keep ? o.y : 0.0f;
        o.z = keep ? o.z : 0.0f;
        o.w = keep ? o.w : 0.0f;
    }
    v_pred[i] = o;
}

template <typename GT, int CG>
void launch_forward(const float *pred, const void *gt, const uint8_t *mask, const float *background, uint32_t npix,
                    float *out_pred, float *out_gt, hipStream_t s) {
    const dim3 grid(ceil_div(npix, kThreads)), block(kThreads);
    const float4 *p = reinterpret_cast<const float4 *>(pred);
    float4 *o = reinterpret_cast<float4 *>(out_pred);
    const GT *g = static_cast<const GT *>(gt);
    if (background && mask)
        hipLaunchKernelGGL((k_compose_forward<GT, CG, true, true>), grid, block, 0, s, p, g, mask, background, npix, o,
                           out_gt);
    else if (background)
        hipLaunchKernelGGL((k_compose_forward<GT, CG, true, false>), grid, block, 0, s, p, g, mask, background, npix, o,
                           out_gt);
    else
        hipLaunchKernelGGL((k_compose_forward<GT, CG, false, true>), grid, block, 0, s, p, g, mask, background, npix, o,
                           out_gt);
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_compose_forward(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t gt_channels,
                                     const uint8_t *mask, const float *background, uint32_t w, uint32_t h,
                                     float *out_pred, float *out_gt, brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !pred || !gt || !out_pred || !out_gt || (!mask && !background)) return BRUSH_ERR_INVALID_ARG;
    if (gt_dtype > BRUSH_EVAL_GT_F32 || (gt_channels != 3 && gt_channels != 4)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(gt, 16) || misaligned(out_pred, 16) || misaligned(out_gt, 16) ||
        misaligned(background, 4))
        return BRUSH_ERR_INVALID_ARG;
    if (out_pred == pred || static_cast<const void *>(out_gt) == gt || out_gt == out_pred) return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool u8 = gt_dtype == BRUSH_EVAL_GT_U8;
    if (gt_channels == 3)
        u8 ? launch_forward<uint8_t, 3>(pred, gt, mask, background, npix, out_pred, out_gt, s)
           : launch_forward<float, 3>(pred, gt, mask, background, npix, out_pred, out_gt, s);
    else
        u8 ? launch_forward<uint8_t, 4>(pred, gt, mask, background, npix, out_pred, out_gt, s)
           : launch_forward<float, 4>(pred, gt, mask, background, npix, out_pred, out_gt, s);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_compose_backward(const float *v_out, const uint8_t *mask, const float *background, uint32_t w,
                                      uint32_t h, float *v_pred, brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !v_out || !v_pred || (!mask && !background)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(v_out, 16) || misaligned(v_pred, 16) || misaligned(background, 4)) return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(npix, kThreads)), block(kThreads);
    const float4 *v = reinterpret_cast<const float4 *>(v_out);
    float4 *o = reinterpret_cast<float4 *>(v_pred);
    if (background && mask)
        hipLaunchKernelGGL((k_compose_backward<true, true>), grid, block, 0, s, v, mask, background, npix, o);
    else if (background)
        hipLaunchKernelGGL((k_compose_backward<true, false>), grid, block, 0, s, v, mask, background, npix, o);
    else
        hipLaunchKernelGGL((k_compose_backward<false, true>), grid, block, 0, s, v, mask, background, npix, o);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
