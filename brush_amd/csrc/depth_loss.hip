// depth_loss.hip — depth supervision: an L1 loss between the rendered expected depth and a per-view depth map, and both
// of its gradients, in one pass over the pixels (brush_depth_loss).  Per pixel p, with a = pred[p].w (alpha of the raw
// render), D = depth[p] (the accumulated depth sum T alpha z of brush_render_forward_depth) and the target
// t = raw * scale + offset (f32 multiply, then f32 add) from a u16 or f32 map:
//   valid(p) = target present (u16: raw != 0; f32: finite and raw > 0)  and  t > 0  and  D > 0  and  a >= alpha_min
//   BRUSH_DEPTH_LOSS_DEPTH      d = D / a   r = d - t   v_D = g / a          v_a = -(g d) / a
//   BRUSH_DEPTH_LOSS_DISPARITY  q = a / D   r = q - t   v_D = -(g q) / D     v_a = g / D
// g = c sign(r), sign(0) = 0, c = (float)(weight / (w h)): the mean runs over ALL w h pixels (as the 3DGS trainer's depth
// term does), not over the valid ones, which is what lets a pixel's gradient be written in the pass that first sees it.
//
//   k_depth_loss<MODE, GT>: one pixel per lane, grid-stride.  Writes v_depth[p] (0 where invalid), adds v_a into the
//       alpha word of v_pred[p] (valid pixels only: every other word of v_pred keeps its bits), and carries one float64
//       accumulator of |r| and one exact integer count of valid pixels per lane; then the reduction of fixed_sum.hpp:
//       the fixed shuffle tree per wave (the count as uint32), the four waves through LDS in wave order, one row
//       {sum, count} per workgroup with ordinary stores.
//   k_depth_loss_finalize : one workgroup sums the rows at fixed strides through the same tree and writes
//       stats = {(float)(c sum), (float)(count / (w h))}; with loss_accum it then does *loss_accum += stats[0].
// No atomics, no counters, no allocation, no synchronisation: graph-capturable, and the same inputs give the same bits
// on every call.  The grids are functions of w h alone.  Compiled with -ffp-contract=off; the divisions are IEEE.
// Roofline: HBM stream.  Useful bytes per pixel: 4 (alpha) + 4 (D) + 2|4 (target) read, 4 (v_depth) written, 4 + 4 for
// the alpha read-modify-write; the two stride-16 alpha accesses move whole lines of pred and v_pred, so the traffic is
// 16 + 4 + 2|4 + 4 + 16 + 16 = 58|60 bytes per pixel.
#include <cmath>

#include "fixed_sum.hpp"
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = kSumThreads;
// Workgroups of k_depth_loss: four per CU; larger images take further sweeps of the grid-stride loop.
constexpr uint32_t kMaxDepthRows = 1024;
constexpr uint32_t kRowWords = 2;  // {sum |r|, valid count}, both float64 (a count below 2^28 is exact)

// The raw target word as f32, and whether the map holds a measurement there.
__device__ __forceinline__ bool ld_target(const uint16_t *t, uint32_t i, float &raw) {
    const uint16_t x = t[i];
    raw = (float)x;
    return x != 0;
}
__device__ __forceinline__ bool ld_target(const float *t, uint32_t i, float &raw) {
    raw = t[i];
    return raw > 0.0f && raw < INFINITY;  // NaN fails both
}

struct DepthLossArgs {
    float c, scale, offset, alpha_min;
};

// v_pred is read and written at the alpha word only; pred and v_pred are different arrays (checked by the entry point).
template <uint32_t MODE, typename GT>
__global__ __launch_bounds__(kThreads) void k_depth_loss(const float4 *__restrict__ pred, const float *__restrict__ depth,
                                                         const GT *__restrict__ target, const DepthLossArgs a,
                                                         uint32_t npix, float *__restrict__ v_depth,
                                                         float *__restrict__ v_pred, double *__restrict__ rows) {
    __shared__ double red_sum[kThreads / kWave];
    __shared__ uint32_t red_cnt[kThreads / kWave];
    double acc = 0.0;
    uint32_t cnt = 0;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < npix; i += gridDim.x * kThreads) {
        const float al = reinterpret_cast<const float *>(pred)[(size_t)i * 4 + 3];
        const float D = depth[i];
        float raw;
        const bool present = ld_target(target, i, raw);
        const float t = raw * a.scale + a.offset;
        const bool valid = present && t > 0.0f && D > 0.0f && al >= a.alpha_min;
        float vD = 0.0f;
        if (valid) {
            float r, va;
            if constexpr (MODE == BRUSH_DEPTH_LOSS_DEPTH) {
                const float d = D / al;
                r = d - t;
                const float g = a.c * (r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f));
                vD = g / al;
                va = -(g * d) / al;
            } else {
                const float q = al / D;
                r = q - t;
                const float g = a.c * (r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f));
                vD = -(g * q) / D;
                va = g / D;
            }
            acc += (double)fabsf(r);
            cnt += 1u;
            if (v_pred) v_pred[(size_t)i * 4 + 3] += va;
        }
        if (v_depth) v_depth[i] = vD;
    }
    acc = tree_sum(acc);
    cnt = tree_sum(cnt);
    if (lane_id() == 0) red_sum[threadIdx.x / kWave] = acc, red_cnt[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        rows[(size_t)blockIdx.x * kRowWords + 0] = sum_waves_in_order(red_sum);
        rows[(size_t)blockIdx.x * kRowWords + 1] = (double)sum_waves_in_order(red_cnt);  // uint32 until here
    }
}

// Fixed per-thread strides over the rows, the fixed shuffle tree, the four waves in order (fixed_sum.hpp).
__global__ __launch_bounds__(kThreads) void k_depth_loss_finalize(const double *__restrict__ rows, uint32_t nrows,
                                                                  float c, uint32_t npix, float *__restrict__ stats,
                                                                  float *__restrict__ loss_accum) {
    __shared__ double red[kThreads / kWave][kRowWords];
    double sum = 0.0, cnt = 0.0;  // block_sum_rows (fixed_sum.hpp) written out: thread 0 takes both words
    for (uint32_t r = threadIdx.x; r < nrows; r += kThreads) {
        sum += rows[(size_t)r * kRowWords + 0];
        cnt += rows[(size_t)r * kRowWords + 1];
    }
    sum = tree_sum(sum);
    cnt = tree_sum(cnt);
    if (lane_id() == 0) red[threadIdx.x / kWave][0] = sum, red[threadIdx.x / kWave][1] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = sum_waves_in_order(&red[0][0], kRowWords);
        const double n = sum_waves_in_order(&red[0][1], kRowWords);
        const float loss = (float)((double)c * s);
        stats[0] = loss;
        stats[1] = (float)(n / (double)npix);
        if (loss_accum) *loss_accum += loss;
    }
}

uint32_t depth_loss_rows(uint32_t npix) { return capped_rows(npix, kThreads, kMaxDepthRows); }
size_t depth_loss_workspace_bytes(uint32_t npix) { return row_bytes(depth_loss_rows(npix), kRowWords); }

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_depth_loss_workspace_size(uint32_t w, uint32_t h, size_t *bytes) {
    const uint32_t npix = checked_pixels(w, h);
    if (!bytes || !npix) return BRUSH_ERR_INVALID_ARG;
    *bytes = depth_loss_workspace_bytes(npix);
    return BRUSH_OK;
}

extern "C" int brush_depth_loss(const float *pred, const float *depth, const void *target, const BrushDepthLoss *cfg,
                                uint32_t w, uint32_t h, float *v_depth, float *v_pred, float *stats, float *loss_accum,
                                void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !pred || !depth || !target || !cfg || !stats || !workspace) return BRUSH_ERR_INVALID_ARG;
    if (!(cfg->alpha_min > 0.0f) || cfg->mode > BRUSH_DEPTH_LOSS_DISPARITY || cfg->gt_dtype > BRUSH_DEPTH_GT_F32)
        return BRUSH_ERR_INVALID_ARG;
    const bool u16 = cfg->gt_dtype == BRUSH_DEPTH_GT_U16;
    if (misaligned(pred, 16) || misaligned(depth, 4) || misaligned(target, u16 ? 2 : 4) || misaligned(v_depth, 4) ||
        misaligned(v_pred, 16) || misaligned(stats, 4) || misaligned(loss_accum, 4) || misaligned(workspace, 8) ||
        v_pred == pred || (v_depth && v_depth == depth))
        return BRUSH_ERR_INVALID_ARG;
    if (workspace_bytes < depth_loss_workspace_bytes(npix)) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *rows = static_cast<double *>(workspace);
    const uint32_t nrows = depth_loss_rows(npix);
    DepthLossArgs a;
    a.c = (float)((double)cfg->weight / (double)npix);
    a.scale = cfg->scale, a.offset = cfg->offset, a.alpha_min = cfg->alpha_min;
    auto launch = [&](auto mode, auto gt) {  // (mode, target type) -> template arguments, as dispatch_dm
        using GT = decltype(gt);
        hipLaunchKernelGGL((k_depth_loss<mode(), GT>), dim3(nrows), dim3(kThreads), 0, s,
                           reinterpret_cast<const float4 *>(pred), depth, static_cast<const GT *>(target), a, npix,
                           v_depth, v_pred, rows);
    };
    auto by_dtype = [&](auto mode) { u16 ? launch(mode, uint16_t{}) : launch(mode, float{}); };
    cfg->mode == BRUSH_DEPTH_LOSS_DEPTH ? by_dtype(IntC<BRUSH_DEPTH_LOSS_DEPTH>{})
                                        : by_dtype(IntC<BRUSH_DEPTH_LOSS_DISPARITY>{});
    hipLaunchKernelGGL(k_depth_loss_finalize, dim3(1), dim3(kThreads), 0, s, rows, nrows, a.c, npix, stats, loss_accum);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
