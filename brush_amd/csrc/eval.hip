// eval.hip — image metrics of a held-out view (eval_stats, crates/brush-train/src/eval.rs:27-77): MSE and PSNR of the
// RGB channels (eval.rs:55-59) and the mean of the SSIM map of ssim.rs:42-101 (Ssim::new(window, 3)).
//
//   k_eval_metrics : the separable two-pass blur of k_ssim_forward (train_step.hip) with nothing per pixel written: no
//       derivative maps, only per-wave partial sums of the SSIM map and of the squared RGB error.  A wave marches a
//       64-column strip of one colour channel down the image; per marched row the lane's (pred, gt) pair goes through a
//       per-wave LDS row buffer for the horizontal blur of the five moments, the vertical blur runs over a register
//       ring of the last WIN blurred rows.  Reads 4 B of pred and 1 or 4 B of gt per pixel and channel (the halo
//       re-reads stay in L2); writes 16 B per wave.  Alpha is never read: the reference compares to_rgb8() images,
//       dropping alpha without blending (eval.rs:50-57).
//   k_eval_finalize : one workgroup sums the partials in a fixed order (f64; fixed_sum.hpp, the four waves pairwise)
//       and writes {mse, psnr, ssim}.
// No atomics and a fixed reduction order: the same inputs give the same bits on every call and stream.
#include "internal.hpp"
#include "ssim_dev.hpp"

namespace brush {
namespace {

constexpr float kLn10 = 2.30258509299404568402f;  // std::f32::consts::LN_10
constexpr int kFinalizeThreads = kSumThreads;

// SSIM map position (oy, ox) for oy in the block's kSegRows rows, ox in the wave's kOutCols columns; the squared error
// of input pixel (iy, ix) is counted by the wave holding map position (iy+1, ix+1), as k_ssim_forward counts |pred-gt|.
template <int WIN, typename GT>
__global__ __launch_bounds__(192) void k_eval_metrics(const float *__restrict__ pred, const GT *__restrict__ gt,
                                                      uint32_t gt_channels, uint32_t w, uint32_t h, Window win,
                                                      double *__restrict__ partials) {
    using G = Geo<WIN>;
    __shared__ float rows[3][2][kRowBuf];
    const int ch = threadIdx.x / kWave, l = lane_id();
    float *ra = rows[ch][0], *rb = rows[ch][1];
    const int W2 = w + 2, H2 = h + 2;
    const int x0 = blockIdx.x * G::kOutCols, oy0 = blockIdx.y * G::kSegRows;
    const int ix = x0 - G::kPad + l;
    const bool col_ok = ix >= 0 && ix < (int)w;
    const int ox = x0 + l;
    const bool out_col = l < G::kOutCols && ox < W2;
    const bool own_col = l >= G::kPad - 1 && l < G::kPad - 1 + G::kOutCols;
    const uint32_t ixc = (uint32_t)min(max(ix, 0), (int)w - 1);
    const uint32_t pc = (ixc * 4u + (uint32_t)ch) * 4u;           // pred column byte offset (< 16 w, host-checked)
    const uint32_t gc = ixc * gt_channels + (uint32_t)ch;         // gt column element index
    float hq[WIN][5];
    double msum = 0.0, se = 0.0;
    struct Row {
        float a, b;
    };
    // marched row r -> (pred, gt) of the lane's column, zero outside the image; unconditional loads (clamped address
    // + select) three rows ahead of their use, wave-uniform row pointers
    auto fetch = [&](int r) {
        const int iy = oy0 - G::kPad + r;  // uniform
        const bool ok = col_ok && iy >= 0 && iy < (int)h;
        const uint32_t iyc = (uint32_t)min(max(iy, 0), (int)h - 1);
        const float *prow = pred + (size_t)iyc * w * 4u;
        const GT *grow = gt + (size_t)iyc * w * gt_channels;
        Row v;
        v.a = ld_off(prow, pc);
        v.b = ld_gt(grow, gc);
        v.a = ok ? v.a : 0.0f, v.b = ok ? v.b : 0.0f;
        return v;
    };
    Row pf[3] = {fetch(0), fetch(1), fetch(2)};  // ring turned by WIN % 3 once per unrolled body, as in k_ssim_forward
    for (int r0 = 0; r0 < G::kSegRows + WIN - 1; r0 += WIN) {
#pragma unroll
        for (int j = 0; j < WIN; j++) {
            const int r = r0 + j;
            const Row c = pf[j % 3];
            ra[l] = c.a, rb[l] = c.b;
            if (own_col && r >= G::kPad - 1 && r < G::kPad - 1 + G::kSegRows) {
                const float d = c.a - c.b;
                se += (double)(d * d);
            }
            pf[j % 3] = fetch(r + 3);
            wave_lds_sync();
            float sa, sb, saa, sbb, sab;
            {
                const float av = ra[l], bv = rb[l];
                const float ga = win.g[0] * av, gb = win.g[0] * bv;
                sa = ga, sb = gb, saa = ga * av, sbb = gb * bv, sab = ga * bv;
            }
#pragma unroll
            for (int k = 1; k < WIN; k++) {
                const float av = ra[l + k], bv = rb[l + k];
                const float ga = win.g[k] * av, gb = win.g[k] * bv;
                sa += ga, sb += gb, saa += ga * av, sbb += gb * bv, sab += ga * bv;
            }
            wave_lds_sync();
            hq[j][0] = sa, hq[j][1] = sb, hq[j][2] = saa, hq[j][3] = sbb, hq[j][4] = sab;
            const int oy = oy0 + r - (WIN - 1);
            if (r >= WIN - 1 && oy < H2 && out_col) {  // ring slot of marched row r - (WIN - 1) + k is (j + 1 + k) % WIN
                float v[5];
#pragma unroll
                for (int q = 0; q < 5; q++) v[q] = win.g[0] * hq[(j + 1) % WIN][q];
#pragma unroll
                for (int k = 1; k < WIN; k++) {
#pragma unroll
                    for (int q = 0; q < 5; q++) v[q] += win.g[k] * hq[(j + 1 + k) % WIN][q];
                }
                const float mx = v[0], my = v[1];
                const float mu_xx = mx * mx, mu_yy = my * my, mu_xy = mx * my;
                const float sxx = fmaxf(v[2] - mu_xx, 0.0f), syy = fmaxf(v[3] - mu_yy, 0.0f), sxy = v[4] - mu_xy;
                // the map's one division, IEEE as ssim.rs:98-99 (no derivative terms share it here)
                msum += (double)(((mu_xy * 2.0f + kC1) * (sxy * 2.0f + kC2)) /
                                 ((mu_xx + mu_yy + kC1) * (sxx + syy + kC2)));
            }
        }
        if constexpr (WIN % 3 == 1) {
            const Row t = pf[0];
            pf[0] = pf[1], pf[1] = pf[2], pf[2] = t;
        } else if constexpr (WIN % 3 == 2) {
            const Row t = pf[2];
            pf[2] = pf[1], pf[1] = pf[0], pf[0] = t;
        }
    }
    msum = tree_sum(msum), se = tree_sum(se);
    const uint32_t nwave = gridDim.x * gridDim.y * 3, wv = (blockIdx.y * gridDim.x + blockIdx.x) * 3 + ch;
    if (l == 0) partials[wv] = msum, partials[nwave + wv] = se;
}

// out = {mse, psnr, ssim}: fixed per-thread strides, fixed wave order.  PSNR in f32 from the f32 MSE as eval.rs:59
// (mse == 0 gives +inf).
__global__ __launch_bounds__(kFinalizeThreads) void k_eval_finalize(const double *__restrict__ partials, uint32_t nwave,
                                                                    double inv_rgb_count, double inv_map_count,
                                                                    float *__restrict__ out) {
    __shared__ double red[2][kFinalizeThreads / kWave];
    double ms = 0.0, se = 0.0;
    for (uint32_t i = threadIdx.x; i < nwave; i += kFinalizeThreads) ms += partials[i], se += partials[nwave + i];
    ms = tree_sum(ms), se = tree_sum(se);
    if (lane_id() == 0) red[0][threadIdx.x / kWave] = ms, red[1][threadIdx.x / kWave] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        ms = sum_waves_pairwise(red[0]);
        se = sum_waves_pairwise(red[1]);
        const float mse = (float)(se * inv_rgb_count);
        out[0] = mse;
        out[1] = logf(1.0f / mse) * 10.0f / kLn10;
        out[2] = (float)(ms * inv_map_count);
    }
}

// Upper bound of the metrics kernel's wave count over the supported windows (the workspace is sized without knowing
// the window): the narrowest column strip (window 15) times the shortest row segment (window 3), three waves a block.
inline size_t eval_waves_max(uint32_t w, uint32_t h) {
    return (size_t)ceil_div(w + 2, (uint32_t)Geo<kMaxWin>::kOutCols) * ceil_div(h + 2, (uint32_t)Geo<3>::kSegRows) * 3;
}

template <typename GT>
void launch_eval(const float *pred, const GT *gt, uint32_t gt_channels, uint32_t w, uint32_t h, uint32_t ssim_window,
                 double *partials, float *out, hipStream_t s) {
    const Window win = make_window((int)ssim_window);
    uint32_t nwave = 0;
    dispatch_window(ssim_window, [&](auto wc) {
        using G = Geo<wc()>;
        const dim3 grid(ceil_div(w + 2, (uint32_t)G::kOutCols), ceil_div(h + 2, (uint32_t)G::kSegRows));
        nwave = grid.x * grid.y * 3;
        hipLaunchKernelGGL((k_eval_metrics<wc(), GT>), grid, dim3(192), 0, s, pred, gt, gt_channels, w, h, win,
                           partials);
    });
    const double inv_rgb = 1.0 / (3.0 * (double)w * (double)h);
    const double inv_map = 1.0 / (3.0 * (double)(w + 2) * (double)(h + 2));
    hipLaunchKernelGGL(k_eval_finalize, dim3(1), dim3(kFinalizeThreads), 0, s, partials, nwave, inv_rgb, inv_map, out);
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_eval_workspace_size(uint32_t w, uint32_t h, size_t *bytes) {
    if (!bytes || w == 0 || h == 0) return BRUSH_ERR_INVALID_ARG;
    *bytes = align_up(2 * eval_waves_max(w, h) * sizeof(double), 256);
    return BRUSH_OK;
}

extern "C" int brush_eval_metrics(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t w, uint32_t h,
                                  uint32_t gt_channels, uint32_t ssim_window, float *out, void *workspace,
                                  size_t workspace_bytes, brush_stream_t stream) {
    if (!pred || !gt || !out || !workspace || w == 0 || h == 0) return BRUSH_ERR_INVALID_ARG;
    if (gt_dtype != BRUSH_EVAL_GT_U8 && gt_dtype != BRUSH_EVAL_GT_F32) return BRUSH_ERR_INVALID_ARG;
    if (gt_channels != 3 && gt_channels != 4) return BRUSH_ERR_INVALID_ARG;
    if (!window_ok(ssim_window)) return BRUSH_ERR_INVALID_ARG;        // odd sizes 3..15
    if (16ull * w * h >= (1ull << 32)) return BRUSH_ERR_INVALID_ARG;  // 32-bit byte offsets into pred (268 M pixels)
    size_t need = 0;
    brush_eval_workspace_size(w, h, &need);
    if (workspace_bytes < need) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partials = static_cast<double *>(workspace);
    if (gt_dtype == BRUSH_EVAL_GT_U8)
        launch_eval(pred, static_cast<const uint8_t *>(gt), gt_channels, w, h, ssim_window, partials, out, s);
    else
        launch_eval(pred, static_cast<const float *>(gt), gt_channels, w, h, ssim_window, partials, out, s);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
