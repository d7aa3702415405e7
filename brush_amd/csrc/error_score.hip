// error_score.hip — per-splat image error for error-driven densification (Rota Bulo et al., "Revising Densification in
// Gaussian Splatting", ECCV 2024): a per-pixel error map is distributed to the splats by their blending weights.
// Two entries (include/brush_hip.h):
//   brush_l1_error_map         k_l1_error_map<GT, CG, MASK>: one pixel per lane, the mean absolute colour difference of a
//                              render and its target, clamped to 1, 0 under a mask.
//   brush_render_error_scores  k_error_quad: a replay of a finished forward's compositing walk (replay_walk.hpp) that
//                              ends in one per-splat reduction, sum over pixels of rint(fac e 2^24), fac = alpha T the
//                              weight the forward added the splat with and e the pixel's error clamped to [0, 1].
//
// The reference has no such pass: its refinement densifies on the mean screen-space gradient norm (train.rs:448-449).
//
// gfx950 layout of k_error_quad: the walk's.  Each lane reads its pixel's error once, in front of the walk.  Per walked
// (record, quadrant) that was added to a pixel the wave reduces the quantised product on the VALU (DPP) and lane 0 sends
// a non-zero sum to the splat's row with one no-return 64-bit integer add: order independent, so the result is bitwise
// repeatable in either aux mode.
#include "replay_walk.hpp"
#include "ssim_dev.hpp"

namespace brush {
namespace {

// Per lane, once, in front of the walk (replay_walk.hpp): E = error_map[py * w + px] (0 outside a ragged frame),
// e = min(max(E, 0), 1): a NaN and every negative value are 0, everything above 1 is 1.  Per walked (record, quadrant)
// with the entry added in any lane, the splat's row g = global_from_compact_gid[cgid] receives
//   view_err[g] += sum over lanes of (uint32) rint((fac e) 2^24)   (ties to even; at most 64 2^24 per record)
// with fac = alpha T where the forward added the entry, else 0; a zero sum is not sent.
__global__ __launch_bounds__(kRasterThreads) void k_error_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ error_map, unsigned long long *__restrict__ view_err) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    // the map's row pitch is w, not the tile-padded width; w h < 2^28, so the index fits 32 bits
    const float E = inside ? error_map[py * w + px] : 0.0f;
    const float e = fminf(fmaxf(E, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
    BRUSH_REPLAY_WALK_STATE;
    BRUSH_REPLAY_WALK_BEGIN(true, 6, (void)0, __uint_as_float(gid), 0.f)
    const float fac = hit ? alpha * T : 0.0f;
    BRUSH_REPLAY_WALK_DIE(false)
    BRUSH_REPLAY_WALK_ADD()
    if (ballot64(hit) != 0ull) {
        // fac e: one f32 rounding; the scale by 2^24 is exact (fac e <= 1)
        const uint32_t q24 = wave_sum((uint32_t)__builtin_rintf((fac * e) * kQ24));
        const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(b.z));
        if (q24 != 0u && g < n_splats && lane == 0u) atomicAdd(view_err + g, (unsigned long long)q24);
    }
    BRUSH_REPLAY_WALK_END
}

constexpr uint32_t kMapThreads = 256;

// out = min(((|dr| + |dg|) + |db|) * (1/3), 1) of the render's first three channels against the target's, +0 where a
// mask rules the pixel out (by selection).  No product feeds an add: contraction has nothing to fuse, and a float32
// restatement gives the same bits.  One pixel per lane over the whole grid (w h < 2^28 fits one).
template <typename GT, int CG, bool MASK>
__global__ __launch_bounds__(kMapThreads) void k_l1_error_map(const float4 *__restrict__ pred,
                                                              const GT *__restrict__ gt,
                                                              const uint8_t *__restrict__ mask, uint32_t npix,
                                                              float *__restrict__ out) {
    const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
    if (i >= npix) return;
    const float4 p = pred[i];
    const float dr = p.x - ld_gt(gt, i * (uint32_t)CG);
    const float dg = p.y - ld_gt(gt, i * (uint32_t)CG + 1u);
    const float db = p.z - ld_gt(gt, i * (uint32_t)CG + 2u);
    float v = fminf(((fabsf(dr) + fabsf(dg)) + fabsf(db)) * (1.0f / 3.0f), 1.0f);
    if constexpr (MASK) v = mask[i] != 0 ? v : 0.0f;
    out[i] = v;
}

template <typename GT, int CG>
void launch_map(const float *pred, const void *gt, const uint8_t *mask, uint32_t npix, float *out, hipStream_t s) {
    const dim3 grid(ceil_div(npix, kMapThreads)), block(kMapThreads);
    const float4 *p = reinterpret_cast<const float4 *>(pred);
    const GT *g = static_cast<const GT *>(gt);
    if (mask)
        hipLaunchKernelGGL((k_l1_error_map<GT, CG, true>), grid, block, 0, s, p, g, mask, npix, out);
    else
        hipLaunchKernelGGL((k_l1_error_map<GT, CG, false>), grid, block, 0, s, p, g, mask, npix, out);
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_l1_error_map(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t gt_channels,
                                  const uint8_t *mask, float *out, uint32_t w, uint32_t h, brush_stream_t stream) {
    const uint32_t npix = checked_pixels(w, h);
    if (!npix || !pred || !gt || !out) return BRUSH_ERR_INVALID_ARG;
    if (gt_dtype > BRUSH_EVAL_GT_F32 || (gt_channels != 3 && gt_channels != 4)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(out, 4) || (gt_dtype == BRUSH_EVAL_GT_F32 && misaligned(gt, 4)))
        return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool u8 = gt_dtype == BRUSH_EVAL_GT_U8;
    if (gt_channels == 3)
        u8 ? launch_map<uint8_t, 3>(pred, gt, mask, npix, out, s) : launch_map<float, 3>(pred, gt, mask, npix, out, s);
    else
        u8 ? launch_map<uint8_t, 4>(pred, gt, mask, npix, out, s) : launch_map<float, 4>(pred, gt, mask, npix, out, s);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_render_error_scores(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *error_map,
                                         uint64_t *view_err, uint32_t n, brush_stream_t stream) {
    WalkArgs a;
    if (!error_map || !view_err || !walk_args(h_uniforms, h_aux, n, stream, a)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(error_map, 4) || misaligned(view_err, 8)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    walk_launch(k_error_quad, a, error_map, reinterpret_cast<unsigned long long *>(view_err));
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
