// error_score.hip — per-splat image error for error-driven densification (Rota Bulo et al., "Revising Densification in
// Gaussian Splatting", ECCV 2024): a per-pixel error map is distributed to the splats by their blending weights.
// Two entries (include/brush_hip.h):
//   brush_l1_error_map         k_l1_error_map<GT, CG, MASK>: one pixel per lane, the mean absolute colour difference of a
//                              render and its target, clamped to 1, 0 under a mask.
//   brush_render_error_scores  k_error_quad: a replay of a finished forward's compositing walk (the walk of
//                              contribution.hip, restated: DESIGN §9 lists the duplication as an open lever) that ends in
//                              one per-splat reduction, sum over pixels of rint(fac e 2^24), fac = alpha T the weight the
//                              forward added the splat with and e the pixel's error clamped to [0, 1].
//
// The reference has no such pass: its refinement densifies on the mean screen-space gradient norm (train.rs:448-449).
//
// gfx950 layout of k_error_quad: the forward's.  One wave64 per 8x8 quadrant, four waves per tile, the XCD-contiguous
// block remap, records staged per wave in LDS in batches of 64 and read back as wave-uniform broadcasts, quad_may_pass()
// skipping a (record, quadrant) on the scalar unit, no s_barrier, no LDS atomics.  Each lane reads its pixel's error once,
// in front of the walk.  Per walked (record, quadrant) that was added to a pixel the wave reduces the quantised product
// on the VALU (DPP) and lane 0 sends a non-zero sum to the splat's row with one no-return 64-bit integer add: order
// independent, so the result is bitwise repeatable in either aux mode.
#include "raster_common.hpp"
#include "ssim_dev.hpp"

namespace brush {
namespace {

// One staged record: 32 bytes, read back as wave-uniform broadcasts.
struct ErrorRec {
    float4 a;  // mean.x, mean.y, conic.x, conic.y
    float4 b;  // conic.z, opacity, global id (bits), -
};
static_assert(sizeof(ErrorRec) * kTilesPerBlock * kBatch == 8192, "one ErrorRec per wave and batch slot");

constexpr float kQ24 = 16777216.0f;  // the fixed point of the summed product: 2^24

// The forward's walk (k_rasterize_quad, float image) with the same expressions per pixel: sigma, power, alpha_u, the
// 0.999 clamp, the test `power <= 0 && alpha_u >= 1/255`, next_T, the `next_T <= 1e-4` stop and the NaN pixel centre
// after a stop, so that T evolves as it did in the forward.  It walks until every pixel of the wave has stopped or the
// list ends.
//
// Per lane, once: E = error_map[py * w + px] (0 outside a ragged frame), e = min(max(E, 0), 1): a NaN and every
// negative value are 0, everything above 1 is 1.  Per walked (record, quadrant) with the entry added in any lane, the
// splat's row g = global_from_compact_gid[cgid] receives
//   view_err[g] += sum over lanes of (uint32) rint((fac e) 2^24)   (ties to even; at most 64 2^24 per record)
// with fac = alpha T where the forward added the entry, else 0; a zero sum is not sent.
__global__ __launch_bounds__(kRasterThreads) void k_error_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ error_map, unsigned long long *__restrict__ view_err) {
    __shared__ ErrorRec lds_all[kTilesPerBlock][kBatch];
    const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    ErrorRec *lds = lds_all[q];
    const uint32_t tile_id = xcd_contiguous_block();
    if (tile_id >= num_tiles) return;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t qx0 = (tile_id % tbx) * kTileWidth + (q & 1u) * 8u, qy0 = (tile_id / tbx) * kTileWidth + (q >> 1) * 8u;
    if (qx0 >= w || qy0 >= h) return;  // quadrant entirely outside a ragged frame
    const uint32_t px = qx0 + (lane & 7u), py = qy0 + (lane >> 3);
    const float bx = (float)qx0 + 0.5f, by = (float)qy0 + 0.5f;
    const bool inside = px < w && py < h;
    const float pcy = (float)py + 0.5f;  // rasterize.wgsl:32
    float pcx = inside ? (float)px + 0.5f : __builtin_nanf("");
    // the map's row pitch is w, not the tile-padded width; w h < 2^28, so the index fits 32 bits
    const float E = inside ? error_map[py * w + px] : 0.0f;
    const float e = fminf(fmaxf(E, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0

    const uint64_t inside_mask = ballot64(inside);
    uint64_t live = inside_mask;
    uint32_t walked = 0;
    float T = 1.0f;
    const uint32_t nvis = min(*num_visible, n_splats);
    // a finished forward leaves r0 <= r1 <= min(num_intersections, cap); nothing beyond the list's capacity is read
    const uint32_t r0 = tile_bins[tile_id * 2], r1 = min(tile_bins[tile_id * 2 + 1], cap);
    for (uint32_t batch_start = r0; batch_start < r1 && live != 0ull; batch_start += kBatch) {
        const uint32_t remaining = min(kBatch, r1 - batch_start);
        bool may = false;
        float rec[6];
        uint32_t gid = kInvalid;
        if (lane < remaining) {
            const uint32_t cgid = gid_from_isect[batch_start + lane];
            if (cgid < nvis) {  // every entry of a finished forward's list is
                const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;
#pragma unroll
                for (int k = 0; k < 5; k++) rec[k] = p[k];
                rec[5] = p[8];  // the opacity the splat is drawn with (antialiased mode: already compensated)
                gid = global_from_compact[cgid];
                may = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], bx, by);
            }
        }
        uint64_t mask = ballot64(may);
        if (mask == 0ull) continue;
        wave_sync();  // the previous batch's broadcasts are done (LDS is in order per wave)
        if (may) {
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds[lane].b = make_float4(rec[4], rec[5], __uint_as_float(gid), 0.f);
        }
        wave_sync();
        while (mask != 0ull) {
            const uint32_t t = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const float4 a = lds[t].a;
            const float4 b = lds[t].b;
            const float opac = b.y;
            // rasterize.wgsl:80-99, the forward's association (rasterize.hip)
            const float dx = a.x - pcx, dy = a.y - pcy;
            const float sigma = fmaf(0.5f, fmaf(a.z * dx, dx, (b.x * dy) * dy), (a.w * dy) * dx);
            const float power = sigma * kNegLog2e;
            const float alpha_u = opac * __builtin_amdgcn_exp2f(power);
            const bool pass = power <= 0.0f && alpha_u >= 1.0f / 255.0f;  // never true for a stopped pixel (NaN)
            const float alpha = vmin(0.999f, alpha_u);
            const float next_T = T * (1.0f - alpha);
            const bool stop = pass && next_T <= 1e-4f;  // :88-91: stop WITHOUT adding this entry
            const bool hit = pass && !stop;
            const float fac = hit ? alpha * T : 0.0f;
            if (stop) pcx = __builtin_nanf("");
            if (hit) T = next_T;
            if (ballot64(hit) != 0ull) {
                // fac e: one f32 rounding; the scale by 2^24 is exact (fac e <= 1)
                const uint32_t q24 = wave_sum((uint32_t)__builtin_rintf((fac * e) * kQ24));
                const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(b.z));
                if (q24 != 0u && g < n_splats && lane == 0u) atomicAdd(view_err + g, (unsigned long long)q24);
            }
            // all pixels stopped?  one compare every 4th record, as the forward
            if ((++walked & 3u) == 0u) {
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;
                if (live == 0ull) break;
            }
        }
    }
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
    if (!h_uniforms || !h_aux || !error_map || !view_err) return BRUSH_ERR_INVALID_ARG;
    const BrushUniforms &u = *h_uniforms;
    const BrushAux &aux = *h_aux;
    const uint32_t w = u.img_size[0], h = u.img_size[1], tbx = u.tile_bounds[0], tby = u.tile_bounds[1];
    if (!checked_pixels(w, h) || tbx != ceil_div(w, kTileWidth) || tby != ceil_div(h, kTileWidth))
        return BRUSH_ERR_INVALID_ARG;
    if (!aux.projected_splats || !aux.tile_bins || !aux.compact_gid_from_isect || !aux.global_from_compact_gid ||
        !aux.num_visible || aux.max_intersects == 0)
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(error_map, 4) || misaligned(view_err, 8)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    const uint32_t tiles = tbx * tby;
    // one workgroup (4 quadrant waves) per tile; a multiple of 8 for the XCD remap
    hipLaunchKernelGGL(k_error_quad, dim3(ceil_div(tiles, 8u) * 8u), dim3(kRasterThreads), 0,
                       static_cast<hipStream_t>(stream), w, h, tbx, tiles, aux.compact_gid_from_isect, aux.tile_bins,
                       aux.max_intersects, aux.projected_splats, aux.global_from_compact_gid, aux.num_visible, n,
                       error_map, reinterpret_cast<unsigned long long *>(view_err));
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
