// contribution.hip — per-splat rendered contribution: a replay of the forward's compositing walk over the tile lists a
// finished forward left behind, ending in per-splat reductions instead of a pixel store.  Kernel, launcher and ABI
// entry (brush_render_contributions) live here; the walk itself is replay_walk.hpp's.
//
// The reference has no such pass (its refinement prunes on sigmoid(raw_opacity) and scale alone, train.rs:395-470);
// the statistic is RadSplat's max blending weight and LightGaussian's summed weight, defined on the forward's own
// arithmetic (rasterize.wgsl:57-101).
//
// gfx950 layout: the walk's (replay_walk.hpp).  A staged record carries xy, conic, opacity and the splat's GLOBAL id;
// colour is not read.  Per walked (record, quadrant) that changed a pixel, the wave reduces
// max(fac), sum(rint(fac 2^24)), popcount(added), popcount(stopped) on the VALU (DPP) and lanes 0..2 send them to the
// splat's row with no-return integer atomics: max on the bits of a non-negative float and 64-bit adds, all of them
// order independent, so the result is bitwise repeatable in either aux mode.
#include "replay_walk.hpp"

namespace brush {
namespace {

// Max over the wave of an unsigned value, in every lane: the DPP ladder of wave_inclusive_scan (lanes without a source
// take 0, the identity), then lane 63 through the scalar unit.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = dpp_max_u32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_max_u32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_max_u32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_max_u32<0x118, 0xf>(v);  // row_shr:8
    v = dpp_max_u32<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
    v = dpp_max_u32<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3
    return wave_bcast(v, 63u);
}

// Per walked (record, quadrant) and lane, with the walk's hit and stop (replay_walk.hpp):
//   fac  = alpha * T where the forward added the entry, else 0
// and the splat's row g = global_from_compact_gid[cgid] receives
//   max_bits[g]    = max(max_bits[g], bits(max over lanes of fac))
//   counts[g][0]  += sum over lanes of (uint32) rint(fac 2^24)   (ties to even; at most 64 2^24 per record)
//   counts[g][1]  += popcount(hit),  counts[g][2] += popcount(stop)
// when hit | stop is set in any lane (a scalar branch).  Nothing else is written unless the self-check is on
// (out_img != nullptr): every inside pixel then compares the bits of its replayed 1 - T with out_img[pix].w and its
// last added entry with final_index[pix]; the wave adds the count of differing pixels to mismatch[0].
__global__ __launch_bounds__(kRasterThreads) void k_contribution_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const uint32_t *__restrict__ final_index, const float4 *__restrict__ out_img, uint32_t *__restrict__ max_bits,
    unsigned long long *__restrict__ counts, uint32_t *__restrict__ mismatch) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    BRUSH_REPLAY_WALK_STATE;
    uint32_t fin = 0;
    BRUSH_REPLAY_WALK_BEGIN(true, 6, (void)0, __uint_as_float(gid), 0.f)
    const float fac = hit ? alpha * T : 0.0f;
    BRUSH_REPLAY_WALK_DIE(false)
    BRUSH_REPLAY_WALK_ADD(fin = batch_start + t)
    const uint64_t hit_mask = ballot64(hit), stop_mask = ballot64(stop);
    if ((hit_mask | stop_mask) != 0ull) {
        const uint32_t fac_max = wave_max_u32(__float_as_uint(fac));  // fac >= 0: its bits order as it does
        const uint32_t q24 = wave_sum((uint32_t)__builtin_rintf(fac * kQ24));
        const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(b.z));
        if (g < n_splats) {
            if (lane < 3u) {
                const uint32_t v = lane == 0u   ? q24
                                   : lane == 1u ? (uint32_t)__builtin_popcountll(hit_mask)
                                                : (uint32_t)__builtin_popcountll(stop_mask);
                atomicAdd(counts + (size_t)g * 3u + lane, (unsigned long long)v);
            }
            if (lane == 0u) atomicMax(max_bits + g, fac_max);
        }
    }
    BRUSH_REPLAY_WALK_END
    if (out_img) {
        bool differs = false;
        if (inside) {
            const size_t pix = (size_t)px + (size_t)py * w;
            differs = __float_as_uint(1.0f - T) != __float_as_uint(out_img[pix].w) || fin != final_index[pix];
        }
        const uint32_t bad = (uint32_t)__builtin_popcountll(ballot64(differs));
        if (bad != 0u && lane == 0u) atomicAdd(mismatch, bad);
    }
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_render_contributions(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *out_img,
                                          uint32_t *max_bits, uint64_t *counts, uint32_t *mismatch, uint32_t n,
                                          brush_stream_t stream) {
    WalkArgs a;
    if (!max_bits || !counts || !walk_args(h_uniforms, h_aux, n, stream, a)) return BRUSH_ERR_INVALID_ARG;
    if ((out_img != nullptr) != (mismatch != nullptr) || (out_img && !h_aux->final_index)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(out_img, 16) || misaligned(max_bits, 4) || misaligned(counts, 8) || misaligned(mismatch, 4))
        return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    walk_launch(k_contribution_quad, a, h_aux->final_index, reinterpret_cast<const float4 *>(out_img), max_bits,
                reinterpret_cast<unsigned long long *>(counts), mismatch);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
