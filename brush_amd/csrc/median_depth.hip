// median_depth.hip — median depth and the splat under every pixel: a replay of the forward's compositing walk over the
// tile lists a finished brush_render_forward_depth left behind, ending in a per-pixel PICK instead of a reduction.
// Kernel, launcher and ABI entry (brush_render_median_depth) live here; the walk itself is replay_walk.hpp's.
//
// The reference has no depth output at all; the definition is the one 2DGS, GOF, RaDe-GS and gsplat's 2DGS path fuse
// into their meshes: the depth of the splat at which the accumulated opacity 1 - T first reaches `level` (one half for
// the median), on the forward's own arithmetic (rasterize.wgsl:57-101).
//
// gfx950 layout: the walk's, with no atomics.  A staged record carries xy, conic, opacity, the splat's camera-space z
// (compact_depth) and its GLOBAL id; colour is not read.
// A pixel is live until it has crossed the level or stopped; the wave leaves the list as soon as no pixel is live, so an
// opaque scene walks the front of every list only.  Every pixel is written by exactly one lane, once: the result is
// bitwise repeatable.
#include "replay_walk.hpp"

namespace brush {
namespace {

// The median entry of a pixel is the first entry the walk (replay_walk.hpp) ADDED whose next_T is <= t_level
// (= 1.0f - level, rounded once on the host); an entry that stops the pixel is never the median.  A pixel that crossed
// or stopped takes a NaN centre, which fails every later alpha test: it keeps its first crossing and counts as not
// live.  The record's two own words are the splat's z and its global id.
//
// Every inside pixel writes out_depth[pix] = the bits of compact_depth[cgid] of its median entry (0.0f: none) and, with
// out_id, out_id[pix] = that entry's global id (-1: none); n_splats == 0 reads no list at all.
__global__ __launch_bounds__(kRasterThreads) void k_median_depth_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ compact_depth, float t_level, float *__restrict__ out_depth,
    int32_t *__restrict__ out_id) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    BRUSH_REPLAY_WALK_STATE;
    float med_z = 0.0f;
    uint32_t med_id = 0xFFFFFFFFu;
    BRUSH_REPLAY_WALK_BEGIN(n_splats != 0u, 7, rec[6] = compact_depth[cgid], rec[6], __uint_as_float(gid))
    const bool cross = hit && next_T <= t_level;
    BRUSH_REPLAY_WALK_ADD()
    if (cross) {
        med_z = b.z;
        med_id = __float_as_uint(b.w);
    }
    BRUSH_REPLAY_WALK_DIE(cross)  // the pixel keeps its first crossing
    BRUSH_REPLAY_WALK_END
    if (inside) {
        const size_t pix = (size_t)px + (size_t)py * w;
        out_depth[pix] = med_z;
        if (out_id) out_id[pix] = (int32_t)med_id;
    }
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_render_median_depth(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                         const float *compact_depth, float level, float *out_depth, int32_t *out_id,
                                         uint32_t n, brush_stream_t stream) {
    WalkArgs a;
    if (!compact_depth || !out_depth || !walk_args(h_uniforms, h_aux, n, stream, a)) return BRUSH_ERR_INVALID_ARG;
    if (!(level > 0.0f && level < 1.0f)) return BRUSH_ERR_INVALID_ARG;  // (a NaN fails too)
    if (misaligned(compact_depth, 4) || misaligned(out_depth, 4) || misaligned(out_id, 4)) return BRUSH_ERR_INVALID_ARG;
    const float t_level = 1.0f - level;  // once, in float32: what every pixel compares its next_T with
    // n == 0 launches too: every pixel is written on every call
    walk_launch(k_median_depth_quad, a, compact_depth, t_level, out_depth, out_id);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
