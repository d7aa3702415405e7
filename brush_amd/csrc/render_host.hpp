// render_host.hpp — what the host units behind the render entries share (render.hip, render_bwd.hip, view_records.hip,
// profiler.hip): the checks of (uniforms, aux), the frame the compositing launchers take, the optimizer arguments of
// the fused forms and the stage marks.  Host only, no kernel; every unit that includes it is built with FLAGS_render.
#pragma once
#include "internal.hpp"

namespace brush {

inline bool aux_det(const BrushAux &a) { return (a.flags & BRUSH_AUX_DETERMINISTIC) != 0; }

inline bool aux_ok(const BrushAux *a, bool need_final_index) {
    if (a && (a->flags & ~(BRUSH_AUX_DETERMINISTIC | BRUSH_AUX_ACCUM_ZEROED | BRUSH_AUX_ANTIALIASED)) != 0)
        return false;  // unknown flag bits
    if (a && aux_det(*a) && !a->isect_unsorted_pos) return false;
    return a && a->projected_splats && a->uniforms_buffer && a->num_intersections && a->num_visible &&
           (a->final_index || !need_final_index) && a->cum_tiles_hit && a->tile_bins &&
           a->compact_gid_from_isect && a->global_from_compact_gid && a->compact_from_global_gid && a->overflow;
}

inline bool uniforms_ok(const BrushUniforms *u) {
    if (!u || u->sh_degree > 4) return false;  // render.rs:44-52
    if (u->tile_bounds[0] != ceil_div(u->img_size[0], kTileWidth) ||
        u->tile_bounds[1] != ceil_div(u->img_size[1], kTileWidth))
        return false;  // render.rs:82-85
    return true;
}

// The frame of both compositing launches, from a checked (uniforms, aux).
inline RasterFrame raster_frame(const BrushUniforms &u, const BrushAux &aux) {
    return {u.img_size[0], u.img_size[1], u.tile_bounds[0], u.tile_bounds[1], aux.compact_gid_from_isect,
            aux.tile_bins, aux.projected_splats, aux.final_index};
}

// render_bwd.hip.  Shared by the fused backward+Adam forms and brush_reduce_view_records_adam: validates the optimizer
// arguments and fills the kernel-side struct.
bool fill_adam_fuse(const BrushAdamConfig *cfg, float *means, float *log_scales, float *rotation, float *raw_opacity,
                    float *sh, uint32_t n, float *moment1, float *moment2, float *next_quats_fed, float *grad_2d_accum,
                    float *xy_grad_counts, uint32_t w, uint32_t h, uint32_t sh_degree, AdamFuse *out);

// profiler.hip.  Opt-in stage timing: nothing happens unless a profiler is attached to the calling thread.
enum StagePass { kFwdPass = 0, kBwdPass = 1 };
// Records event `idx` of the pass on `s`: 0 = the pass starts, 1 + i = its stage i has been enqueued.
void mark_stage(StagePass pass, hipStream_t s, int idx);
// true: the attached profiler asks the pass to end behind `stage` (prefix timing)
bool stop_behind(int stage);

}  // namespace brush
