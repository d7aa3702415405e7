// internal.hpp — host-side launch functions, one group per translation unit.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "lazy_sh.hpp"

namespace brush {

struct ViewParams;

// Device work queue of (splat, tile-chunk) items for the balanced tile walks (tile_walk.hpp: WalkQueue is the
// kernels' typed view of it, and states what the count pass leaves here for the emit pass).
struct WalkWs {
    uint32_t *counter;      // [1], zeroed by the cull kernel
    uint32_t *items;        // [capacity * 2] (compact gid, chunk index)
    uint32_t *chunk_count;  // [capacity]
    uint32_t *chunk_mask;   // one 64-bit hit mask per item: [capacity * 2] are used; the workspace carves
                            //     [capacity * 8] (brush_fwd_workspace_size is observable)
    uint32_t *slot_of;      // [N]
    uint32_t *inline_mask;  // [N * 2] (64-bit hit mask per inline splat)
    uint32_t capacity;
};

// project.hip
size_t cull_block_count(uint32_t n);
hipError_t launch_project_cull(const ViewParams &vp, const BrushUniforms &u, const BrushAux &aux,
                               uint32_t num_tiles, const float *means, const float *log_scales,
                               const float *quats, const float *sh, const float *raw_opac, float *proj_global,
                               uint32_t *key_all, uint32_t *block_counts, uint32_t *keys,
                               uint32_t *gids, uint32_t *bin_edges /* [num_tiles][2], zeroed here */,
                               const WalkWs &walk, const LazySh &lazy /* BrushAux::lazy_sh, or off */, hipStream_t s);

// tile_count.hip (tile_walk.hpp)
hipError_t launch_project_visible(const ViewParams &vp, const float *proj_global, const uint32_t *num_visible,
                                  uint32_t *global_from_compact, uint32_t *compact_from_global, float *projected,
                                  uint32_t *tiles_hit, const WalkWs &walk, hipStream_t s);

// tile_emit.hip (tile_walk.hpp)
hipError_t launch_map_intersects(const ViewParams &vp, const float *projected, const uint32_t *cum_tiles_hit,
                                 const uint32_t *num_visible, uint32_t cap, uint32_t *tile_ids, uint32_t *gids,
                                 const WalkWs &walk, hipStream_t s);
// perm / gid_unsorted / gid_sorted: deterministic mode only (nullptr otherwise), see k_tile_bin_edges.
hipError_t launch_tile_bin_edges(const uint32_t *sorted_tile_ids, const uint32_t *num_intersections,
                                 uint32_t cap, uint32_t *tile_bins, const uint32_t *perm,
                                 const uint32_t *gid_unsorted, uint32_t *gid_sorted, hipStream_t s);

// tile_sort.hip (sort_common.hpp)
// The tile sort: sort_launch's arguments with edge_keys = num_tiles, same outputs and workspace.  In the default mode
// (compact gids as values, keys_out == nullptr, edges given), with the fused launch shape and a tile id of 9 to 16
// significant bits (257 to 65 536 tiles) it is three launches: one count + scatter pair on the id's top 8 bits, then
// one workgroup per bucket orders its bucket by the bits below and stores the bin edges of its tiles.  Anything else
// runs sort_launch.
hipError_t tile_sort_launch(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                            const uint32_t *d_n, uint32_t max_n, uint32_t bits, void *ws, hipStream_t s, uint32_t *edges,
                            uint32_t num_tiles);

// rasterize.hip (forward), rasterize_bwd.hip (backward, zero-fill); raster_common.hpp, raster_zero_fill.hpp
// What both compositing launches take from (uniforms, aux): the frame and the tile lists of one render
// (render_host.hpp: raster_frame).  The forward writes tile_bins and final_index, the backward reads them.
struct RasterFrame {
    uint32_t w, h, tbx, tby;
    const uint32_t *compact_gid_from_isect;
    uint32_t *tile_bins;
    const float *projected;
    uint32_t *final_index;
};
// The forward's image and its optional depth outputs (brush_render_forward_depth: both or neither, float image only).
struct RasterOut {
    int raster_u32;              // img: packed rgba8 words, rows u32_pitch pixels apart; else [h][w] float4
    uint32_t u32_pitch;
    void *img;
    const float *compact_depth;  // [n] z, compact order
    float *out_depth;            // [h][w]: accumulated depth
};
// bin_edges != nullptr: the tile sort's last pass left (~start, end) per tile there (sort_launch: edges) instead of a
// GetTileBinEdges launch; the kernel decodes them and writes tile_bins (every tile) for the aux / the backward.
// zero_rows: nullable, [n][kCompactStride], the first *num_visible rows are zeroed (BrushAux::bwd_accum).
hipError_t launch_rasterize(const RasterFrame &f, const RasterOut &out, const uint32_t *bin_edges, float *zero_rows,
                            const uint32_t *num_visible, uint32_t n, hipStream_t s);
// Zero-fill the compositing backward carries beside its arithmetic: the dense gradient arrays of the same backward
// (render.rs:539-547,573-575 zero-fills them with separate launches).  The kernel is bound by VALU issue and moves
// little memory, so its waves store the zeros in passing, one KiB (64 lanes x 16 B) per wave instruction, paced over
// the records they walk; the parameter VJP kernel behind it then writes the visible splats' rows only.
constexpr uint32_t kFillSegs = 6;
struct ZeroFill {
    float *base[kFillSegs];                // 16-byte aligned array starts
    uint32_t full[kFillSegs];              // whole 16-byte chunks of the array
    uint32_t tail[kFillSegs];              // floats behind them (0..3)
    uint32_t first_block[kFillSegs + 1];   // cumulative KiB blocks (the last block of an array may be partial)
    __host__ __device__ bool active() const { return first_block[kFillSegs] != 0u; }
};
// Fills `zf` for the given arrays (nullptr / 0 floats: skipped).  False — and an inactive `zf` — when an array is not
// 16-byte aligned or too large for 32-bit chunk counts: the caller then keeps the zeros in the VJP kernel.
bool make_zero_fill(ZeroFill *zf, float *const *arrays, const size_t *floats, uint32_t count);
// What the compositing backward reads and adds to; {}: no depth term, default mode.
struct RasterGrads {
    const float *out_img, *v_out;
    float *v_compact;
    // depth term (brush_render_backward_depth), both or neither
    const float *compact_depth;  // [n] z, compact order
    const float *v_depth;        // [h][w]: gradient of the accumulated depth
    // deterministic mode, both or neither
    const uint32_t *unsorted_pos;
    float *rows;                 // [max_intersects][kCompactStride]
};
hipError_t launch_rasterize_backward(const RasterFrame &f, const RasterGrads &g, const ZeroFill &fill, hipStream_t s);

// project_bwd.hip, view_records.hip
// Optimizer state for the fused backward + Adam form (brush_render_backward_adam).
struct AdamFuse {
    float *means, *log_scales, *rotation, *raw_opac, *sh;  // parameters, updated in place
    float *m1, *m2;                                        // [means 3N | log_scales 3N | quats 4N | raw_opac N | sh 3CN]
    float lr[5];                                           // means, log_scales, rotation, raw_opac, sh (dc)
    float sh_lerp, beta1, beta2, eps, rbc1, rbc2;          // rbc = 1 / (1 - beta^time), see adam_stepped()
    uint32_t quat_vjp, vec_ok;
    float *norm_rot_out;                                   // optional [N,4]: updated rotation / |rotation| (next forward's input)
    float *grad_2d_accum, *xy_grad_counts;                 // optional [N]: refinement statistics (train.rs:284-316)
    float half_w, half_h;
    float stat_scale;                                      // BrushAdamConfig::xy_stat_scale (0 -> 1)
    LazySh lazy;                                           // BrushAdamConfig::lazy_sh (off: every SH block is stepped)
};
hipError_t launch_lazy_sh_flush(const LazySh &lazy, float *sh, uint32_t n, uint32_t row_floats, hipStream_t s);
// Deterministic mode: where a splat's compact-order sums come from (see det_sums.hpp); partials == nullptr
// selects the default atomic accumulators in v_compact.
struct DetSumsArgs {
    const uint32_t *cum_tiles_hit = nullptr;
    const uint32_t *num_intersections = nullptr;
    const float *partials = nullptr;
    uint32_t cap = 0;
};
hipError_t launch_sum_isect_rows(const float *rows, const uint32_t *num_intersections, const uint32_t *cum_tiles_hit,
                                 uint32_t cap, float *v_compact, float *partials, hipStream_t s);
// Antialiased mode (BRUSH_AUX_ANTIALIASED) in the kernels' template arguments: the per-splat kernels that differ in that
// mode take DM = SH degree | kAaMode where they took the degree, so the instantiations without it are unchanged.
constexpr int kDegMask = 7, kAaMode = 8;
// Runtime (sh_degree, antialiased) -> compile-time template argument of a kernel launch: f receives an IntC<...>, whose
// `dm()` is the argument.  dispatch_degree: degrees 0-4 (anything above: 4); dispatch_dm adds the kAaMode bit;
// dispatch_dm_lazy, for the deferred-SH forms (rows of whole 16-byte chunks): degrees 1 and 3 only (anything else: 3).
template <int D> using IntC = std::integral_constant<int, D>;
template <int D, typename F>
void dispatch_aa(bool antialiased, F &&f) { antialiased ? f(IntC<D | kAaMode>{}) : f(IntC<D>{}); }
template <typename F>
void dispatch_degree(uint32_t sh_degree, F &&f) {
    switch (sh_degree) {
        case 0: return f(IntC<0>{});
        case 1: return f(IntC<1>{});
        case 2: return f(IntC<2>{});
        case 3: return f(IntC<3>{});
        default: return f(IntC<4>{});
    }
}
template <typename F>
void dispatch_dm(uint32_t sh_degree, bool antialiased, F &&f) {
    dispatch_degree(sh_degree, [&](auto deg) { dispatch_aa<deg()>(antialiased, f); });
}
template <typename F>
void dispatch_dm_lazy(uint32_t sh_degree, bool antialiased, F &&f) {
    sh_degree == 1 ? dispatch_aa<1>(antialiased, f) : dispatch_aa<3>(antialiased, f);
}
hipError_t launch_project_backward(const ViewParams &vp, const float *means, const float *log_scales,
                                   const float *quats, const float *raw_opac,
                                   const uint32_t *compact_from_global, const float *v_compact,
                                   float *v_means, float *v_xy,
                                   float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                   const AdamFuse *adam, const DetSumsArgs &det,
                                   bool prezeroed /* dense form only: the arrays are already zero (ZeroFill), the
                                   visible splats' rows alone are written */,
                                   hipStream_t s, bool antialiased = false /* BRUSH_AUX_ANTIALIASED */);
// View-sharded data parallelism (view_records.hip): per-view 64-byte gradient records, their index by global id and
// the deterministic per-splat sum over views (dense arrays, or straight into the Adam update when adam != nullptr).
hipError_t launch_project_backward_records(const ViewParams &vp, const float *means, const float *log_scales,
                                           const float *quats, const float *raw_opac, const uint32_t *num_visible,
                                           const uint32_t *global_from_compact, const float *v_compact,
                                           float *records, uint32_t max_rows, const DetSumsArgs &det, hipStream_t s);
hipError_t launch_reduce_view_records(const float *records, uint32_t num_views, uint32_t rows_per_view,
                                      const uint32_t *view_rows, const uint32_t *view_offsets /* nullable */,
                                      const float *campos, const float *means, uint32_t n,
                                      uint32_t sh_degree, uint32_t *index, float *v_means, float *v_scales,
                                      float *v_quats, float *v_sh, float *v_opac, const AdamFuse *adam, hipStream_t s);
// brush_render_backward_depth: v_means[g] += v_z viewmat row 2 for every visible splat, v_z = word 9 of its compact
// row (default mode) or the fixed-order sum of word 10 of its intersection rows (deterministic mode).  Runs after
// launch_sum_isect_rows / launch_project_backward.
hipError_t launch_sum_isect_depth(const float *rows, const uint32_t *num_intersections, const uint32_t *cum_tiles_hit,
                                  uint32_t cap, float *v_compact, float *partials, hipStream_t s);
hipError_t launch_depth_means_grad(const ViewParams &vp, const uint32_t *num_visible, uint32_t n,
                                   const uint32_t *global_from_compact, const float *v_compact, const DetSumsArgs &det,
                                   float *v_means, hipStream_t s);
hipError_t launch_zero_compact_grads(const uint32_t *num_visible, uint32_t n, float *v_compact, hipStream_t s);

// pose_grad.hip
// v_viewmat[12] (row-major 3x4, [d L / d W row r | d L / d t[r]]) from the compact-order sums of the visible splats, in
// float64 partial sums with a fixed order; every word is written.  Runs after the compositing backward and BEFORE
// launch_project_backward: the fused Adam forms overwrite `means` in place.  pose_ws: pose_grad_workspace_bytes(n).
size_t pose_grad_workspace_bytes(uint32_t n);
hipError_t launch_view_grad(const ViewParams &vp, const float *means, const float *log_scales, const float *quats,
                            const float *raw_opac, const uint32_t *num_visible, uint32_t n,
                            const uint32_t *global_from_compact, const float *v_compact, const DetSumsArgs &det,
                            bool has_depth /* v_z of brush_render_backward_depth is present */, bool antialiased,
                            void *pose_ws, float *v_viewmat, hipStream_t s);

// distortion.hip
// The gradient replay of the depth-distortion term: ADDS its per-record VJP into the compact rows (words 0-4, 8, 9) of a
// default-mode backward, between the compositing backward and launch_project_backward.  Validates its own arguments and
// returns a BrushStatus (BRUSH_ERR_INVALID_ARG in deterministic mode).  distortion_args_ok: the same checks without the
// launch, for an entry that has other launches in front of this one.
bool distortion_args_ok(const BrushAux *h_aux, const BrushDistortion *cfg, const float *stats, const float *v_distortion);
int launch_distortion_grad(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *compact_depth,
                           const BrushDistortion *cfg, const float *stats, const float *v_distortion, uint32_t n,
                           float *v_compact, brush_stream_t stream);

}  // namespace brush
