// render.hip — host orchestration of the forward pass behind the C ABI, and the library's version, status strings and
// last-HIP-error slot.  (The backward: render_bwd.hip.  The stage profiler: profiler.hip.)
//
// Replaces render_forward (crates/brush-render/src/render.rs:55-323).  Like the reference it only enqueues work on
// the caller's stream and never reads a count back to the host; unlike the reference it
// performs no allocation (the caller passes one workspace) and needs no indirect-dispatch
// helper kernels (kernels read the device-side counts and grid-stride).
#include <stdlib.h>

#include "render_host.hpp"
#include "splat_math.hpp"

namespace brush {

static thread_local int g_last_hip_error = 0;
void set_last_hip_error(int e) { g_last_hip_error = e; }

namespace {

struct FwdWs {
    uint32_t *key_all;       // [N] depth bits or 0xFFFFFFFF
    uint32_t *block_counts;  // [ceil(N/256)]
    uint32_t *pre_keys;      // [N] compacted, unsorted
    uint32_t *pre_gids;      // [N]
    uint32_t *sorted_keys;   // [N]
    uint32_t *tiles_hit;     // [N]
    float *proj_global;      // [N][12] projected record staged by the cull kernel under the global id
    uint32_t *tile_unsorted; // [cap]
    uint32_t *gid_unsorted;  // [cap]
    uint32_t *tile_sorted;   // [cap]
    uint32_t *bin_edges;     // [tiles][2] (~start, end) accumulated by the tile sort's last pass
    void *scan_ws;
    void *sort_ws;           // sized for max(N, cap)
    WalkWs walk;             // (splat, chunk) queue of the tile walks
    size_t bytes;
};

FwdWs carve_fwd(void *ws, uint32_t n, uint32_t cap, uint32_t num_tiles) {
    FwdWs f;
    Carver c(ws);
    const size_t nn = n ? n : 1, cc = cap ? cap : 1;
    f.key_all = c.take<uint32_t>(nn);
    f.block_counts = c.take<uint32_t>(cull_block_count(n));
    f.pre_keys = c.take<uint32_t>(nn);
    f.pre_gids = c.take<uint32_t>(nn);
    f.sorted_keys = c.take<uint32_t>(nn);
    f.tiles_hit = c.take<uint32_t>(nn);
    f.proj_global = c.take<float>(nn * 12);
    f.tile_unsorted = c.take<uint32_t>(cc);
    f.gid_unsorted = c.take<uint32_t>(cc);
    f.tile_sorted = c.take<uint32_t>(cc);
    f.bin_edges = c.take<uint32_t>((size_t)(num_tiles ? num_tiles : 1) * 2);
    f.scan_ws = c.take<char>(scan_workspace_bytes(n));
    f.sort_ws = c.take<char>(sort_workspace_bytes(n > cap ? n : cap));
    f.walk.capacity = (uint32_t)nn;
    f.walk.counter = c.take<uint32_t>(1);
    f.walk.items = c.take<uint32_t>(nn * 2);
    f.walk.chunk_count = c.take<uint32_t>(nn);
    f.walk.chunk_mask = c.take<uint32_t>(nn * 8);
    f.walk.slot_of = c.take<uint32_t>(nn);
    f.walk.inline_mask = c.take<uint32_t>(nn * 2);
    f.bytes = c.bytes();
    return f;
}

// One forward call as its entry describes it, filled by field name ({}: everything absent).
struct ForwardCall {
    const BrushUniforms *uniforms;
    const float *means, *log_scales, *quats, *sh_coeffs, *raw_opacity;
    uint32_t n;
    int raster_u32;      // out_img holds packed rgba8 words, rows u32_pitch pixels apart (0: the width) ...
    uint32_t u32_pitch;
    void *out_img;       // ... or [h][w] float4
    const BrushAux *aux;
    void *workspace;
    size_t workspace_bytes;
    brush_stream_t stream;
    // optional depth outputs (float image only), both there or both absent
    float *out_depth;      // [h][w] accumulated depth
    float *compact_depth;  // [n] camera-space z of the visible splats, compact order
};

}  // namespace
}  // namespace brush

using namespace brush;

#ifndef BRUSH_BUILD_TAG
#define BRUSH_BUILD_TAG ""  // the test / development twins of the library name themselves here (Makefile)
#endif
extern "C" const char *brush_version(void) { return "brush_amd 0.4.0 (gfx950)" BRUSH_BUILD_TAG; }

extern "C" const char *brush_status_string(int status) {
    switch (status) {
        case BRUSH_OK: return "ok";
        case BRUSH_ERR_INVALID_ARG: return "invalid argument";
        case BRUSH_ERR_WORKSPACE_SMALL: return "workspace too small";
        case BRUSH_ERR_HIP: return "HIP runtime error";
        case BRUSH_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

extern "C" int brush_last_hip_error(void) { return g_last_hip_error; }

extern "C" uint32_t brush_default_max_intersects(uint32_t n, uint32_t w, uint32_t h) {
    const uint64_t tiles = (uint64_t)ceil_div(w, kTileWidth) * ceil_div(h, kTileWidth);
    uint64_t m = (uint64_t)n * tiles;  // render.rs:204-206 (saturating_mul)
    if (m > 128ull * 65535ull) m = 128ull * 65535ull;
    return m ? (uint32_t)m : 1u;
}

extern "C" int brush_fwd_workspace_size(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree,
                                        uint32_t max_intersects, size_t *bytes) {
    if (!bytes || sh_degree > 4) return BRUSH_ERR_INVALID_ARG;
    *bytes = carve_fwd(nullptr, n, max_intersects, ceil_div(w, kTileWidth) * ceil_div(h, kTileWidth)).bytes;
    return BRUSH_OK;
}

// Host-side default only (not cached, not read by any render entry point): see brush_hip.h.
extern "C" int brush_deterministic(void) {
    const char *e = getenv("BRUSH_DETERMINISTIC");
    return (e && e[0] == '1') ? 1 : 0;
}

// The checks every forward shares (an entry makes its own first: all refusals come before any HIP call, and an invalid
// argument is reported whatever the workspace's size; a refused BrushAux::lazy_sh alone comes behind the size), then the
// stage sequence.
static int render_forward_impl(const ForwardCall &c) {
    if (!uniforms_ok(c.uniforms) || !aux_ok(c.aux, !c.raster_u32) || !c.out_img || !c.workspace)
        return BRUSH_ERR_INVALID_ARG;
    if ((c.out_depth != nullptr) != (c.compact_depth != nullptr) || (c.out_depth && c.raster_u32))
        return BRUSH_ERR_INVALID_ARG;
    const uint32_t n = c.n;
    if (n > 0 && (!c.means || !c.log_scales || !c.quats || !c.sh_coeffs || !c.raw_opacity)) return BRUSH_ERR_INVALID_ARG;
    const BrushAux &aux = *c.aux;
    const uint32_t cap = aux.max_intersects;
    if (cap == 0) return BRUSH_ERR_INVALID_ARG;
    const FwdWs ws = carve_fwd(c.workspace, n, cap, c.uniforms->tile_bounds[0] * c.uniforms->tile_bounds[1]);
    if (c.workspace_bytes < ws.bytes) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(c.stream);

    BrushUniforms u = *c.uniforms;
    u.num_visible = 0;
    u.total_splats = n;
    u.padding = 0;
    const ViewParams vp = make_view_params(u, n);
    const uint32_t num_tiles = u.tile_bounds[0] * u.tile_bounds[1];

    LazySh lazy;  // deferred Adam of the SH block (BrushAux::lazy_sh): colours from the caught-up coefficients
    if (!make_lazy_sh(aux.lazy_sh, u.sh_degree, &lazy)) return BRUSH_ERR_INVALID_ARG;
    mark_stage(kFwdPass, s, 0);
    // uniforms buffer, counters, tile_bins = 0; ProjectSplats + order-preserving compaction
    // (render.rs:102-142)
    BRUSH_HIP_CHECK(launch_project_cull(vp, u, aux, num_tiles, c.means, c.log_scales, c.quats, c.sh_coeffs,
                                        c.raw_opacity, ws.proj_global, ws.key_all, ws.block_counts, ws.pre_keys,
                                        ws.pre_gids, ws.bin_edges, ws.walk, lazy, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_PROJECT_CULL);
    if (stop_behind(BRUSH_STAGE_PROJECT_CULL)) return BRUSH_OK;
    // DepthSort: keys = f32 depth bits, all 32 bits (render.rs:151-156).  With a depth output the sorted keys go to
    // the caller's compact_depth: camera-space z of every visible splat in compact order, read by the compositing
    // kernels of the forward and of the backward.
    BRUSH_HIP_CHECK(depth_sort_launch(ws.pre_keys, ws.pre_gids,
                                      c.compact_depth ? reinterpret_cast<uint32_t *>(c.compact_depth) : ws.sorted_keys,
                                      aux.global_from_compact_gid, aux.num_visible, n, ws.sort_ws, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_DEPTH_SORT);
    if (stop_behind(BRUSH_STAGE_DEPTH_SORT)) return BRUSH_OK;
    // ProjectVisible (render.rs:161-184)
    BRUSH_HIP_CHECK(launch_project_visible(vp, ws.proj_global, aux.num_visible, aux.global_from_compact_gid,
                                           aux.compact_from_global_gid, aux.projected_splats, ws.tiles_hit,
                                           ws.walk, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_PROJECT_VISIBLE);
    if (stop_behind(BRUSH_STAGE_PROJECT_VISIBLE)) return BRUSH_OK;
    // PrefixSum over all N, tail treated as 0 (render.rs:186-192); total -> num_intersections
    BRUSH_HIP_CHECK(scan_launch(ws.tiles_hit, aux.cum_tiles_hit, n, aux.num_visible, aux.num_intersections, cap,
                                aux.overflow, ws.scan_ws, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_PREFIX_SUM);
    if (stop_behind(BRUSH_STAGE_PREFIX_SUM)) return BRUSH_OK;
    // MapGaussiansToIntersect (render.rs:211-223)
    BRUSH_HIP_CHECK(launch_map_intersects(vp, aux.projected_splats, aux.cum_tiles_hit, aux.num_visible, cap,
                                          ws.tile_unsorted, ws.gid_unsorted, ws.walk, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_MAP_INTERSECTS);
    if (stop_behind(BRUSH_STAGE_MAP_INTERSECTS)) return BRUSH_OK;
    // Tile sort on bits = 32 - clz(num_tiles) (render.rs:227-237)
    uint32_t bits = 0;
    while (bits < 32 && (num_tiles >> bits) != 0) bits++;
    // Deterministic mode: the sort carries the pre-sort positions (aux.isect_unsorted_pos) and the gids follow by
    // a gather in the bin-edge kernel.  Default mode: GetTileBinEdges (render.rs:239-262) has no launch of its own —
    // the sort's last pass sees every key next to its neighbours in final order and records the edges of the runs
    // (ws.bin_edges), the compositing kernel decodes them and writes aux.tile_bins.
    const bool det = aux_det(aux);
    // The sorted tile ids are read by nobody once the edges come out of the sort: not written in the default mode.  (With
    // three or more passes, i.e. more than 65 535 tiles, the ping-pong also routes an intermediate pass through the
    // output buffer, so it is kept then.)
    const bool drop_keys = !det && bits <= 16;
    // 257 to 65 535 tiles in the default mode with the fused sort shape: one scatter into tile-range buckets, the bins
    // are ordered and their edges stored by the workgroup that finishes a bucket.
    BRUSH_HIP_CHECK(tile_sort_launch(ws.tile_unsorted, det ? nullptr : ws.gid_unsorted,
                                     drop_keys ? nullptr : ws.tile_sorted,
                                     det ? aux.isect_unsorted_pos : aux.compact_gid_from_isect, aux.num_intersections,
                                     cap, bits, ws.sort_ws, s, det ? nullptr : ws.bin_edges, num_tiles));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_TILE_SORT);
    if (stop_behind(BRUSH_STAGE_TILE_SORT)) return BRUSH_OK;
    if (det) {
        BRUSH_HIP_CHECK(launch_tile_bin_edges(ws.tile_sorted, aux.num_intersections, cap, aux.tile_bins,
                                              aux.isect_unsorted_pos, ws.gid_unsorted, aux.compact_gid_from_isect, s));
        mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_TILE_BINS);
    }  // default mode: the stage has no launch (the edges come out of the tile sort), so it records no event either
    if (stop_behind(BRUSH_STAGE_TILE_BINS)) return BRUSH_OK;
    // Rasterize (render.rs:267-307)
    // (default mode, aux.bwd_accum given: the kernel also zeroes the backward's accumulator rows, BRUSH_AUX_ACCUM_ZEROED)
    RasterOut out{};
    out.raster_u32 = c.raster_u32, out.u32_pitch = c.u32_pitch ? c.u32_pitch : u.img_size[0], out.img = c.out_img;
    out.compact_depth = c.compact_depth, out.out_depth = c.out_depth;
    BRUSH_HIP_CHECK(launch_rasterize(raster_frame(u, aux), out, det ? nullptr : ws.bin_edges,
                                     det ? nullptr : aux.bwd_accum, aux.num_visible, n, s));
    mark_stage(kFwdPass, s, 1 + BRUSH_STAGE_RASTERIZE);
    return BRUSH_OK;
}

extern "C" int brush_render_forward(const BrushUniforms *h_uniforms, const float *means, const float *log_scales,
                                    const float *quats, const float *sh_coeffs, const float *raw_opacity,
                                    uint32_t n, int raster_u32, void *out_img, const BrushAux *h_aux,
                                    void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    ForwardCall c{};
    c.uniforms = h_uniforms, c.aux = h_aux, c.means = means, c.log_scales = log_scales, c.quats = quats;
    c.sh_coeffs = sh_coeffs, c.raw_opacity = raw_opacity, c.n = n, c.raster_u32 = raster_u32, c.out_img = out_img;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return render_forward_impl(c);
}

extern "C" int brush_render_forward_depth(const BrushUniforms *h_uniforms, const float *means,
                                          const float *log_scales, const float *quats, const float *sh_coeffs,
                                          const float *raw_opacity, uint32_t n, float *out_img, float *out_depth,
                                          float *compact_depth, const BrushAux *h_aux, void *workspace,
                                          size_t workspace_bytes, brush_stream_t stream) {
    if (!out_depth || !compact_depth) return BRUSH_ERR_INVALID_ARG;
    ForwardCall c{};
    c.uniforms = h_uniforms, c.aux = h_aux, c.means = means, c.log_scales = log_scales, c.quats = quats;
    c.sh_coeffs = sh_coeffs, c.raw_opacity = raw_opacity, c.n = n, c.out_img = out_img;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.out_depth = out_depth, c.compact_depth = compact_depth;
    return render_forward_impl(c);
}

extern "C" int brush_render_forward_rgba8(const BrushUniforms *h_uniforms, const float *means,
                                          const float *log_scales, const float *quats, const float *sh_coeffs,
                                          const float *raw_opacity, uint32_t n, uint32_t *out_img,
                                          uint32_t row_pitch_pixels, const BrushAux *h_aux, void *workspace,
                                          size_t workspace_bytes, brush_stream_t stream) {
    if (!h_uniforms || row_pitch_pixels < h_uniforms->img_size[0]) return BRUSH_ERR_INVALID_ARG;
    ForwardCall c{};
    c.uniforms = h_uniforms, c.aux = h_aux, c.means = means, c.log_scales = log_scales, c.quats = quats;
    c.sh_coeffs = sh_coeffs, c.raw_opacity = raw_opacity, c.n = n, c.out_img = out_img;
    c.raster_u32 = 1, c.u32_pitch = row_pitch_pixels;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return render_forward_impl(c);
}

extern "C" uint32_t brush_rgba8_row_pitch(uint32_t width) { return (width + 63u) / 64u * 64u; }
