// render_bwd.hip — host orchestration of the backward pass behind the C ABI: one call description (BackwardCall), one
// opening, and the dense, fused (backward + Adam) and record entries on it.  No kernel.
//
// Replaces RenderBackwards::backward (crates/brush-render/src/render.rs:465-626).  Like the forward (render.hip) it only
// enqueues work on the caller's stream, allocates nothing and reads no count back to the host.
#include "render_host.hpp"
#include "splat_math.hpp"

namespace brush {
namespace {

struct BwdWs {
    float *v_compact;  // [N, kCompactStride] compact-order gradient rows (first V used)
    float *rows;       // deterministic mode: [cap, kCompactStride] one row per intersection, emission order
    float *partials;   // deterministic mode: [ceil(cap / 64), 2, kCompactStride] chunk-border partial sums
    size_t bytes;
};

BwdWs carve_bwd(void *ws, uint32_t n, uint32_t cap, bool det) {
    BwdWs b;
    Carver c(ws);
    const size_t nn = n ? n : 1;
    b.v_compact = c.take<float>(nn * kCompactStride);
    b.rows = b.partials = nullptr;
    if (det) {
        const size_t cc = cap ? cap : 1;
        b.rows = c.take<float>(cc * kCompactStride);
        b.partials = c.take<float>((size_t)ceil_div((uint32_t)cc, kWave) * 2 * kCompactStride);
    }
    b.bytes = c.bytes();
    return b;
}

// The depth-distortion term of brush_render_backward_distortion (distortion.hip).
struct DistortionTerm {
    const BrushDistortion *cfg;
    const float *stats, *v;
};

// The six dense gradients, in the order every entry takes them.
struct DenseGrads {
    float *v_means, *v_xy, *v_scales, *v_quats, *v_sh, *v_opac;
};

// One backward call as its entry describes it, filled by field name ({}: everything absent).  render_backward_impl
// reads all of it, brush_render_backward_records the part in front of the gradients.
struct BackwardCall {
    const BrushUniforms *uniforms;
    const BrushAux *aux;
    const float *means, *log_scales, *quats, *raw_opacity;
    uint32_t n;
    const float *out_img, *v_out;
    float *v_means, *v_xy, *v_scales, *v_quats, *v_sh, *v_opac;  // dense gradients (the fused forms: v_xy only)
    const AdamFuse *adam;                                        // fused forms: the optimizer step of the VJP kernel
    void *workspace;
    size_t workspace_bytes;
    brush_stream_t stream;
    // optional terms, each all there or all absent
    const float *compact_depth, *v_depth;  // depth
    float *v_viewmat;                      // pose
    void *pose_ws;
    const DistortionTerm *dist;
};

// The part of a BackwardCall every entry shares, and the dense gradients of the entries that have them; the entry sets
// its own term behind it.
BackwardCall common_call(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                         const float *log_scales, const float *quats, const float *raw_opacity, uint32_t n,
                         const float *out_img, const float *v_out, void *workspace, size_t workspace_bytes,
                         brush_stream_t stream, const DenseGrads &g = {}) {
    BackwardCall c{};
    c.uniforms = h_uniforms, c.aux = h_aux, c.means = means, c.log_scales = log_scales, c.quats = quats;
    c.raw_opacity = raw_opacity, c.n = n, c.out_img = out_img, c.v_out = v_out;
    c.v_means = g.v_means, c.v_xy = g.v_xy, c.v_scales = g.v_scales, c.v_quats = g.v_quats, c.v_sh = g.v_sh;
    c.v_opac = g.v_opac;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return c;
}

// What open_backward leaves for the kernels behind the compositing backward.
struct BackwardOpen {
    BwdWs ws;
    ViewParams vp;
    DetSumsArgs det;
    bool filled;  // the compositing kernel zero-filled the dense gradients in passing
    hipStream_t s;
};

}  // namespace

bool fill_adam_fuse(const BrushAdamConfig *cfg, float *means, float *log_scales, float *rotation, float *raw_opacity,
                    float *sh, uint32_t n, float *moment1, float *moment2, float *next_quats_fed, float *grad_2d_accum,
                    float *xy_grad_counts, uint32_t w, uint32_t h, uint32_t sh_degree, AdamFuse *out) {
    if (!cfg || cfg->time == 0) return false;
    if (n > 0 && (!means || !log_scales || !rotation || !raw_opacity || !sh || !moment1 || !moment2)) return false;
    auto aligned = [](const void *p) { return !misaligned(p, 16); };
    if (!aligned(rotation) || (next_quats_fed && !aligned(next_quats_fed))) return false;
    if ((grad_2d_accum == nullptr) != (xy_grad_counts == nullptr)) return false;
    AdamFuse af{};
    af.means = means, af.log_scales = log_scales, af.rotation = rotation, af.raw_opac = raw_opacity, af.sh = sh;
    af.m1 = moment1, af.m2 = moment2;
    af.lr[0] = cfg->lr_mean, af.lr[1] = cfg->lr_scale, af.lr[2] = cfg->lr_rotation, af.lr[3] = cfg->lr_opac;
    af.lr[4] = cfg->lr_coeffs_dc;
    af.sh_lerp = cfg->sh_rest_lerp, af.beta1 = cfg->beta1, af.beta2 = cfg->beta2, af.eps = cfg->epsilon;
    adam_bias_corrections(cfg->beta1, cfg->beta2, cfg->time, &af.rbc1, &af.rbc2);
    af.quat_vjp = cfg->rotation_grad_wrt_normalized;
    af.norm_rot_out = next_quats_fed;
    af.grad_2d_accum = grad_2d_accum, af.xy_grad_counts = xy_grad_counts;
    af.half_w = (float)w / 2.0f, af.half_h = (float)h / 2.0f;
    af.stat_scale = cfg->xy_stat_scale > 0.0f ? cfg->xy_stat_scale : 1.0f;
    af.vec_ok = (n % 4 == 0) && aligned(means) && aligned(log_scales) && aligned(sh) && aligned(moment1) &&
                aligned(moment2);
    if (cfg->lazy_sh) {
        // deferred Adam of the SH block: this step is optimizer time now + 1, the SH segments are the tails of the
        // moment arrays, and the chunked (16-byte) path must be the one that runs
        if (!make_lazy_sh(cfg->lazy_sh, sh_degree, &af.lazy) || !af.vec_ok || cfg->lazy_sh->now + 1u != cfg->time ||
            cfg->lazy_sh->sh_moment1 != moment1 + (size_t)11 * n || cfg->lazy_sh->sh_moment2 != moment2 + (size_t)11 * n)
            return false;
    }
    *out = af;
    return true;
}

}  // namespace brush

using namespace brush;

extern "C" int brush_bwd_workspace_size_flags(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree,
                                              uint32_t max_intersects, uint32_t flags, size_t *bytes) {
    (void)w;
    (void)h;
    // Only the bits that size the workspace are taken (brush_hip.h); BRUSH_AUX_ANTIALIASED sizes nothing and is refused
    // like any other bit, as before it existed.
    if (!bytes || sh_degree > 4 || (flags & ~BRUSH_AUX_DETERMINISTIC) != 0) return BRUSH_ERR_INVALID_ARG;
    *bytes = carve_bwd(nullptr, n, max_intersects, (flags & BRUSH_AUX_DETERMINISTIC) != 0).bytes;
    return BRUSH_OK;
}

extern "C" int brush_bwd_workspace_size_ex(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree,
                                           uint32_t max_intersects, size_t *bytes) {
    return brush_bwd_workspace_size_flags(n, w, h, sh_degree, max_intersects, 0u, bytes);
}

extern "C" int brush_bwd_workspace_size(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree, size_t *bytes) {
    return brush_bwd_workspace_size_ex(n, w, h, sh_degree, brush_default_max_intersects(n, w, h), bytes);
}

extern "C" int brush_pose_grad_workspace_size(uint32_t n, size_t *bytes) {
    if (!bytes) return BRUSH_ERR_INVALID_ARG;
    *bytes = pose_grad_workspace_bytes(n);
    return BRUSH_OK;
}

// RasterizeBackwards (render.rs:505-532): the compact-order sums of every visible splat.  Default: zero the
// accumulators, add with hardware float atomics.  Deterministic mode: one stored row per intersection, then the
// fixed-order per-splat sums (no zero-fill, no atomics).  Fills `det` for the consumer kernel.
// `fill` (may be inactive): zero-fill the compositing kernel carries in passing; *filled says whether it ran.
static int composite_backward(const BackwardCall &c, const BrushUniforms &u, const BwdWs &ws, DetSumsArgs *det,
                              const ZeroFill &fill, bool *filled, hipStream_t s) {
    const BrushAux &aux = *c.aux;
    const RasterFrame frame = raster_frame(u, aux);
    *filled = fill.active() && frame.tbx * frame.tby != 0u;  // (no tiles: no launch)
    RasterGrads g{};
    g.out_img = c.out_img, g.v_out = c.v_out, g.v_compact = ws.v_compact;
    g.compact_depth = c.compact_depth, g.v_depth = c.v_depth;
    if (ws.rows) {
        // no zero-fill stage in this mode: no launch, no event
        g.unsorted_pos = aux.isect_unsorted_pos, g.rows = ws.rows;
        BRUSH_HIP_CHECK(launch_rasterize_backward(frame, g, fill, s));
        BRUSH_HIP_CHECK(launch_sum_isect_rows(ws.rows, aux.num_intersections, aux.cum_tiles_hit, aux.max_intersects,
                                              ws.v_compact, ws.partials, s));
        if (c.v_depth)  // after the rows' sums: those write word 9 of their rows as 0
            BRUSH_HIP_CHECK(launch_sum_isect_depth(ws.rows, aux.num_intersections, aux.cum_tiles_hit,
                                                   aux.max_intersects, ws.v_compact, ws.partials, s));
        mark_stage(kBwdPass, s, 2);
        det->cum_tiles_hit = aux.cum_tiles_hit;
        det->num_intersections = aux.num_intersections;
        det->partials = ws.partials;
        det->cap = aux.max_intersects;
        return BRUSH_OK;
    }
    // compact-order accumulators are atomically added to: zero the first V rows (render.rs:505-507) — unless the
    // forward of this render already did (BrushAux::bwd_accum + BRUSH_AUX_ACCUM_ZEROED)
    if (!(aux.flags & BRUSH_AUX_ACCUM_ZEROED)) {
        BRUSH_HIP_CHECK(launch_zero_compact_grads(aux.num_visible, c.n, ws.v_compact, s));
        mark_stage(kBwdPass, s, 1);
    }
    if (stop_behind(BRUSH_STAGE_BWD_ZERO)) return BRUSH_OK;
    BRUSH_HIP_CHECK(launch_rasterize_backward(frame, g, fill, s));
    mark_stage(kBwdPass, s, 2);
    return BRUSH_OK;
}

// The opening every backward shares: the checks of what every BackwardCall holds (an entry makes its own first: all
// refusals come before any HIP call, and an invalid argument is reported whatever the workspace's size), the
// workspace, the view parameters, and the compositing backward with `fill` carried in passing.
static int open_backward(const BackwardCall &c, const ZeroFill &fill, BackwardOpen *o) {
    if (!uniforms_ok(c.uniforms) || !aux_ok(c.aux, true) || !c.out_img || !c.v_out || !c.workspace)
        return BRUSH_ERR_INVALID_ARG;
    if (c.n > 0 && (!c.means || !c.log_scales || !c.quats || !c.raw_opacity)) return BRUSH_ERR_INVALID_ARG;
    const BrushAux &aux = *c.aux;
    o->ws = carve_bwd(c.workspace, c.n, aux.max_intersects, aux_det(aux));
    if (c.workspace_bytes < o->ws.bytes) return BRUSH_ERR_WORKSPACE_SMALL;
    if ((aux.flags & BRUSH_AUX_ACCUM_ZEROED) && !aux_det(aux) && aux.bwd_accum != o->ws.v_compact) return BRUSH_ERR_INVALID_ARG;
    o->s = static_cast<hipStream_t>(c.stream);
    BrushUniforms u = *c.uniforms;
    u.total_splats = c.n;
    o->vp = make_view_params(u, c.n);
    mark_stage(kBwdPass, o->s, 0);
    return composite_backward(c, u, o->ws, &o->det, fill, &o->filled, o->s);
}

static int render_backward_impl(const BackwardCall &c) {
    if (c.dist && (!c.v_depth || c.adam || c.v_viewmat || !distortion_args_ok(c.aux, c.dist->cfg, c.dist->stats, c.dist->v)))
        return BRUSH_ERR_INVALID_ARG;
    if ((c.compact_depth != nullptr) != (c.v_depth != nullptr) || (c.v_depth && c.adam)) return BRUSH_ERR_INVALID_ARG;
    if ((c.v_viewmat != nullptr) != (c.pose_ws != nullptr)) return BRUSH_ERR_INVALID_ARG;
    if (c.n > 0 && !c.v_xy) return BRUSH_ERR_INVALID_ARG;
    if (c.n > 0 && !c.adam && (!c.v_means || !c.v_scales || !c.v_quats || !c.v_sh || !c.v_opac)) return BRUSH_ERR_INVALID_ARG;

    // Dense gradients (render.rs:539-547,573-575 zero-fill them with launches of their own): the VALU-bound compositing
    // kernel stores the zeros in passing, the VJP kernel behind it writes the visible splats' rows only.
    ZeroFill fill{};
    if (!c.adam && c.n > 0 && uniforms_ok(c.uniforms)) {  // (refused uniforms: the opening says so)
        const BrushUniforms &u = *c.uniforms;
        const size_t nn = c.n, C = (size_t)(u.sh_degree + 1) * (u.sh_degree + 1);
        float *const arrays[kFillSegs] = {c.v_sh, c.v_means, c.v_scales, c.v_quats, c.v_opac, c.v_xy};
        const size_t floats[kFillSegs] = {nn * C * 3, nn * 3, nn * 3, nn * 4, nn, nn * 2};
        (void)make_zero_fill(&fill, arrays, floats, kFillSegs);  // (unaligned / oversized arrays: zeros stay in the VJP kernel)
        // a frame of a few tiles has a few waves: more than 1 MiB of zeros per tile would turn the compositing launch
        // into a slow fill (1 M splats on a 64 x 64 frame); the all-in-one VJP kernel writes them at stream rate
        const uint64_t tiles = (uint64_t)u.tile_bounds[0] * u.tile_bounds[1];
        if (fill.first_block[kFillSegs] > 1024ull * (tiles ? tiles : 1ull)) fill = ZeroFill{};
    }
    BackwardOpen o;
    if (const int rc = open_backward(c, fill, &o)) return rc;
    if (stop_behind(BRUSH_STAGE_BWD_ZERO) || stop_behind(BRUSH_STAGE_RASTERIZE_BWD)) return BRUSH_OK;
    const BrushAux &aux = *c.aux;
    const bool antialiased = (aux.flags & BRUSH_AUX_ANTIALIASED) != 0;
    // depth distortion: its per-record VJP joins the compact rows the compositing backward has just summed
    if (c.dist)
        if (const int rc = launch_distortion_grad(c.uniforms, c.aux, c.compact_depth, c.dist->cfg, c.dist->stats,
                                                  c.dist->v, c.n, o.ws.v_compact, c.stream))
            return rc;
    // camera-pose gradient: ahead of the parameter VJP, whose fused Adam forms overwrite `means` in place
    if (c.v_viewmat)
        BRUSH_HIP_CHECK(launch_view_grad(o.vp, c.means, c.log_scales, c.quats, c.raw_opacity, aux.num_visible, c.n,
                                         aux.global_from_compact_gid, o.ws.v_compact, o.det, c.v_depth != nullptr,
                                         antialiased, c.pose_ws, c.v_viewmat, o.s));
    // GatherGrads + ProjectBackwards fused, dense outputs written once (render.rs:534-594)
    BRUSH_HIP_CHECK(launch_project_backward(o.vp, c.means, c.log_scales, c.quats, c.raw_opacity,
                                            aux.compact_from_global_gid, o.ws.v_compact, c.v_means, c.v_xy, c.v_scales,
                                            c.v_quats, c.v_sh, c.v_opac, c.adam, o.det, o.filled, o.s, antialiased));
    // depth: z = viewmat row 2 . [mean, 1] carries v_z into v_means
    if (c.v_depth)
        BRUSH_HIP_CHECK(launch_depth_means_grad(o.vp, aux.num_visible, c.n, aux.global_from_compact_gid, o.ws.v_compact,
                                                o.det, c.v_means, o.s));
    mark_stage(kBwdPass, o.s, 3);
    return BRUSH_OK;
}

extern "C" int brush_render_backward(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                     const float *log_scales, const float *quats, const float *raw_opacity,
                                     uint32_t n, const float *out_img, const float *v_out, float *v_means,
                                     float *v_xy, float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                     void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    return render_backward_impl(common_call(h_uniforms, h_aux, means, log_scales, quats, raw_opacity, n, out_img, v_out,
                                            workspace, workspace_bytes, stream,
                                            {v_means, v_xy, v_scales, v_quats, v_sh, v_opac}));
}

extern "C" int brush_render_backward_depth(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                           const float *log_scales, const float *quats, const float *raw_opacity,
                                           uint32_t n, const float *out_img, const float *v_out,
                                           const float *compact_depth, const float *v_depth, float *v_means,
                                           float *v_xy, float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                           void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    if (!compact_depth || !v_depth) return BRUSH_ERR_INVALID_ARG;
    BackwardCall c = common_call(h_uniforms, h_aux, means, log_scales, quats, raw_opacity, n, out_img, v_out, workspace,
                                 workspace_bytes, stream, {v_means, v_xy, v_scales, v_quats, v_sh, v_opac});
    c.compact_depth = compact_depth, c.v_depth = v_depth;
    return render_backward_impl(c);
}

extern "C" int brush_render_backward_distortion(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                                const float *means, const float *log_scales, const float *quats,
                                                const float *raw_opacity, uint32_t n, const float *out_img,
                                                const float *v_out, const float *compact_depth, const float *v_depth,
                                                const BrushDistortion *cfg, const float *stats,
                                                const float *v_distortion, float *v_means, float *v_xy, float *v_scales,
                                                float *v_quats, float *v_sh, float *v_opac, void *workspace,
                                                size_t workspace_bytes, brush_stream_t stream) {
    if (!compact_depth || !v_depth) return BRUSH_ERR_INVALID_ARG;
    const DistortionTerm dist{cfg, stats, v_distortion};
    BackwardCall c = common_call(h_uniforms, h_aux, means, log_scales, quats, raw_opacity, n, out_img, v_out, workspace,
                                 workspace_bytes, stream, {v_means, v_xy, v_scales, v_quats, v_sh, v_opac});
    c.compact_depth = compact_depth, c.v_depth = v_depth, c.dist = &dist;
    return render_backward_impl(c);
}

extern "C" int brush_render_backward_pose(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                          const float *log_scales, const float *quats, const float *raw_opacity,
                                          uint32_t n, const float *out_img, const float *v_out,
                                          const float *compact_depth, const float *v_depth, float *v_means,
                                          float *v_xy, float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                          void *workspace, size_t workspace_bytes, float *v_viewmat,
                                          void *pose_workspace, size_t pose_workspace_bytes, brush_stream_t stream) {
    if (!v_viewmat || !pose_workspace) return BRUSH_ERR_INVALID_ARG;
    if (pose_workspace_bytes < pose_grad_workspace_bytes(n)) return BRUSH_ERR_WORKSPACE_SMALL;
    BackwardCall c = common_call(h_uniforms, h_aux, means, log_scales, quats, raw_opacity, n, out_img, v_out, workspace,
                                 workspace_bytes, stream, {v_means, v_xy, v_scales, v_quats, v_sh, v_opac});
    c.compact_depth = compact_depth, c.v_depth = v_depth, c.v_viewmat = v_viewmat, c.pose_ws = pose_workspace;
    return render_backward_impl(c);
}

// The two fused forms; (v_viewmat, pose_ws): the pose pair as the entry gives it, or (nullptr, nullptr).
static int render_backward_adam_impl(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                     const BrushAdamConfig *cfg, float *means, float *log_scales,
                                     const float *quats_fed, float *rotation, float *raw_opacity, float *sh,
                                     uint32_t n, const float *out_img, const float *v_out, float *v_xy,
                                     float *moment1, float *moment2, float *next_quats_fed,
                                     float *grad_2d_accum, float *xy_grad_counts, void *workspace,
                                     size_t workspace_bytes, brush_stream_t stream, float *v_viewmat,
                                     void *pose_ws) {
    if (!cfg || cfg->time == 0 || !h_uniforms || h_uniforms->sh_degree > 4) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(quats_fed, 16)) return BRUSH_ERR_INVALID_ARG;
    AdamFuse af{};
    if (!fill_adam_fuse(cfg, means, log_scales, rotation, raw_opacity, sh, n, moment1, moment2, next_quats_fed,
                        grad_2d_accum, xy_grad_counts, h_uniforms->img_size[0], h_uniforms->img_size[1],
                        h_uniforms->sh_degree, &af))
        return BRUSH_ERR_INVALID_ARG;
    BackwardCall c = common_call(h_uniforms, h_aux, means, log_scales, quats_fed, raw_opacity, n, out_img, v_out,
                                 workspace, workspace_bytes, stream);
    c.v_xy = v_xy, c.adam = &af;
    c.v_viewmat = v_viewmat, c.pose_ws = pose_ws;
    return render_backward_impl(c);
}

extern "C" int brush_render_backward_adam(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                          const BrushAdamConfig *cfg, float *means, float *log_scales,
                                          const float *quats_fed, float *rotation, float *raw_opacity, float *sh,
                                          uint32_t n, const float *out_img, const float *v_out, float *v_xy,
                                          float *moment1, float *moment2, float *next_quats_fed,
                                          float *grad_2d_accum, float *xy_grad_counts, void *workspace,
                                          size_t workspace_bytes, brush_stream_t stream) {
    return render_backward_adam_impl(h_uniforms, h_aux, cfg, means, log_scales, quats_fed, rotation, raw_opacity, sh, n,
                                     out_img, v_out, v_xy, moment1, moment2, next_quats_fed, grad_2d_accum,
                                     xy_grad_counts, workspace, workspace_bytes, stream, nullptr, nullptr);
}

extern "C" int brush_render_backward_adam_pose(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                               const BrushAdamConfig *cfg, float *means, float *log_scales,
                                               const float *quats_fed, float *rotation, float *raw_opacity, float *sh,
                                               uint32_t n, const float *out_img, const float *v_out, float *v_xy,
                                               float *moment1, float *moment2, float *next_quats_fed,
                                               float *grad_2d_accum, float *xy_grad_counts, void *workspace,
                                               size_t workspace_bytes, float *v_viewmat, void *pose_workspace,
                                               size_t pose_workspace_bytes, brush_stream_t stream) {
    if (!v_viewmat || !pose_workspace) return BRUSH_ERR_INVALID_ARG;
    if (pose_workspace_bytes < pose_grad_workspace_bytes(n)) return BRUSH_ERR_WORKSPACE_SMALL;
    return render_backward_adam_impl(h_uniforms, h_aux, cfg, means, log_scales, quats_fed, rotation, raw_opacity, sh, n,
                                     out_img, v_out, v_xy, moment1, moment2, next_quats_fed, grad_2d_accum,
                                     xy_grad_counts, workspace, workspace_bytes, stream, v_viewmat, pose_workspace);
}

// ---- view-sharded data parallelism (build extension): the per-view records on the shared opening; their
// reduction over views is view_records.hip ------------------------------------------------------------------------

extern "C" int brush_render_backward_records(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                             const float *log_scales, const float *quats, const float *raw_opacity,
                                             uint32_t n, const float *out_img, const float *v_out, float *records,
                                             uint32_t max_rows, void *workspace, size_t workspace_bytes,
                                             brush_stream_t stream) {
    if ((n > 0 && max_rows > 0 && !records) || misaligned(records, 16)) return BRUSH_ERR_INVALID_ARG;
    if (h_aux && (h_aux->flags & BRUSH_AUX_ANTIALIASED)) return BRUSH_ERR_INVALID_ARG;  // out of scope (brush_hip.h)
    const BackwardCall c = common_call(h_uniforms, h_aux, means, log_scales, quats, raw_opacity, n, out_img, v_out,
                                       workspace, workspace_bytes, stream);
    BackwardOpen o;
    if (const int rc = open_backward(c, ZeroFill{}, &o)) return rc;
    BRUSH_HIP_CHECK(launch_project_backward_records(o.vp, means, log_scales, quats, raw_opacity, h_aux->num_visible,
                                                    h_aux->global_from_compact_gid, o.ws.v_compact, records, max_rows,
                                                    o.det, o.s));
    mark_stage(kBwdPass, o.s, 3);
    return BRUSH_OK;
}
