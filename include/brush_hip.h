/*
 * brush_hip.h — C ABI of libbrush_hip.so: the MI355X (gfx950) replacement for the
 * splat-rasterizer hot path of wartron/brush.
 *
 * Drop-in boundary.  Each entry point names the reference interface it replaces
 * (paths relative to the reference checkout):
 *
 *   brush_render_forward    <- render_forward / Backend::render_splats
 *                              crates/brush-render/src/render.rs:55-323, src/lib.rs:66-86
 *   brush_render_backward   <- impl Backward<_,6> for RenderBackwards
 *                              crates/brush-render/src/render.rs:465-626
 *   brush_radix_argsort_u32 <- radix_argsort          crates/brush-sort/src/lib.rs:32-37
 *   brush_inclusive_scan_u32<- prefix_sum             crates/brush-prefix-sum/src/lib.rs:17
 *   *_workspace_size        <- create_tensor / client.empty scratch allocation
 *                              crates/brush-kernel/src/lib.rs:125-150
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer unless its name starts with `h_`.
 *   - The caller owns all memory (inputs, outputs, aux, workspace).  The library never
 *     allocates, frees or synchronises on these paths; all work is enqueued on `stream`
 *     (a hipStream_t) and the call returns immediately.  Data-dependent sizes
 *     (num_visible, num_intersections) stay on the device.
 *   - Functions are re-entrant: no global mutable state, per-call workspace; every mode switch is an argument
 *     (BrushAux::flags), nothing on these paths reads the environment.
 *   - Return value: BRUSH_OK or a negative BrushStatus; nothing aborts.
 *   - All floating point is f32, all indices/counts u32 (i32-typed tensors in Burn).
 */
#ifndef BRUSH_HIP_H
#define BRUSH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *brush_stream_t; /* hipStream_t */

typedef enum BrushStatus {
    BRUSH_OK = 0,
    BRUSH_ERR_INVALID_ARG = -1,    /* bad shape / null pointer / sh_degree > 4 / bits > 32 */
    BRUSH_ERR_WORKSPACE_SMALL = -2,
    BRUSH_ERR_HIP = -3,            /* a HIP call failed; see brush_last_hip_error() */
    BRUSH_ERR_NO_DEVICE = -4
} BrushStatus;

/* RenderUniforms, 28 words — crates/brush-render/src/shaders/helpers.wgsl:7-30, filled like
 * render.rs:102-116.  viewmat is world->camera, column-major.  num_visible is an OUTPUT of the
 * forward pass inside aux.uniforms_buffer (word 25, render.rs:145-149); the host copy passed
 * in is read-only and its num_visible/total_splats/padding fields are ignored. */
typedef struct BrushUniforms {
    float viewmat[16];
    float focal[2];
    uint32_t img_size[2]; /* (w, h) */
    uint32_t tile_bounds[2];
    float pixel_center[2];
    uint32_t sh_degree;
    uint32_t num_visible;
    uint32_t total_splats;
    uint32_t padding;
} BrushUniforms;

#define BRUSH_TILE_WIDTH 16u
#define BRUSH_PROJECTED_FLOATS 9u /* ProjectedSplat, helpers.wgsl:33-43 */

/* Deferred Adam for the spherical-harmonics block (build extension of the training harness; optional everywhere it
 * appears).  81 % of the optimizer's bytes at SH degree 3 are the coefficients and their two moments (48 of 59 floats
 * per splat), yet the forward reads a splat's coefficients only when the splat passes the cull, and a splat that is
 * not visible has a zero gradient.  With this state attached, the optimizer steps of a splat's SH block that carry a
 * zero gradient are not applied when they happen; they stay pending and are replayed - the same float operations in the
 * same order as burn's Adam::step would have run them, step by step, so the values are bit-identical to the eager
 * optimizer - when the block is next needed: by the forward in registers (a pure read: the forward still modifies none
 * of its inputs), by the fused backward before it applies the step that does carry a gradient, or by
 * brush_lazy_sh_flush.  sh_time[g] is the optimizer time the stored SH block of splat g is current for.
 * `table` row i holds (1 / (1 - beta1^t), 1 / (1 - beta2^t), lr_coeffs_dc, sh_rest_lerp) of optimizer time
 * t = base + 1 + i, as brush_lazy_sh_fill_table computes them - the code that serves BrushAdamConfig::time in the fused
 * eager step, so a replayed step uses the very floats the eager step was given; every pending time must lie inside the
 * table: flush before `now` leaves it.  (Fused forms: the update is x - lr (m rbc1) rcp(sqrt(v rbc2) + eps) with
 * v_sqrt_f32 / v_rcp_f32, 1 ulp each; WGSL specifies its division to 2.5 ulp.) */
typedef struct BrushLazySh {
    const float *table;   /* device, [capacity][4] */
    uint32_t base;        /* optimizer time of row 0, minus 1 */
    uint32_t capacity;
    uint32_t now;         /* optimizer steps taken so far (the eager optimizer's `time` after its last step) */
    uint32_t *sh_time;    /* device, [N]; <= now */
    float *sh_moment1;    /* device, [N][C][3]: the SH segment of moment1 (moment1 + 11 N) */
    float *sh_moment2;
    float beta1, beta2, epsilon;
} BrushLazySh;

/* Device-pointer mirror of RenderAux (crates/brush-render/src/lib.rs:20-33).  All buffers are
 * caller-allocated with the shapes below and must stay alive and unmodified between
 * brush_render_forward and brush_render_backward (render.rs:436-446). */
typedef struct BrushAux {
    float *projected_splats;           /* [N,9] f32; rows < num_visible valid, compact order */
    uint32_t *uniforms_buffer;         /* [28]  written by forward (num_visible at word 25) */
    uint32_t *num_intersections;       /* [1]   = min(sum tiles hit, max_intersects) */
    uint32_t *num_visible;             /* [1] */
    uint32_t *final_index;             /* [h,w] last contributing isect id (0 if none) */
    uint32_t *cum_tiles_hit;           /* [N]   inclusive scan of tiles hit; tail == total */
    uint32_t *tile_bins;               /* [ty,tx,2] [start,end) into compact_gid_from_isect */
    uint32_t *compact_gid_from_isect;  /* [max_intersects] sorted by (tile, depth) */
    uint32_t *global_from_compact_gid; /* [N] depth order; entries >= num_visible are 0 */
    uint32_t *compact_from_global_gid; /* [N] inverse of global_from_compact_gid, 0xFFFFFFFF for
                                          non-visible splats (build extension: lets the backward
                                          write each dense gradient exactly once) */
    uint32_t *overflow;                /* [1] set to 1 when intersections were truncated at
                                          max_intersects (the reference truncates silently,
                                          map_gaussian_to_intersects.wgsl:40) */
    uint32_t max_intersects;           /* capacity; reference: min(N*tiles, 128*65535)
                                          (render.rs:204-206) */
    uint32_t *isect_unsorted_pos;      /* [max_intersects] or NULL.  Deterministic mode (flags &
                                          BRUSH_AUX_DETERMINISTIC) only: position each sorted intersection had in
                                          emission order (grouped by splat), written by the forward and used by
                                          the backward to sum a splat's per-tile gradient rows in a fixed order.
                                          Must be non-NULL in that mode, ignored otherwise. */
    uint32_t flags;                    /* BRUSH_AUX_* bits, chosen PER CALL; the forward and the backward of one
                                          render must be given the same BRUSH_AUX_DETERMINISTIC and
                                          BRUSH_AUX_ANTIALIASED bits */
    float *bwd_accum;                  /* NULL, or the buffer the caller will pass as `workspace` to the backward of
                                          this render (brush_bwd_workspace_size* bytes).  Default mode only: the
                                          forward's last kernel then also zeroes the backward's per-splat accumulator
                                          rows (the first num_visible 64-byte rows of that buffer), and a backward
                                          called with BRUSH_AUX_ACCUM_ZEROED skips its zero-fill launch.  The
                                          reference zero-fills inside the backward (render.rs:505-507); at 100 k
                                          visible splats that launch is 6 us of a 345 us step for 6.6 MB of stores the
                                          VALU-bound compositing kernel carries for free. */
    const BrushLazySh *lazy_sh;        /* NULL, or the deferred-Adam state of the SH coefficients (host pointer, read
                                          during the call only): the forward then evaluates a visible splat's colour
                                          from its coefficients with the pending zero-gradient steps replayed in
                                          registers.  `sh_coeffs` itself is not written. */
} BrushAux;

/* BrushAux::flags */
#define BRUSH_AUX_DETERMINISTIC 1u /* bitwise reproducible gradients: the compositing backward stores one gradient
                                      row per intersection and sums a splat's rows in a fixed order instead of
                                      using hardware float atomics (whose arrival order is unspecified; the
                                      reference's CAS queue, rasterize_backwards.wgsl:276-301, has the same
                                      nondeterminism).  Needs isect_unsorted_pos and the larger backward workspace
                                      of brush_bwd_workspace_size_flags. */
#define BRUSH_AUX_ACCUM_ZEROED 2u  /* backward only, default mode: `workspace` == aux.bwd_accum of the forward of this
                                      render, nothing has written to it since, and no backward has consumed it yet
                                      (the FIRST backward after that forward): the accumulators are already zero.  A
                                      second backward of the same forward must clear the bit (it zero-fills itself). */
#define BRUSH_AUX_ANTIALIASED 4u   /* antialiased mode (build extension; Mip-Splatting's 2D filter, gsplat's
                                      rasterize_mode="antialiased"): every projected covariance S still gets the 0.3 px^2
                                      blur (helpers.wgsl:153-157), and the opacity a splat is drawn with is scaled so
                                      that its integrated weight stays what it was before the blur:
                                          o = sigmoid(raw) * comp,  comp = sqrt(max(0, det(S) / det(S + 0.3 I)))
                                      with det(S) from the unblurred covariance (0 where det(S) <= 0).  Word 8 of a
                                      projected_splats row holds o; xy, conic, colour and the visible set are those of the
                                      plain mode (intersections can only drop: the tile test sees the smaller o).
                                      Gradient: with v_o the compositing gradient with respect to o,
                                          v_raw = v_o comp sigmoid(1 - sigmoid)
                                      and v_comp = v_o sigmoid enters the gradient of S + 0.3 I = (c00, c01, c11) as
                                          v_sqr = v_comp 0.5 / (comp + 1e-6),
                                          v_c00 += v_sqr ((1 - comp^2) conic.x - 0.3 det(conic)),
                                          v_c01 += 2 v_sqr (1 - comp^2) conic.y,
                                          v_c11 += v_sqr ((1 - comp^2) conic.z - 0.3 det(conic))
                                      (the reference's disabled VJP, project_backwards.wgsl:112-128; nothing where
                                      comp = 0), then the plain chain to means, scales and quats.  The forward and the
                                      backward of one render must be given the same bit.  Accepted by the forward entry
                                      points, brush_render_backward(_depth) and brush_render_backward_adam, in both
                                      modes.  The mode needs no extra workspace: size the backward with the render's
                                      flags & BRUSH_AUX_DETERMINISTIC (brush_bwd_workspace_size_flags takes only the bits
                                      that size the workspace and refuses this one, as it did before the bit existed).
                                      brush_render_backward_records (data-parallel training) returns
                                      BRUSH_ERR_INVALID_ARG with it (out of scope). */

/* ---- introspection ------------------------------------------------------------------ */
const char *brush_version(void);
const char *brush_status_string(int status);
/* hipError_t of the last failing HIP call on this host thread (0 if none). */
int brush_last_hip_error(void);
/* Reference limit helper: min(N * tiles, 128*65535), at least 1 (render.rs:204-206). */
uint32_t brush_default_max_intersects(uint32_t n, uint32_t w, uint32_t h);

/* ---- radix argsort (brush-sort) ----------------------------------------------------- */
/* Stable LSD argsort of the first *d_n (device scalar, <= max_n) key/value pairs on the low
 * 4*ceil(bits/4) key bits (the reference runs ceil(bits/4) 4-bit passes,
 * brush-sort/src/lib.rs:58).  Inputs are not modified; outputs hold the sorted pairs in
 * [0, *d_n); elements beyond are unspecified (sort_scatter.wgsl:118-121). */
int brush_radix_argsort_workspace_size(uint32_t max_n, size_t *bytes);
int brush_radix_argsort_u32(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                            uint32_t *vals_out, const uint32_t *d_n, uint32_t max_n,
                            uint32_t sorting_bits, void *workspace, size_t workspace_bytes,
                            brush_stream_t stream);

/* ---- prefix sum (brush-prefix-sum) ---------------------------------------------------- */
/* out[i] = in[0] + ... + in[i] (wrapping u32), n known on the host like the reference's
 * tensor shape (brush-prefix-sum/src/lib.rs:19). in == out is allowed. */
int brush_inclusive_scan_workspace_size(uint32_t n, size_t *bytes);
int brush_inclusive_scan_u32(const uint32_t *in, uint32_t *out, uint32_t n, void *workspace,
                             size_t workspace_bytes, brush_stream_t stream);

/* ---- render forward ------------------------------------------------------------------- */
int brush_fwd_workspace_size(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree,
                             uint32_t max_intersects, size_t *bytes);
/* means[N,3] log_scales[N,3] quats[N,4] (w,x,y,z; already normalised) sh_coeffs[N,C,3]
 * raw_opacity[N].
 * Quaternion contract (this entry point, brush_render_forward_rgba8 and brush_render_forward_depth): quats must be
 * unit, as Splats.render and the trainer (brush_normalize_quats) provide them.  Results equal the reference's for
 * |q| <= 1.1; beyond that a splat whose centre is off-frame may be culled where the reference keeps it (the cull's
 * screen-bounds prefilter bounds the covariance by s_max^2 without reading the quaternion, project.hip).
 * out_img: raster_u32 == 0 -> float[h,w,4] (rgb, 1-T); != 0 -> uint32[h,w]
 * packed RGBA8 (rasterize.wgsl:106-109) and aux->final_index is not written. */
int brush_render_forward(const BrushUniforms *h_uniforms, const float *means,
                         const float *log_scales, const float *quats, const float *sh_coeffs,
                         const float *raw_opacity, uint32_t n, int raster_u32, void *out_img,
                         const BrushAux *h_aux, void *workspace, size_t workspace_bytes,
                         brush_stream_t stream);

/* Forward-only display path: packed RGBA8 (rasterize.wgsl:106-109) written
 * with rows `row_pitch_pixels` pixels apart, so the viewer's texture upload needs no padding
 * copy.  The reference pads the [h,w] u32 image into a zero [h, ceil(w/64)*64] tensor because
 * WebGPU wants bytes_per_row % 256 == 0 (crates/brush-ui/src/burn_texture.rs:17-26);
 * brush_rgba8_row_pitch(w) returns that pitch.  out_img: [h * row_pitch_pixels] u32; columns
 * >= w of each row are left untouched.  aux.final_index may be NULL (not written, as in the
 * reference's RASTER_U32 variant).  Otherwise identical to brush_render_forward(raster_u32=1). */
uint32_t brush_rgba8_row_pitch(uint32_t width);
int brush_render_forward_rgba8(const BrushUniforms *uniforms, const float *means, const float *log_scales,
                               const float *quats, const float *sh_coeffs, const float *raw_opacity,
                               uint32_t n, uint32_t *out_img, uint32_t row_pitch_pixels, const BrushAux *aux,
                               void *workspace, size_t workspace_bytes, brush_stream_t stream);

/* Accumulated depth beside the colour image (build extension; the reference has no depth output).  For a pixel p
 *     D(p) = sum_i T_i alpha_i z_i
 * over exactly the entries the colour forward composites into p: the same alpha (0.999 clamp), the same
 * alpha >= 1/255 test and T <= 1e-4 stop, in the same order.  z_i is the camera-space z of splat i's mean
 * (p_view.z, project_forward.wgsl:67), the key of the depth sort.  D is NOT normalised: the alpha-normalised
 * expected depth is D / alpha with alpha = out_img[..., 3].
 * out_img, final_index, tile_bins, the counts and every other aux array come out bitwise identical to
 * brush_render_forward(raster_u32 = 0) with the same aux flags; the workspace is brush_fwd_workspace_size's.
 * out_depth: [h,w] f32.  compact_depth: [N] f32, written with z of the visible splats in compact (depth) order;
 * keep it for brush_render_backward_depth. */
int brush_render_forward_depth(const BrushUniforms *h_uniforms, const float *means, const float *log_scales,
                               const float *quats, const float *sh_coeffs, const float *raw_opacity, uint32_t n,
                               float *out_img, float *out_depth, float *compact_depth, const BrushAux *h_aux,
                               void *workspace, size_t workspace_bytes, brush_stream_t stream);

/* ---- render backward ------------------------------------------------------------------ */
/* A host-side DEFAULT for BrushAux::flags, nothing more: 1 when the environment holds BRUSH_DETERMINISTIC=1 (read
 * on every call, never cached, never consulted by the render entry points themselves).  A host that wants the
 * mode per call (a viewer thread beside a trainer task) sets or clears BRUSH_AUX_DETERMINISTIC itself. */
int brush_deterministic(void);
/* Backward workspace for a call with these BrushAux::flags and this intersection capacity (the deterministic mode
 * keeps 64 bytes per intersection).  `flags` holds the bits that size the workspace, i.e. BRUSH_AUX_DETERMINISTIC or
 * nothing; any other bit returns BRUSH_ERR_INVALID_ARG (an antialiased render passes flags & BRUSH_AUX_DETERMINISTIC). */
int brush_bwd_workspace_size_flags(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree, uint32_t max_intersects,
                                   uint32_t flags, size_t *bytes);
/* Shorthands: flags = 0 (the default mode); brush_bwd_workspace_size also assumes
 * brush_default_max_intersects(n, w, h). */
int brush_bwd_workspace_size(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree,
                             size_t *bytes);
int brush_bwd_workspace_size_ex(uint32_t n, uint32_t w, uint32_t h, uint32_t sh_degree, uint32_t max_intersects,
                                size_t *bytes);
/* Gradients in the parent order of render.rs:420-427,598-624:
 * v_means[N,3] v_xy[N,2] (global order, pixel units) v_scales[N,3] (log-space)
 * v_quats[N,4] v_sh[N,C,3] v_opac[N] — dense, every element written, 0 for non-visible
 * splats.  out_img / v_out are float[h,w,4].  The six gradient arrays are written from the first kernel of the call on
 * (their zeros ride on the compositing backward): they must not overlap any input of the call, the aux buffers or the
 * workspace — as separately allocated Burn tensors never do. */
int brush_render_backward(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                          const float *means, const float *log_scales, const float *quats,
                          const float *raw_opacity, uint32_t n, const float *out_img,
                          const float *v_out, float *v_means, float *v_xy, float *v_scales,
                          float *v_quats, float *v_sh, float *v_opac, void *workspace,
                          size_t workspace_bytes, brush_stream_t stream);

/* brush_render_backward for a brush_render_forward_depth render, with v_depth [h,w] the gradient of out_depth.  The
 * depth is a fourth colour channel whose per-splat value is z (compact_depth of that forward) under the backward's
 * rules (0.99 clamp, rasterize_backwards.wgsl:239), and dL/dz_i = sum_p T alpha v_depth(p) flows into v_means through
 * z = row 2 of viewmat . [mean, 1].  Same workspace (brush_bwd_workspace_size_flags), same aliasing rules and same
 * outputs as brush_render_backward; with v_depth = 0 the deterministic mode gives its gradients bit for bit. */
int brush_render_backward_depth(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                const float *log_scales, const float *quats, const float *raw_opacity, uint32_t n,
                                const float *out_img, const float *v_out, const float *compact_depth,
                                const float *v_depth, float *v_means, float *v_xy, float *v_scales, float *v_quats,
                                float *v_sh, float *v_opac, void *workspace, size_t workspace_bytes,
                                brush_stream_t stream);

/* ---- camera-pose gradient (build extension) ---------------------------------------------------------------- */
/* brush_render_backward_depth that also returns the gradient with respect to the camera: v_viewmat[12] (device, f32),
 * row-major 3x4 = [d L / d W row r | d L / d t[r]] of the world-to-camera transform p = W mean + t that
 * BrushUniforms::viewmat holds column-major (W[r][c] = viewmat[4 c + r], t[r] = viewmat[12 + r]).  All twelve words
 * are written on every call, zeros included (no visible splat, n = 0).  compact_depth / v_depth may both be NULL: the
 * call is then brush_render_backward plus v_viewmat.  The six dense gradients are exactly those of
 * brush_render_backward / _depth (bit for bit in deterministic mode).
 * Per visible splat the chain of the parameter backward is followed to its last link (v_p, the gradient at p, and v_T,
 * the gradient at T = J W): v_t = sum v_p, v_W = sum (v_p mean^T + J^T v_T), summed in float64 in a fixed order with no
 * atomics: the same inputs give the same words (bit for bit when the compact sums are, i.e. in deterministic mode).
 * Conventions inherited from that backward: J is taken at the unclamped p_view; no gradient flows through the SH view
 * direction (mean - viewmat[12..14]), so above SH degree 0 this is the gradient with the colours held fixed; culling and
 * tile decisions are piecewise constant.  Intrinsics (focal, centre) get no gradient.
 * pose_workspace: brush_pose_grad_workspace_size(n) bytes (8-byte aligned), scratch, no state between calls.  No
 * allocation, no synchronisation: the call can be captured into a graph. */
int brush_pose_grad_workspace_size(uint32_t n, size_t *bytes);
int brush_render_backward_pose(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                               const float *log_scales, const float *quats, const float *raw_opacity, uint32_t n,
                               const float *out_img, const float *v_out, const float *compact_depth,
                               const float *v_depth, float *v_means, float *v_xy, float *v_scales, float *v_quats,
                               float *v_sh, float *v_opac, void *workspace, size_t workspace_bytes, float *v_viewmat,
                               void *pose_workspace, size_t pose_workspace_bytes, brush_stream_t stream);

/* ---- view-sharded data parallelism (build extension; the reference is single-device, batch 1:
 *      crates/brush-train/src/train.rs:216-219) ------------------------------------------------ */
/* One process per GPU renders one view of the replicated splats; the step needs the SUM over views of the
 * parameter gradients.  A view's gradient is non-zero only for its visible splats and its SH row is rank one
 * (v_sh[g] = Y(dir_view(g)) (x) v_rgb[g], gather_grads.wgsl:186-222), so it is exchanged as one 64-byte record
 * per VISIBLE splat (16 f32, compact = depth order):
 *   [gid as u32 bits | v_means(3) | v_scales(3) | v_quats(4) | v_opac | v_rgb(3) | |v_xy * (w/2, h/2)|]
 * instead of 52+12C bytes per splat.  The caller all-gathers the records (RCCL; brush_amd/dist.py), then the
 * per-splat sum over views runs in view order 0..W-1 without atomics: bit-identical on every rank and from run
 * to run, so replicated parameters stay replicated.
 *
 * brush_render_backward_records: brush_render_backward without the dense outputs.  Writes rows
 * c < min(num_visible, max_rows) of `records` ([max_rows][16], 16-byte aligned); rows beyond max_rows are DROPPED:
 * size max_rows from the view's num_visible (known after the forward).  Same workspace as brush_render_backward. */
int brush_render_backward_records(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *means,
                                  const float *log_scales, const float *quats, const float *raw_opacity, uint32_t n,
                                  const float *out_img, const float *v_out, float *records, uint32_t max_rows,
                                  void *workspace, size_t workspace_bytes, brush_stream_t stream);
/* Scratch of the reduction: num_views * n u32 (row of splat g in view v's records).  Results never depend on its
 * contents (entries are validated against the record they point to), but set it to 0xFF bytes once before the first
 * use: the reduction clears the entries it consumes, so from then on an entry nobody wrote this step is recognised
 * without a gather.  No reset between steps. */
int brush_view_index_size(uint32_t n, uint32_t num_views, size_t *bytes);
/* Sum over views -> dense gradients.  records: [num_views][rows_per_view][16]; view v owns its first
 * view_rows[v] rows (device array [num_views], values > rows_per_view are clamped).  view_offsets (device array
 * [num_views], or NULL): when given the views are PACKED — view v owns rows [view_offsets[v], + view_rows[v]) of a
 * buffer of rows_per_view rows in all — which is what an all-gather of exactly num_visible records per view leaves
 * (the padded form moves num_views x the largest view).  campos: [num_views][3] =
 * viewmat[3].xyz of each view (the term the reference uses as camera position, project_visible.wgsl:232-233);
 * means: [N,3].  Every element of v_means [N,3] v_scales [N,3] v_quats [N,4] v_sh [N,C,3] v_opac [N] is written
 * (0 for splats no view sees). */
int brush_reduce_view_records(const float *records, uint32_t num_views, uint32_t rows_per_view,
                              const uint32_t *view_rows, const uint32_t *view_offsets, const float *campos,
                              const float *means, uint32_t n, uint32_t sh_degree, float *v_means, float *v_scales,
                              float *v_quats, float *v_sh, float *v_opac, void *view_index, size_t view_index_bytes,
                              brush_stream_t stream);

/* ---- training iteration around the op (build extension) -------------------- */
/* The reference's SplatTrainer::step (crates/brush-train/src/train.rs:211-393) wraps the op in
 * Burn tensor ops: image loss, Adam, gradient statistics.  These entry points are the fused
 * HIP equivalents, so the metric's train iters/s is not bounded by caller-side launches. */

/* loss = mean|pred_cmp - gt| * (1 - ssim_weight) - SSIM(pred_rgb, gt_rgb) * ssim_weight when
 * ssim_weight > 0, else the plain L1 mean (train.rs:243-268); SSIM as ssim.rs:42-101 (Gaussian
 * window, sigma 1.5, zero padding div_ceil(window, 2) so the SSIM map is (h+2)x(w+2), variances clamped at 0).
 * pred: [h,w,4]; gt: [h,w,gt_channels], gt_channels 3 or 4 (4 compares alpha too, train.rs:248-252).
 * Writes loss[0] (device) and v_pred [h,w,4] = grad_scale * d loss / d pred.  ssim_window: odd sizes 3..15
 * (TrainConfig::ssim_window_size, train.rs:63, default 11); anything else returns BRUSH_ERR_INVALID_ARG. */
int brush_loss_workspace_size(uint32_t w, uint32_t h, size_t *bytes);
int brush_l1_ssim_loss(const float *pred, const float *gt, uint32_t w, uint32_t h, uint32_t gt_channels,
                       float ssim_weight, uint32_t ssim_window, float grad_scale, float *loss, float *v_pred,
                       void *workspace, size_t workspace_bytes, brush_stream_t stream);

/* ---- evaluation on held-out views (build extension) -------------------------------------- */
/* The per-view metrics of eval_stats (crates/brush-train/src/eval.rs:27-77) in one metrics-only pass: writes
 * out[0..2] = {mse, psnr, ssim} (device, f32) and nothing per pixel.
 *   mse  = mean((pred_rgb - gt_rgb)^2) over h*w*3 elements (eval.rs:55-57);
 *   psnr = ln(1 / mse) * 10 / LN_10 in f32 (eval.rs:59), +inf when mse == 0;
 *   ssim = mean of the SSIM map of ssim.rs:42-101 with Ssim::new(ssim_window, 3): Gaussian window sigma 1.5, zero
 *          padding div_ceil(window, 2) (map (h+2)x(w+2)x3), variances clamped at 0, C1 = 0.01^2, C2 = 0.03^2.
 * pred: [h,w,4] f32, the op's output; only RGB is read.  gt: [h,w,gt_channels], gt_channels 3 or 4, elements u8
 * (BRUSH_EVAL_GT_U8, read as (float)b / 255.0f with an IEEE division, as image_to_tensor) or f32 (BRUSH_EVAL_GT_F32).
 * The alpha of both is ignored: the reference compares to_rgb8() images (eval.rs:50-57).  ssim_window: odd sizes 3..15
 * (the reference's eval uses 11).  Sums are reduced per block, then by one workgroup in a fixed order: the same inputs
 * give the same bits on every call; no allocation or synchronisation, so the call can be captured into a graph.
 * Images of 2^28 pixels or more return BRUSH_ERR_INVALID_ARG. */
#define BRUSH_EVAL_GT_U8 0u
#define BRUSH_EVAL_GT_F32 1u
int brush_eval_workspace_size(uint32_t w, uint32_t h, size_t *bytes);
int brush_eval_metrics(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t w, uint32_t h,
                       uint32_t gt_channels, uint32_t ssim_window, float *out, void *workspace,
                       size_t workspace_bytes, brush_stream_t stream);

/* brush_l1_ssim_loss with the ground truth's element type chosen per call: gt_dtype BRUSH_EVAL_GT_U8 (a training image
 * kept on the device as uploaded, read as (float)b / 255.0f with an IEEE division, as image_to_tensor) or
 * BRUSH_EVAL_GT_F32 (the same as brush_l1_ssim_loss).  A u8 target gives the bits of an f32 target holding u8 / 255:
 * loss and v_pred are bitwise those of brush_l1_ssim_loss on that f32 image.  Same workspace
 * (brush_loss_workspace_size), the same argument checks and status codes; any other gt_dtype returns
 * BRUSH_ERR_INVALID_ARG. */
int brush_l1_ssim_loss_gt(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t w, uint32_t h,
                          uint32_t gt_channels, float ssim_weight, uint32_t ssim_window, float grad_scale, float *loss,
                          float *v_pred, void *workspace, size_t workspace_bytes, brush_stream_t stream);

/* Hyper-parameters of one optimizer step: the five learning rates of train.rs:275-282, the lerp
 * factor 1/lr_coeffs_sh_scale for SH coefficients >= 1 (train.rs:336-351), Adam betas/epsilon
 * (AdamConfig::new().with_epsilon(1e-15), train.rs:184) and the 1-based step count. */
typedef struct BrushAdamConfig {
    float lr_mean, lr_scale, lr_rotation, lr_opac, lr_coeffs_dc, sh_rest_lerp;
    float beta1, beta2, epsilon;
    uint32_t time;
    /* 1: `quats` holds the raw rotation parameter and v_quats is the gradient wrt rotation/|rotation|
     * (what Splats::render feeds the op, gaussian_splats.rs:174-175); the chain rule through the
     * normalisation is applied before the moment update.  0: v_quats is used as is. */
    uint32_t rotation_grad_wrt_normalized;
    /* Multiplies the screen-space statistic |v_xy * (w/2, h/2)| before it is added to grad_2d_accum (fused forms only).
     * With B views per step the upstream gradient carries the 1/B of the mean over the batch (train.rs:239-268), so the
     * statistic the densification threshold is compared with (train.rs:284-316, tuned for B = 1) would shrink B-fold:
     * pass B here to keep the reference's magnitude.  0 is read as 1. */
    float xy_stat_scale;
    /* Fused forms only (brush_render_backward_adam, brush_reduce_view_records_adam): NULL, or the deferred-Adam state
     * of the SH block.  The SH coefficients and moments of splats the view (no view of the batch) sees are then left
     * alone (their step stays pending); a seen splat's block first has its pending steps replayed, then takes this
     * step, and its sh_time becomes `time`.  Requires lazy_sh->now + 1 == time and 3 C floats per row a multiple of 4
     * (SH degree 1 or 3). */
    const BrushLazySh *lazy_sh;
} BrushAdamConfig;
/* One Adam step on all five parameter groups in one launch.  v_*: the gradient arrays of
 * brush_render_backward; moment1 / moment2: N*(11+3C) floats each, owned by the caller, laid out
 * [means 3N | log_scales 3N | quats 4N | raw_opac N | sh 3CN] and zero before the first step.
 * Parameters are updated in place.  Every optimizer entry point of this header computes the update as
 * x - lr (m rbc1) rcp(sqrt(v rbc2) + eps), rbc = 1 / (1 - beta^time) formed on the host, with v_sqrt_f32 / v_rcp_f32
 * (1 ulp each; WGSL, which the reference's optimizer runs in, allows 2.5 ulp on a division) and no FMA contraction:
 * from the same gradients the separate calls, the fused call and its deferred-SH form leave the same bits. */
int brush_adam_step(const BrushAdamConfig *cfg, uint32_t n, uint32_t sh_degree, float *means, float *log_scales,
                    float *quats, float *raw_opac, float *sh, const float *v_means, const float *v_scales,
                    const float *v_quats, const float *v_opac, const float *v_sh, float *moment1,
                    float *moment2, brush_stream_t stream);
/* brush_render_backward and brush_adam_step in one pass: the projection-backward kernel sends every
 * parameter-gradient element straight through the optimizer update instead of storing it, so the
 * dense gradients (52+12C bytes per splat) never travel to HBM and back.  Same arguments as the two
 * calls it replaces: `quats_fed` is the [N,4] array the forward was fed (rotation/|rotation| when
 * cfg->rotation_grad_wrt_normalized), `rotation` the raw parameter; means / log_scales / rotation /
 * raw_opacity / sh are updated in place, v_xy [N,2] is still written.  Optional outputs (NULL to
 * skip): next_quats_fed [N,4] = updated rotation / |rotation| (what the next forward is fed, saves
 * brush_normalize_quats; must not alias quats_fed); grad_2d_accum / xy_grad_counts [N] updated as
 * brush_refine_stats does.  Single-view training only: data-parallel training needs the gradients
 * (brush_render_backward). */
int brush_render_backward_adam(const BrushUniforms *uniforms, const BrushAux *aux, const BrushAdamConfig *cfg,
                               float *means, float *log_scales, const float *quats_fed, float *rotation,
                               float *raw_opacity, float *sh, uint32_t n, const float *out_img,
                               const float *v_out, float *v_xy, float *moment1, float *moment2,
                               float *next_quats_fed, float *grad_2d_accum, float *xy_grad_counts,
                               void *workspace, size_t workspace_bytes, brush_stream_t stream);
/* brush_render_backward_adam (eager or cfg->lazy_sh) that also writes the camera-pose gradient v_viewmat[12] of
 * brush_render_backward_pose, from the means as they were BEFORE this call's update (the pose kernels run ahead of the
 * kernel that steps them).  Parameters, moments and v_xy come out bit for bit as from brush_render_backward_adam. */
int brush_render_backward_adam_pose(const BrushUniforms *uniforms, const BrushAux *aux, const BrushAdamConfig *cfg,
                                    float *means, float *log_scales, const float *quats_fed, float *rotation,
                                    float *raw_opacity, float *sh, uint32_t n, const float *out_img,
                                    const float *v_out, float *v_xy, float *moment1, float *moment2,
                                    float *next_quats_fed, float *grad_2d_accum, float *xy_grad_counts,
                                    void *workspace, size_t workspace_bytes, float *v_viewmat, void *pose_workspace,
                                    size_t pose_workspace_bytes, brush_stream_t stream);
/* brush_reduce_view_records and brush_adam_step in one pass (data-parallel counterpart of
 * brush_render_backward_adam): the summed gradients go straight through the optimizer update, every rank applies
 * the same bits.  means / log_scales / rotation / raw_opacity / sh are updated in place (means is also the source
 * of the SH view directions: each splat is read before it is written).  width / height: image size of the
 * statistics (train.rs:300-302).  Optional (NULL to skip): next_quats_fed [N,4]; grad_2d_accum / xy_grad_counts
 * [N] += sum over views of the record's |v_xy * (w/2, h/2)| / number of views that saw the splat
 * (train.rs:284-316 for a batch of views). */
int brush_reduce_view_records_adam(const float *records, uint32_t num_views, uint32_t rows_per_view,
                                   const uint32_t *view_rows, const uint32_t *view_offsets, const float *campos,
                                   const BrushAdamConfig *cfg,
                                   uint32_t width, uint32_t height, float *means, float *log_scales, float *rotation,
                                   float *raw_opacity, float *sh, uint32_t n, uint32_t sh_degree, float *moment1,
                                   float *moment2, float *next_quats_fed, float *grad_2d_accum, float *xy_grad_counts,
                                   void *view_index, size_t view_index_bytes, brush_stream_t stream);
/* Applies every pending step of every splat's SH block (sh [N][C][3] and the two SH moment segments of `lazy`) and sets
 * sh_time[g] = lazy->now for all g: afterwards sh / moments are what the eager optimizer would hold.  Call it before
 * anything reads the coefficients without going through the op (export, refinement, a switch back to the eager step). */
int brush_lazy_sh_flush(const BrushLazySh *lazy, float *sh, uint32_t n, uint32_t sh_degree, brush_stream_t stream);
/* Host helper: rows [capacity][4] of BrushLazySh::table for optimizer times base+1 .. base+capacity, computed by the
 * code that turns BrushAdamConfig::time into the bias corrections of an eager step (so both use the same floats). */
int brush_lazy_sh_fill_table(float beta1, float beta2, float lr_coeffs_dc, float sh_rest_lerp, uint32_t base,
                             uint32_t capacity, float *host_rows);
/* normalized[i] = rotation[i] / |rotation[i]| (gaussian_splats.rs:174-175); [N,4], 16-byte aligned. */
int brush_normalize_quats(const float *rotation, float *normalized, uint32_t n, brush_stream_t stream);
/* train.rs:284-316: grad_2d_accum[g] += |v_xy[g] * (w/2, h/2)|; xy_grad_counts[g] += 1 for every
 * visible splat g of this view (both [N] f32). */
int brush_refine_stats(const BrushAux *h_aux, const float *v_xy, uint32_t n, uint32_t w, uint32_t h,
                       float *grad_2d_accum, float *xy_grad_counts, brush_stream_t stream);

/* ---- MCMC densification (Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo") ---------- */
/* The three per-splat kernels of the strategy (brush_amd/mcmc.py drives them).  All take a stream, allocate nothing,
 * never synchronise, use no atomics and can be captured into a graph; a zero count returns BRUSH_OK without touching the
 * pointers; a NULL or misaligned (floats: 4 bytes, rotation: 16 bytes) argument is BRUSH_ERR_INVALID_ARG. */
/* means[g] += Sigma_g (xi_g gate_g scale): Sigma = R diag(exp(2 log_scale)) R^T with R from rotation / |rotation|
 * ((w, x, y, z)), gate = 1 / (1 + exp(-100 ((1 - sigmoid(raw_opacity)) - 0.995))), scale = noise_lr * lr_mean of the step.
 * xi_g: three standard normals from Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) (seed: 64 bits, carried by the
 * ABI's one 64-bit scalar type) and counter (g, step, 0x4D434D43, 0): the output words x0..x3 give the uniforms
 * u_i = ((x_i >> 8) + 0.5) 2^-24 and xi = (r cos(2 pi u1), r sin(2 pi u1), sqrt(-2 ln u2) cos(2 pi u3)), r = sqrt(-2 ln u0).
 * A step is a pure function of (seed, step, g): repeatable bit for bit, whatever n and the other splats are.
 * xi_out: NULL, or [n,3] that receives xi.  Only means (and xi_out) is written. */
int brush_mcmc_inject_noise(float *means, const float *log_scales, const float *rotation, const float *raw_opacity,
                            uint32_t n, float scale, size_t seed, uint32_t step, float *xi_out, brush_stream_t stream);
/* Adds the gradients of opacity_reg * mean_g sigmoid(raw_g) and scale_reg * mean_{g,k} exp(log_scale_{g,k}) into the
 * dense gradient arrays of brush_render_backward, before brush_adam_step consumes them:
 * v_opac[g] += opacity_reg / n * s (1 - s), v_scales[g,k] += scale_reg / (3 n) * exp(log_scale).  The terms are formed
 * in float64 and each sum is rounded to f32 once; a weight of 0 leaves its array's bits alone. */
int brush_mcmc_reg_grads(const float *raw_opacity, const float *log_scales, uint32_t n, float opacity_reg,
                         float scale_reg, float *v_opac, float *v_scales, brush_stream_t stream);
/* Eq. 9 of the paper (gsplat's compute_relocation) on m gathered rows, each split into N = clamp(ratio, 1, 51) copies:
 * with o = sigmoid(raw), o' = 1 - (1 - o)^(1/N) and D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1),
 * log_scales_out = log_scales_in + ln(o / D) on all three axes and raw_opacity_out = logit(clamp(o', min_opacity,
 * 1 - 2^-24)) (the scale term uses the unclamped o').  Computed in float64 (the alternating sum cancels); the outputs
 * must not alias the inputs.  ratio: [m] int32. */
int brush_mcmc_relocation(const float *raw_opacity_in, const float *log_scales_in, const int32_t *ratio, uint32_t m,
                          float min_opacity, float *raw_opacity_out, float *log_scales_out, brush_stream_t stream);

/* ---- per-view exposure compensation (build extension; 3DGS's exposure compensation, gsplat's app_opt) ---------- */
/* A training view carries a 3x4 affine colour map E = [A | b], 12 floats row-major, identity [I | 0] at the start.  For
 * a rendered pixel p = (r, g, b, alpha) (premultiplied, as brush_render_forward writes it):
 *   out_c = A[c][0] r + A[c][1] g + A[c][2] b + alpha b_c  (c = 0..2)      out_alpha = alpha
 * which is A c + b on the un-premultiplied colour, premultiplied again: an uncovered pixel stays empty.  The loss is
 * taken on `out`; with v' = d L / d out the backward returns
 *   v_pred[k] = sum_c A[c][k] v'_c,  v_pred[alpha] = v'_alpha + sum_c b_c v'_c,
 *   v_exposure[c][k] = sum_pixels v'_c p_k (k = 0..2),  v_exposure[c][3] = sum_pixels v'_c alpha
 * the latter summed in float64 (every product exact) in a fixed order with no atomics and rounded to f32 once: the same
 * inputs give the same twelve words, all written on every call.  Images are [h][w][4] f32, 16-byte aligned, w h in
 * [1, 2^28).  `out` may not alias `pred` (the compositing backward needs the raw render); `v_pred` may alias `v_out`.
 * workspace: brush_exposure_workspace_size(w, h) bytes (8-byte aligned, at most 48 KiB), scratch, no state between
 * calls.  All pointers are device pointers except `cfg`.  No allocation, no synchronisation: graph-capturable. */
int brush_exposure_workspace_size(uint32_t w, uint32_t h, size_t *bytes);
int brush_exposure_forward(const float *pred, const float *exposure, uint32_t w, uint32_t h, float *out,
                           brush_stream_t stream);
int brush_exposure_backward(const float *pred, const float *v_out, const float *exposure, uint32_t w, uint32_t h,
                            float *v_pred, float *v_exposure, void *workspace, size_t workspace_bytes,
                            brush_stream_t stream);
/* brush_exposure_backward that also takes the Adam step of this view's E inside its last kernel: with G the float64
 * sums above, g = G + reg (E - [I|0]) (the coupled penalty), m1 = beta1 m1 + (1 - beta1) g, m2 = beta2 m2 + (1 - beta2) g^2,
 * E -= lr (m1 / (1 - beta1^time)) / (sqrt(m2 / (1 - beta2^time)) + epsilon), evaluated in float64 from the stored f32
 * words, each stored word rounded once.  time: the view's 1-based step count (0 is rejected).  exposure / moment1 /
 * moment2: this view's 12 words each, updated in place; v_pred uses E as it was before the step; v_exposure is written
 * as by brush_exposure_backward (before the penalty). */
typedef struct BrushExposureAdam {
    float lr, beta1, beta2, epsilon, reg;
    uint32_t time;
} BrushExposureAdam;
int brush_exposure_backward_adam(const float *pred, const float *v_out, const BrushExposureAdam *cfg, uint32_t w,
                                 uint32_t h, float *v_pred, float *exposure, float *moment1, float *moment2,
                                 float *v_exposure, void *workspace, size_t workspace_bytes, brush_stream_t stream);

/* ---- per-view bilateral grids (build extension; gsplat's use_bilateral_grid, Wang et al. 2024) ------------------- */
/* A training view carries a lattice grid[GL][GH][GW][12] f32, vertex-major, of the 3x4 affine colour maps above (identity
 * [I | 0] at every vertex at the start), 2 <= GW, GH <= 64, 2 <= GL <= 8.  Pixel (x, y) of a [h][w][4] premultiplied
 * render p = (r, g, b, alpha) reads it at (all f32, each operation rounded on its own, never contracted)
 *   w == 1: i0 = 0, fx = 0;  otherwise n = x (GW-1), i0 = min(n div (w-1), GW-2), fx = float(n - i0 (w-1)) / float(w-1)
 *   (y, h, GH give j0, fy the same way: align_corners, border clamp)
 *   lum = (0.299f r + 0.587f g) + 0.114f b;  lc = lum > 0 ? min(lum, 1) : 0 (a NaN gives 0);  z = lc float(GL-1),
 *   k0 = min((int) z, GL-2), fz = z - float(k0);  inside = lum > 0 && lum < 1
 * and with lerp(a, b, f) = a + f (b - a), per word, for k in {k0, k0+1}
 *   L_k = lerp(lerp(G[k][j0][i0], G[k][j0][i0+1], fx), lerp(G[k][j0+1][i0], G[k][j0+1][i0+1], fx), fy)
 *   M = lerp(L_k0, L_k0+1, fz)     S = L_k0+1 - L_k0
 *   out_c = ((M[4c] r + M[4c+1] g) + M[4c+2] b) + alpha M[4c+3]      out_alpha = alpha
 * The identity grid returns pred bit for bit; a grid whose vertices all hold E returns brush_exposure_forward's bits.
 * With v' = d L / d out the backward returns
 *   q = inside ? float(GL-1) ((t_0 + t_1) + t_2) : 0,  t_c = v'_c (((S[4c] r + S[4c+1] g) + S[4c+2] b) + alpha S[4c+3])
 *   v_pred.r = ((M[0] v'_0 + M[4] v'_1) + M[8] v'_2) + 0.299f q  (g, b: words 1 / 2, 0.587f / 0.114f)
 *   v_pred.alpha = v'_alpha + ((M[3] v'_0 + M[7] v'_1) + M[11] v'_2)
 *   v_grid[k][j][i][4c+m] = sum_pixels ((X Y) Z) (v'_c p_m)  (p_3 = alpha), X = 1 - fx at i = i0, fx at i = i0+1, 0
 *   elsewhere, Y and Z likewise: float64 from the f32 fractions, summed in float64 in a fixed order with no atomics
 *   and rounded to f32 once; a vertex no pixel reaches gets +0.  Every word of v_grid is written on every call.
 * Images are 16-byte aligned, sides <= 32768, w h in [1, 2^28); grid is 16-byte aligned.  `out` may not alias `pred`;
 * `v_pred` may alias `v_out`.  workspace: brush_bilagrid_workspace_size bytes (8-byte aligned), scratch, no state
 * between calls.  All pointers are device pointers except `cfg`.  No allocation, no synchronisation: graph-capturable,
 * and the same inputs give the same bits on every call. */
int brush_bilagrid_workspace_size(uint32_t w, uint32_t h, uint32_t gw, uint32_t gh, uint32_t gl, size_t *bytes);
int brush_bilagrid_forward(const float *pred, const float *grid, uint32_t gw, uint32_t gh, uint32_t gl, uint32_t w,
                           uint32_t h, float *out, brush_stream_t stream);
int brush_bilagrid_backward(const float *pred, const float *v_out, const float *grid, uint32_t gw, uint32_t gh,
                            uint32_t gl, uint32_t w, uint32_t h, float *v_pred, float *v_grid, void *workspace,
                            size_t workspace_bytes, brush_stream_t stream);
/* brush_bilagrid_backward that also takes the Adam step of this view's grid inside its last kernel, as
 * brush_exposure_backward_adam does for E, with the total-variation prior in place of the penalty: TV(G) = the sum over
 * the three axes of the mean, over all adjacent vertex pairs along the axis and all 12 words, of (G[v+e] - G[v])^2, and
 * g = v_grid's float64 sums + tv dTV/dG of the grid as it was BEFORE the step (taken in the launch that only reads the
 * grid).  grid / moment1 / moment2: this view's GL GH GW 12 words each, updated in place; v_pred uses the grid as it
 * was before the step; v_grid is written as by brush_bilagrid_backward (before the prior). */
typedef struct BrushBilagridAdam {
    float lr, beta1, beta2, epsilon, tv;
    uint32_t time;
} BrushBilagridAdam;
int brush_bilagrid_backward_adam(const float *pred, const float *v_out, const BrushBilagridAdam *cfg, uint32_t gw,
                                 uint32_t gh, uint32_t gl, uint32_t w, uint32_t h, float *v_pred, float *grid,
                                 float *moment1, float *moment2, float *v_grid, void *workspace, size_t workspace_bytes,
                                 brush_stream_t stream);

/* ---- background colour and loss masks (build extension; gsplat's backgrounds / masks, nerfstudio's mask_path) ----- */
/* Two element-wise maps that sit directly in front of the colour loss and behind it.  The op renders a premultiplied
 * image with no background; a trainer composes it, and the straight-alpha target, over a background colour b, and
 * leaves out the pixels a mask rules out.
 *   pred [h][w][4] f32: the premultiplied render, alpha = pred.w.
 *   gt   [h][w][Cg], Cg = gt_channels = 3 or 4, STRAIGHT alpha: u8 (BRUSH_EVAL_GT_U8, read as (float)b / 255.0f with an
 *        IEEE division) or f32 (BRUSH_EVAL_GT_F32, read as stored).
 *   mask [h][w] u8 or NULL: a pixel is KEPT when mask == NULL or mask[p] != 0 (COLMAP's and nerfstudio's convention).
 *   background: a DEVICE pointer to 3 f32, or NULL.  It lives on the device so that a colour drawn per step costs no
 *        upload and no synchronisation, and the call stays graph-capturable.
 * At least one of mask and background must be given.  Every operation below is one f32 operation rounded on its own
 * (never contracted).  Forward, with a background (out_gt then has 3 channels):
 *   t = 1.0f - alpha;   out_pred.c = pred.c + t * b_c  (c = 0..2);   out_pred.w = alpha
 *   Cg == 4:  s = 1.0f - G_a;   out_gt.c = G_c * G_a + s * b_c            Cg == 3:  out_gt.c = G_c
 * and without one (out_gt then has Cg channels): out_pred = pred, bits kept; out_gt.k = G_k.  A pixel that is not kept
 * is +0.0f in every word of out_pred and out_gt, by selection and not by multiplication: a NaN under the mask does not
 * leak.  The colour loss runs on (out_pred, out_gt); brush_compose_backward turns its v_out = d L / d out_pred into the
 * gradient at pred:
 *   kept:      v_pred.c = v_out.c;   v_pred.w = v_out.w - ((b_0 v_0 + b_1 v_1) + b_2 v_2)   (v_out.w without a background)
 *   not kept:  +0.0f in all four words
 * v_pred may alias v_out.  out_pred may not alias pred (the compositing backward needs the raw render), and out_gt may
 * alias neither gt nor out_pred.
 * Consequences: with a background the target is opaque RGB, so brush_l1_ssim_loss* then runs with gt_channels = 3 and
 * alpha is not compared, as in gsplat.  The L1 mean stays over all w h pixels: masked pixels contribute 0 to L1 and a
 * constant to SSIM, which is nerfstudio's (pred * mask, gt * mask) and the convention brush_depth_loss already has.
 * All pointers are device pointers; the four images are 16-byte aligned, background 4-byte; w h in [1, 2^28).  A NULL
 * required pointer, a misaligned one, both options NULL, any other gt_dtype / gt_channels or size returns
 * BRUSH_ERR_INVALID_ARG, checked before any GPU call.  No workspace, no allocation, no synchronisation:
 * graph-capturable; the same inputs give the same bits on every call. */
int brush_compose_forward(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t gt_channels,
                          const uint8_t *mask, const float *background, uint32_t w, uint32_t h,
                          float *out_pred, float *out_gt, brush_stream_t stream);
int brush_compose_backward(const float *v_out, const uint8_t *mask, const float *background,
                           uint32_t w, uint32_t h, float *v_pred, brush_stream_t stream);

/* ---- depth supervision (build extension; the 3DGS trainer's depth regulariser, gsplat's depth_loss) ------------- */
/* An L1 loss between the rendered expected depth and a per-view depth map, and both of its gradients, in one pass.
 * Per pixel p: a = pred[p].w, the alpha of the raw render pred [h][w][4] f32 (brush_render_forward_depth's image);
 * D = depth[p], its accumulated depth sum T alpha z, [h][w] f32; raw = target[p], [h][w] u16 (BRUSH_DEPTH_GT_U16, e.g.
 * a 16-bit PNG kept on the device as decoded) or f32 (BRUSH_DEPTH_GT_F32), and t = raw * scale + offset (an f32
 * multiply, then an f32 add: a millimetre u16 map is scale = 0.001).  The target is given in the space of the loss
 * (a depth for BRUSH_DEPTH_LOSS_DEPTH, an inverse depth for BRUSH_DEPTH_LOSS_DISPARITY).  A pixel is valid when the
 * target is present (u16: raw != 0; f32: raw finite and > 0), t > 0, D > 0 and a >= alpha_min.  With
 * c = (float)(weight / (w h)) formed in double precision, g = c sign(r), sign(0) = 0, and IEEE divisions:
 *   BRUSH_DEPTH_LOSS_DEPTH      d = D / a,  r = d - t,  v_D = g / a,         v_a = -(g d) / a
 *   BRUSH_DEPTH_LOSS_DISPARITY  q = a / D,  r = q - t,  v_D = -(g q) / D,    v_a = g / D
 * The loss is c sum_valid |r|: the mean runs over ALL w h pixels, as the 3DGS trainer's depth term does, not over the
 * valid ones; that is what lets the gradient be written in the pass that computes the sum (the valid fraction is
 * returned beside it for callers who want the other mean).
 * Outputs: v_depth [h][w] (NULL to skip) is written at every pixel, 0 where invalid.  v_a is ADDED into v_pred[p].w,
 * v_pred [h][w][4] (NULL to skip) being the gradient the colour loss has already written (stream order); its r, g, b
 * words and every word of an invalid pixel keep their bits.  stats[0] = (float)((double) c * sum (double) |r|), the sum
 * taken in float64 in a fixed order without atomics; stats[1] = (float)(valid pixels / (w h)), from an exact count.  A
 * non-NULL loss_accum receives *loss_accum += stats[0] (one f32 add), so a per-step loss log holds the total.
 * pred / v_pred: 16-byte aligned and distinct; w h in [1, 2^28); alpha_min > 0; any other mode / gt_dtype, a NULL
 * required pointer or a misaligned one is BRUSH_ERR_INVALID_ARG, checked before any GPU call.  workspace:
 * brush_depth_loss_workspace_size(w, h) bytes (8-byte aligned, at most 16 KiB), scratch, no state between calls.  All
 * pointers are device pointers except `cfg`.  No allocation, no synchronisation: graph-capturable; the same inputs give
 * the same bits on every call. */
#define BRUSH_DEPTH_LOSS_DEPTH 0u
#define BRUSH_DEPTH_LOSS_DISPARITY 1u
#define BRUSH_DEPTH_GT_U16 0u
#define BRUSH_DEPTH_GT_F32 1u
typedef struct BrushDepthLoss {
    float weight, scale, offset, alpha_min;
    uint32_t mode, gt_dtype;
} BrushDepthLoss;
int brush_depth_loss_workspace_size(uint32_t w, uint32_t h, size_t *bytes);
int brush_depth_loss(const float *pred, const float *depth, const void *target, const BrushDepthLoss *cfg, uint32_t w,
                     uint32_t h, float *v_depth, float *v_pred, float *stats, float *loss_accum, void *workspace,
                     size_t workspace_bytes, brush_stream_t stream);

/* ---- device image pyramid (build extension; nerfstudio's num_downscales, Mip-Splatting's multi-scale eval) -------- */
/* brush_area_resize_u8: an exact area (box) filter on an interleaved u8 image src [h][w][channels], channels 3 or 4,
 * every channel on its own (alpha like the others), to dst [oh][ow][channels] for any 1 <= ow <= w, 1 <= oh <= h.
 * Defined in integers: with x in units where a source pixel is ow wide and an output pixel w wide (y: oh and h),
 *   wx(X,s) = max(0, min((X+1) w, (s+1) ow) - max(X w, s ow)),  wy(Y,r) the same with h and oh,  D = w h,
 *   dst[Y][X][c] = floor((sum_r sum_s wy(Y,r) wx(X,s) src[r][s][c] + floor(D / 2)) / D).
 * One rounding, at the end, and no floating point: an even-sized image halved is (a + b + c + d + 2) >> 2, ow = w and
 * oh = h is the identity, a constant image stays constant.  The sum is held in 32 bits while 255 D + D / 2 < 2^32 and
 * in 64 bits above; both divide exactly.
 * brush_nearest_resize: dst[Y][X] = src[min(((2Y+1) h) / (2 oh), h-1)][min(((2X+1) w) / (2 ow), w-1)] on [h][w]
 * elements of elem_bytes = 2 (u16) or 4 (f32, moved as bits), the rule of the dataset reader for depth maps: a "no
 * measurement" zero never blends into its neighbours.  src / dst aligned to elem_bytes.
 * Both: a NULL pointer, a zero size, ow > w or oh > h, a side above 16384, channels not in {3, 4}, elem_bytes not in
 * {2, 4} or overlapping src / dst ranges return BRUSH_ERR_INVALID_ARG and write nothing, checked before any GPU call.
 * Device pointers.  No workspace, no allocation, no synchronisation, no atomics: graph-capturable; the same inputs give
 * the same bits on every call. */
int brush_area_resize_u8(const uint8_t *src, uint32_t w, uint32_t h, uint32_t channels, uint8_t *dst, uint32_t ow,
                         uint32_t oh, brush_stream_t stream);
int brush_nearest_resize(const void *src, uint32_t elem_bytes, uint32_t w, uint32_t h, void *dst, uint32_t ow,
                         uint32_t oh, brush_stream_t stream);

/* ---- undistortion of COLMAP views (build extension; COLMAP's image_undistorter is the model) ---------------------- */
/* Resamples a distorted w x h source into an ow x oh pinhole image.  All float operations are float32, round to
 * nearest, never contracted; pixel centres are at +0.5.  For output pixel (X, Y):
 *   x  = ((float)X + 0.5f - ocx) * iofx            y likewise
 *   r2 = x*x + y*y
 *   num = 1 + r2*(k1 + r2*(k2 + r2*k3))            den = 1 + r2*(k4 + r2*(k5 + r2*k6))
 *   rad = num / den                                 (always divided; IEEE division)
 *   a  = x*y
 *   xd = x*rad + ((2*p1)*a + p2*(r2 + (2*x)*x))
 *   yd = y*rad + (p1*(r2 + (2*y)*y) + (2*p2)*a)
 *   u  = (fx*xd + cx) - 0.5f                        v = (fy*yd + cy) - 0.5f      (source index space)
 *   qx = (int32) rintf(u * 256.0f)                  qy likewise                  (Q8; NaN or |.| >= 2^30: invalid)
 * (fx, fy, cx, cy): the source camera; (1 / iofx, 1 / iofy, ocx, ocy): the output camera, the host divides in float32;
 * k1..k6, p1, p2: OpenCV's rational model, a model's missing coefficients are zero (COLMAP's SIMPLE_RADIAL, RADIAL,
 * OPENCV and FULL_OPENCV).  A pixel is valid iff 0 <= qx <= (w-1) 256 and 0 <= qy <= (h-1) 256.
 * brush_undistort_u8: interleaved u8 src [h][w][channels], channels 3 or 4, to dst [oh][ow][channels]: x0 = qx >> 8,
 * ax = qx & 255, x1 = min(x0+1, w-1), the same in y, every channel on its own
 *   dst = (sum over the four taps of (256-ax | ax) (256-ay | ay) src + 32768) >> 16
 * (one rounding, in integers); an invalid pixel is 0 in every channel; `valid`, when not NULL, is a u8 [oh][ow] mask
 * that receives 1 for a valid pixel and 0 for an invalid one (it may overlap neither image).
 * brush_undistort_nearest: [h][w] elements of elem_bytes = 2 (u16) or 4 (f32, moved as bits) to [oh][ow]: the element
 * at ((qx+128)>>8, (qy+128)>>8), each clamped to the image; an invalid pixel is 0 ("no measurement"), and a zero never
 * blends into a neighbour.  src / dst aligned to elem_bytes.
 * Both: a NULL pointer (`valid` excepted), a zero size, a side above 8192 (beyond it float32 no longer resolves 1/256
 * px comfortably), channels not in {3, 4}, elem_bytes not in {2, 4} or overlapping ranges return BRUSH_ERR_INVALID_ARG
 * and write nothing, checked before any GPU call.  Device pointers except `map`.  No workspace, no allocation, no
 * synchronisation, no atomics: graph-capturable; the same inputs give the same bits on every call. */
typedef struct BrushUndistort {
    float fx, fy, cx, cy, iofx, iofy, ocx, ocy, k1, k2, k3, k4, k5, k6, p1, p2;
} BrushUndistort;
int brush_undistort_u8(const uint8_t *src, uint32_t w, uint32_t h, uint32_t channels, uint8_t *dst, uint32_t ow,
                       uint32_t oh, uint8_t *valid, const BrushUndistort *map, brush_stream_t stream);
int brush_undistort_nearest(const void *src, uint32_t elem_bytes, uint32_t w, uint32_t h, void *dst, uint32_t ow,
                            uint32_t oh, const BrushUndistort *map, brush_stream_t stream);

/* ---- rendered contribution of every splat (build extension; RadSplat's max blending weight, LightGaussian's summed
 *      weight) -------------------------------------------------------------------------------------------------- */
/* Replays the compositing walk of a FINISHED brush_render_forward / _depth / _rgba8 over the tile lists it left in the
 * aux (projected_splats, tile_bins, compact_gid_from_isect, global_from_compact_gid, num_visible; final_index with the
 * self-check) and accumulates, for every splat the walk meets, into the row of its GLOBAL id g:
 *   max_bits[g]   the bits of max over pixels of fac = alpha T, the weight the forward added the splat's colour with
 *                 (alpha after the 0.999 clamp, T the transmittance in front of it); a non-negative float, so the
 *                 integer max of the bits is the float max;
 *   counts[g][0]  sum_q24: the sum over pixels of (uint32) rint(fac 2^24), ties to even, as an exact integer;
 *                 sum_q24 / 2^24 is the summed weight to half a unit of 2^-24 per added pixel;
 *   counts[g][1]  hits: the number of pixels the forward added the splat to;
 *   counts[g][2]  stops: the number of pixels the splat ENDED without being added.
 * The stop quirk: an entry that passes `sigma >= 0 && alpha >= 1/255` and would take T to 1e-4 or below ends the pixel
 * and is not composited (rasterize.wgsl:88-91).  Such a splat has fac = 0 there, yet removing it changes the image (the
 * entries behind it would be tested against the same T), so it is counted on its own: a splat with hits == 0 and
 * stops == 0 in every view can be removed without changing one bit of any of those views.
 * Per pixel the walk repeats the forward's float operations, in both BRUSH_AUX_DETERMINISTIC settings and with
 * BRUSH_AUX_ANTIALIASED (word 8 of a projected row already holds the compensated opacity).  The entry only
 * ACCUMULATES: the caller zeroes max_bits [N] and counts [N][3] once and may keep them across views (max of maxima,
 * sums of sums).  All four outputs are order-independent integers: the same views give the same bits on every run.
 * Rows of splats the walk never meets (culled, or behind a stack that stopped every pixel of their quadrants first)
 * are not touched.
 * Self-check: out_img ([h,w,4] f32, the image of that forward) and mismatch ([1] u32) are both NULL or both given; with
 * them every pixel compares the bits of its replayed 1 - T with out_img[..., 3] and its last added entry with
 * final_index, and mismatch[0] += the number of pixels that differ (0 for a faithful replay; also accumulated).
 * A NULL required pointer, a misaligned one (out_img: 16 bytes, counts: 8) or tile_bounds that do not belong to img_size
 * return BRUSH_ERR_INVALID_ARG before any device work; n == 0 returns BRUSH_OK and launches nothing.  No workspace, no
 * allocation, no synchronisation: graph-capturable. */
int brush_render_contributions(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                               const float *out_img /* [h,w,4] or NULL */,
                               uint32_t *max_bits /* [N] */, uint64_t *counts /* [N,3]: sum_q24, hits, stops */,
                               uint32_t *mismatch /* [1] or NULL */, uint32_t n, brush_stream_t stream);

/* ---- per-splat image error (build extension; error-driven densification, Rota Bulo et al., "Revising Densification in
 *      Gaussian Splatting", ECCV 2024) ------------------------------------------------------------------------------ */
/* brush_l1_error_map: the per-pixel error the densification score distributes, one pass, a lane per pixel:
 *   out[p] = min(((|dr| + |dg|) + |db|) * (1.0f / 3.0f), 1.0f),   d = pred[p].rgb - gt[p].rgb
 * in exactly this association, every operation one f32 operation (no product feeds an add), so a float32 restatement
 * gives the same bits.  pred [h][w][4] f32 (channels 0..2 are used, as rendered); gt [h][w][Cg], Cg = gt_channels = 3 or
 * 4 (an alpha channel is not read), u8 (BRUSH_EVAL_GT_U8, read as (float)b / 255.0f with an IEEE division) or f32
 * (BRUSH_EVAL_GT_F32); mask [h][w] u8 or NULL: where mask[p] == 0, out[p] = +0.0f (by selection).  A NaN difference
 * gives 1.0f (fminf).  out [h][w] f32, row pitch w.  pred 16-byte aligned, an f32 gt and out 4-byte; w h in [1, 2^28).
 * brush_render_error_scores: replays the compositing walk of a FINISHED forward over the tile lists it left in the aux
 * (projected_splats, tile_bins, compact_gid_from_isect, global_from_compact_gid, num_visible: what
 * brush_render_contributions reads, without final_index) and distributes a per-pixel error to the splats by their
 * blending weights.  error_map [h][w] f32, row pitch w (NOT tile-padded), 4-byte aligned; every pixel reads its value
 * once and clamps it, e = min(max(E, 0), 1): a NaN and every negative value count as 0, everything above 1 as 1.  For
 * every splat the walk meets, into the row of its GLOBAL id g < n:
 *   view_err[g] += sum over the pixels the forward ADDED the splat to of (uint32) rint((fac e) 2^24)
 * with fac = alpha T as in brush_render_contributions (fac e: one f32 product; the scale is exact; ties to even), as
 * exact 64-bit integers: view_err / 2^24 is the splat's share of the view's summed error, "pixels of full error".  The
 * stop quirk is walked as the forward walks it (T evolves identically) and contributes nothing.  With an all-ones map
 * view_err is bit for bit counts[g][0] of brush_render_contributions.  The entry only ACCUMULATES into view_err [N]
 * (8-byte aligned), which the caller zeroes; the adds are order-independent integers, so the same inputs give the same
 * bits on every run, in both BRUSH_AUX_DETERMINISTIC settings and with BRUSH_AUX_ANTIALIASED.
 * Both: a NULL required pointer, a misaligned one, tile_bounds that do not belong to img_size or any other gt_dtype /
 * gt_channels return BRUSH_ERR_INVALID_ARG before any device work; brush_render_error_scores with n == 0 returns
 * BRUSH_OK and launches nothing.  Device pointers except the two structs.  No workspace, no allocation, no
 * synchronisation: graph-capturable. */
int brush_l1_error_map(const float *pred, const void *gt, uint32_t gt_dtype, uint32_t gt_channels,
                       const uint8_t *mask /* [h,w] or NULL */, float *out /* [h,w] */, uint32_t w, uint32_t h,
                       brush_stream_t stream);
int brush_render_error_scores(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                              const float *error_map /* [h,w] */, uint64_t *view_err /* [N] */, uint32_t n,
                              brush_stream_t stream);

/* ---- median depth and the splat under a pixel (build extension; the depth 2DGS, GOF, RaDe-GS and gsplat's 2DGS path
 *      fuse into their meshes) -------------------------------------------------------------------------------------- */
/* Replays the compositing walk of a FINISHED brush_render_forward_depth over the tile lists it left in the aux
 * (projected_splats, tile_bins, compact_gid_from_isect, global_from_compact_gid, num_visible: what
 * brush_render_contributions reads, without final_index) and picks, per pixel, the MEDIAN entry: the first entry the
 * forward ADDED after which the transmittance is at or below t_level,
 *   next_T = T (1 - alpha) <= t_level,   t_level = 1.0f - level   (one f32 subtraction, on the host),
 * i.e. the splat at which the accumulated opacity 1 - T first reaches `level` (0.5: the median).  The comparison is
 * `<=`: an entry that takes T to exactly t_level is the median.  An entry that ends the pixel without being added (the
 * stop quirk, rasterize.wgsl:88-91) is never the median, and a pixel keeps its FIRST crossing.  Per pixel the walk
 * repeats the forward's float operations, in both BRUSH_AUX_DETERMINISTIC settings and with BRUSH_AUX_ANTIALIASED (word
 * 8 of a projected row already holds the compensated opacity), so at level 0.5 a pixel has a median exactly where the
 * forward's alpha is >= 0.5.
 *   out_depth[p]  [h][w] f32: the bits of compact_depth[c] of the median entry's compact id c (compact_depth: what that
 *                 forward left, the camera-space z of every visible splat's mean), or 0.0f when no entry crosses;
 *   out_id[p]     [h][w] i32 or NULL: the median entry's GLOBAL id, or -1.
 * Every in-frame pixel is written on every call, empty tiles and n == 0 (no list is read then) included; nothing is
 * accumulated, every pixel has one writer: bitwise repeatable.  No interpolation between the entries around the
 * crossing, no gradient.  level must be finite with 0 < level < 1; a NULL required pointer, a pointer that is not
 * 4-byte aligned or tile_bounds that do not belong to img_size return BRUSH_ERR_INVALID_ARG before any device work.  No
 * workspace, no allocation, no synchronisation: graph-capturable. */
int brush_render_median_depth(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                              const float *compact_depth /* [N] */, float level, float *out_depth /* [h,w] */,
                              int32_t *out_id /* [h,w] or NULL */, uint32_t n, brush_stream_t stream);

/* ---- per-splat features through the compositing walk (build extension; gsplat's N-channel rasterisation is the model,
 *      LangSplat / Feature-3DGS / Gaussian Grouping / FlashSplat are the uses) ---------------------------------------- */
/* Three replays of the compositing walk of a FINISHED forward over the tile lists it left in the aux (projected_splats,
 * tile_bins, compact_gid_from_isect, global_from_compact_gid, num_visible: what brush_render_error_scores reads).  A
 * "hit" is an entry the forward ADDED to the pixel, fac = alpha T its blending weight; per pixel the walk repeats the
 * forward's float operations (the stop quirk included, which contributes nothing), in both BRUSH_AUX_DETERMINISTIC
 * settings and with BRUSH_AUX_ANTIALIASED.  C channels, 1 <= C <= BRUSH_FEATURE_MAX_CHANNELS, walked in passes of at most
 * 16 (one launch per pass).  The geometry is FROZEN: none of the three produces a gradient for it.
 * brush_render_features: features [N][C] f32, row-major, indexed by GLOBAL id; out [h][w][C] f32, pixel-major, row pitch
 *   w C (NOT tile-padded).  In list order every hit does out[p][c] = fmaf(features[g][c], fac, out[p][c]): the
 *   forward's own association, so the drawn colours (or compact_depth scattered to global ids) as features reproduce
 *   the forward's rgb (or out_depth) bit for bit.  Every in-frame pixel writes all C channels exactly once, +0.0f where
 *   nothing was added, empty tiles and n == 0 (no list is read then; features may be NULL) included.  No atomics:
 *   bitwise repeatable.
 * brush_render_features_backward: the transpose.  v_out [h][w][C] f32, arbitrary;
 *   v_features[g][c] += sum over the pixels p the forward added g to of fac v_out[p][c]
 *   with hardware float atomics, one instruction per (record, 8x8 quadrant, pass) on consecutive words of the row.  The
 *   entry only ACCUMULATES into v_features [N][C] f32, which the caller zeroes.  ORDER DEPENDENT in its last bits.
 * brush_render_feature_sums: the exact transpose of maps in [0, 1].  map_kind BRUSH_FEATURE_MAP_F32: maps [h][w][C] f32,
 *   every value clamped, m = min(max(M, 0), 1): a NaN and every negative value count as 0, everything above 1 as 1.
 *   BRUSH_FEATURE_MAP_LABEL_U8: maps [h][w] u8, channel c's map is `label == c`; a label >= C belongs to no class (255:
 *   "ignore").
 *   sums[g][c] += sum over the pixels the forward added g to of (uint32) rint((fac m[p][c]) 2^24)
 *   (fac m: one f32 product; the scale is exact; ties to even) as exact 64-bit integers, into sums [N][C] u64 (8-byte
 *   aligned), which the caller zeroes.  With C = 1 it is brush_render_error_scores bit for bit; a label image gives the
 *   bits of its one-hot f32 maps.  Order independent: the same inputs give the same bits on every run.
 * All three: a NULL required pointer, a misaligned one (f32: 4 bytes, sums: 8), C outside [1, 64], another map_kind or
 * tile_bounds that do not belong to img_size return BRUSH_ERR_INVALID_ARG before any device work; with n == 0 the
 * forward still writes zeros and the other two return BRUSH_OK and launch nothing.  Device pointers except the two
 * structs.  No workspace, no allocation, no synchronisation: graph-capturable. */
#define BRUSH_FEATURE_MAX_CHANNELS 64u
#define BRUSH_FEATURE_MAP_F32 0u
#define BRUSH_FEATURE_MAP_LABEL_U8 1u
int brush_render_features(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *features /* [N,C] */,
                          uint32_t C, float *out /* [h,w,C] */, uint32_t n, brush_stream_t stream);
int brush_render_features_backward(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                   const float *v_out /* [h,w,C] */, uint32_t C, float *v_features /* [N,C] */,
                                   uint32_t n, brush_stream_t stream);
int brush_render_feature_sums(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                              const void *maps /* [h,w,C] f32 or [h,w] u8 */, uint32_t map_kind, uint32_t C,
                              uint64_t *sums /* [N,C] */, uint32_t n, brush_stream_t stream);

/* ---- normal maps and the depth-normal consistency loss (build extension; 2DGS, GOF, RaDe-GS and PGSR are the models) - */
/* L_n = sum_i w_i (1 - n_i . N): n_i the normal of splat i, w_i = alpha_i T_i its blending weight, N the normal of the
 * surface the rendered depth map implies.  Rendered through brush_render_features (C = 3) on the per-splat normals, the
 * sum over the splats is A - Nr . N per pixel, A the alpha and Nr the rendered normal map of the same forward.
 * Every per-element result is defined operation by operation in f32 (one rounding per operation, no contraction, IEEE
 * division and square root); brush_amd/csrc/normal_loss.hip states the order once.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2,
 * W[r][c] = viewmat[4 c + r], t[r] = viewmat[12 + r] (column-major, as BrushUniforms stores it).
 * brush_splat_normals: normals_out [N][3] f32, every row written (splats that will not be visible too).  k = the index
 *   of the smallest log-scale (the lowest index among equals), a = column k of the rotation matrix of quats[g] (w, x, y,
 *   z: the unit quaternion the forward is fed), n_c = W a, p_c = W mean + t, s = dot(n_c, p_c) > 0 ? -1 : +1; the row is
 *   s n_c, a camera-space normal that faces the camera.
 * brush_splat_normals_backward: k and s recomputed, v_a = s W^T v_normals[g], the VJP of the rotation matrix with v_a
 *   in column k and zeros elsewhere is ADDED into v_quats [N][4]: the gradient at the 4-vector the forward was fed, the
 *   convention of brush_render_backward's v_quats (BrushAdamConfig::rotation_grad_wrt_normalized).  k and s are
 *   piecewise constant: nothing goes to the scales or the means.
 * Both: one lane per splat, n == 0 returns BRUSH_OK without reading the pointers (uniforms excepted).
 * brush_normal_loss: w, h, focal and pixel_center come from `uniforms`.  pred [h][w][4] f32 (alpha A read), depth
 *   [h][w] f32 (the accumulated depth D of brush_render_forward_depth), normals_img [h][w][3] f32 (Nr).  A pixel COUNTS
 *   when A >= alpha_min, D > 0 and both are finite; z = D / A, r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1),
 *   P = z r.  A pixel p is VALID when 1 <= x <= w - 2, 1 <= y <= h - 2, it and its four edge neighbours count and, with
 *   tx = P(x+1,y) - P(x-1,y), ty = P(x,y+1) - P(x,y-1), c = ty x tx (a fronto-parallel plane gives (0, 0, -1)), |c|^2
 *   is finite and > 0.  Nd = c / sqrt(|c|^2) -> depth_normals_out [h][w][3] (NULL to skip), zeros where invalid.
 *   l(p) = A(p) - Nr(p) . Nd(p); loss = kappa sum_valid l, kappa = (float)(weight / (w h)) formed in double: the mean
 *   runs over ALL pixels, as brush_depth_loss's.  stats[0] = (float)((double) kappa * sum (double) l), the sum in a fixed
 *   order without atomics; stats[1] = (float)(valid pixels / (w h)); a non-NULL loss_accum receives += stats[0].
 *   Gradients, each NULL to skip, every pixel of v_depth and v_normals_img written, zero outside their support:
 *     v_normals_img(p) = -kappa Nd(p);  v_Nd = -kappa Nr(p);  v_c = (v_Nd - Nd (Nd . v_Nd)) / |c|
 *     v_ty = tx x v_c,  v_tx = v_c x ty   (0 at invalid centres and off the frame)
 *     v_P(q) = ((v_tx(x-1,y) - v_tx(x+1,y)) + v_ty(x,y-1)) - v_ty(x,y+1)       a gather: no float atomics
 *     v_z(q) = v_P(q) . r(q);  v_depth(q) = v_z(q) / A(q) where q counts, else 0
 *     v_pred[q].w += kappa [q valid] - v_z(q) D(q) / A(q)^2   where q is valid or beside a valid centre; every other word
 *     of v_pred keeps its bits.
 *   normals_img == NULL is the normals-only form: depth_normals_out and stats = {0, valid fraction}; the gradient
 *   pointers and loss_accum must then be NULL.  pred / v_pred 16-byte aligned; no output may alias an input (the inputs
 *   are read across tile seams); alpha_min > 0; w h in [1, 2^28).  workspace: brush_normal_loss_workspace_size(w, h)
 *   bytes (8-byte aligned, at most 16 KiB), scratch.  Device pointers except `uniforms` and `cfg`.  No allocation, no
 *   synchronisation: graph-capturable; the same inputs give the same bits on every call. */
typedef struct BrushNormalLoss {
    float weight, alpha_min;
} BrushNormalLoss;
int brush_splat_normals(const BrushUniforms *uniforms, const float *means, const float *log_scales, const float *quats,
                        uint32_t n, float *normals_out /* [N,3] */, brush_stream_t stream);
int brush_splat_normals_backward(const BrushUniforms *uniforms, const float *means, const float *log_scales,
                                 const float *quats, uint32_t n, const float *v_normals /* [N,3] */,
                                 float *v_quats /* [N,4], accumulated into */, brush_stream_t stream);
int brush_normal_loss_workspace_size(uint32_t w, uint32_t h, size_t *bytes);
int brush_normal_loss(const BrushUniforms *uniforms, const float *pred, const float *depth, const float *normals_img,
                      const BrushNormalLoss *cfg, float *depth_normals_out, float *v_depth, float *v_normals_img,
                      float *v_pred, float *stats, float *loss_accum, void *workspace, size_t workspace_bytes,
                      brush_stream_t stream);

/* ---- depth-distortion term (build extension; 2DGS, GOF, RaDe-GS and gsplat's 2DGS path are the models) ---------- */
/* L(p) = sum over the unordered pairs (i, j) of the entries the forward added to pixel p of w_i w_j (m_i - m_j)^2, with
 * w_i = alpha_i T_i the blending weight, z_i = compact_depth[cgid_i] and m_i = mu(z_i):
 *   BRUSH_DISTORTION_DEPTH  mu(z) = z
 *   BRUSH_DISTORTION_NDC    mu(z) = far_z / (far_z - near_z) (1 - near_z / z), 0 < near_z < far_z finite   (2DGS's mapping)
 * All three entries replay a FINISHED brush_render_forward_depth (its uniforms, aux and compact_depth) on the forward's
 * own walk (0.999 clamp, 1/255 test, the `next_T <= 1e-4` stop without adding); brush_amd/csrc/distortion.hip states
 * the arithmetic.  Device pointers except `uniforms`, `aux` and `cfg`; no allocation, no synchronisation:
 * graph-capturable; n == 0 and empty lists are legal.
 * brush_render_distortion: stats [h][w][4] f32 (16-byte aligned) = (L, W, M1, M2) per pixel, the totals of L and of w,
 *   w c, w c^2 with c_i = m_i - m of the pixel's first entry (L does not change under a shift of every m).  Every pixel
 *   is written, zeros where nothing was added; no atomics, the same inputs give the same bits.
 * brush_distortion_compact_grads: the bare gradient launch.  v_distortion [h][w] f32 is the gradient at L(p), stats
 *   what brush_render_distortion wrote for the same cfg.  v_compact [n][16] f32, rows by COMPACT id in the layout of the
 *   compositing backward's accumulators, is ADDED into with float atomics: words 0, 1 (v_xy), 2-4 (v_conic), 8 (v_opacity
 *   of the drawn opacity) and 9 (v_z); words 5-7 and 10-15 and the rows of splats in no list keep their bits.  Nothing
 *   flows through an alpha the forward clamped at 0.999.  Order dependent in its last bits.
 * brush_render_backward_distortion: brush_render_backward_depth plus the term: the compositing backward as that entry
 *   runs it, brush_distortion_compact_grads on the workspace's compact rows, then the unchanged parameter backward, so
 *   means, scales, rotations, opacities (the antialiased compensation too) receive the term's gradient; v_sh receives
 *   none.  compact_depth and v_depth are required (a zero map if nothing else supervises the depth).  Same workspace,
 *   same aliasing rules and same outputs as brush_render_backward_depth.
 * BRUSH_AUX_DETERMINISTIC: both gradient entries return BRUSH_ERR_INVALID_ARG (that mode keeps one row per intersection
 *   and sums them in a fixed order: there is no compact row to add into). */
#define BRUSH_DISTORTION_DEPTH 0u
#define BRUSH_DISTORTION_NDC 1u
typedef struct BrushDistortion {
    uint32_t mode;
    float near_z, far_z; /* NDC mode only */
} BrushDistortion;
int brush_render_distortion(const BrushUniforms *uniforms, const BrushAux *aux, const float *compact_depth,
                            const BrushDistortion *cfg, uint32_t n, float *stats /* [h,w,4] */, brush_stream_t stream);
int brush_distortion_compact_grads(const BrushUniforms *uniforms, const BrushAux *aux, const float *compact_depth,
                                   const BrushDistortion *cfg, const float *stats, const float *v_distortion /* [h,w] */,
                                   uint32_t n, float *v_compact /* [n][16], ADDED into */, brush_stream_t stream);
int brush_render_backward_distortion(const BrushUniforms *uniforms, const BrushAux *aux, const float *means,
                                     const float *log_scales, const float *quats, const float *raw_opacity, uint32_t n,
                                     const float *out_img, const float *v_out, const float *compact_depth,
                                     const float *v_depth, const BrushDistortion *cfg, const float *stats,
                                     const float *v_distortion, float *v_means, float *v_xy, float *v_scales,
                                     float *v_quats, float *v_sh, float *v_opac, void *workspace, size_t workspace_bytes,
                                     brush_stream_t stream);

/* ---- 3D smoothing filter (build extension; Mip-Splatting, Yu et al. 2024, is the model) ------------------------- */
/* The world-space half of Mip-Splatting: every splat is low-passed at the highest rate any training view sampled it.
 * A splat carries a filter length f; the renderer sees the covariance Sigma + f^2 I and the opacity scaled by
 * sqrt(det Sigma / det(Sigma + f^2 I)).  With Sigma = R diag(s^2) R^T that is a map of the log-scales and the raw opacity
 * alone, so it sits in front of brush_render_forward and its transpose behind brush_render_backward; no other entry
 * point knows of it.  All three entries take a stream, allocate nothing, never synchronise, use no atomics and no
 * workspace and can be captured into a graph; n == 0 returns BRUSH_OK without touching the pointers; a NULL or
 * misaligned (floats: 4 bytes, view records: 16) argument is BRUSH_ERR_INVALID_ARG, checked before any GPU call. */
/* One pinhole view of brush_filter3d_rates, 96 bytes: the world-to-camera matrix column-major as BrushUniforms stores
 * it, the intrinsics in pixels and the image size. */
typedef struct BrushFilterView {
    float viewmat[16];
    float fx, fy, cx, cy;
    uint32_t width, height;
    uint32_t padding[2];
} BrushFilterView;
/* The number of view records brush_filter3d_rates stages in LDS at a time (tests straddle it). */
uint32_t brush_filter3d_view_chunk(void);
/* filter[i], the filter length of splat i from num_views views (a DEVICE array of records).  With p = W_v mean_i, rows
 * summed left to right ((m0 x + m1 y) + m2 z) + t, the pair (i, v) is valid when
 *   p.z > near_z,   -margin w <= (fx p.x) / p.z + cx <= (1 + margin) w,   -margin h <= (fy p.y) / p.z + cy <= (1 + margin) h
 * (Mip-Splatting: near_z 0.2, margin 0.15); nu_i = max over valid v of fx_v / p.z and filter[i] = sqrt(variance) / nu_i
 * (variance 0.2; the root is taken in float64 on the host and rounded once).  A splat no view sees takes the largest
 * length among the seen ones; when none is seen, or num_views == 0 (views may then be NULL), every length is 0.  Max
 * and min are float comparisons and nothing is summed across views: the result depends on neither the view order nor
 * the launch shape.  near_z, margin and variance must be finite and >= 0.  Two launches: one lane per splat with the
 * views staged through LDS, then one workgroup that finds the maximum and fills the unseen rows. */
int brush_filter3d_rates(const float *means, uint32_t n, const BrushFilterView *views, uint32_t num_views, float near_z,
                         float margin, float variance, float *filter, brush_stream_t stream);
/* The forward map, per splat, with s2_k = exp(2 log_scale_k) and f = filter[i] (det_expf / det_logf throughout):
 *   log_scales_out_k = 0.5 ln(s2_k + f^2)
 *   c = prod_k sqrt(s2_k / (s2_k + f^2)),   E = exp(-o),   D = (1 - c) + E
 *   raw_opacity_out = logit(sigmoid(o) c) = ln c - ln D
 * A row with f * f == 0 is copied through bit for bit.  Where c underflows to 0 the result is floored at
 * BRUSH_FILTER3D_MIN_RAW_OPACITY = ln 2^-126 (sigmoid of it is the smallest normal f32): a finite number, never NaN or
 * -inf.  o is read clamped to [-87, 87], so every finite input with log_scale <= 44 gives finite outputs.  The outputs
 * must not alias the inputs. */
#define BRUSH_FILTER3D_MIN_RAW_OPACITY (-87.33654f)
int brush_filter3d_apply(const float *log_scales, const float *raw_opacity, const float *filter, uint32_t n,
                         float *log_scales_out, float *raw_opacity_out, brush_stream_t stream);
/* The transpose, in place on the dense gradients brush_render_backward left for the effective parameters; log_scales
 * and raw_opacity are the RAW parameters, from which c, E and D are recomputed by the forward's own function:
 *   v_scales_k = v_scales_k * s2_k / (s2_k + f^2) + v_opac * (f^2 / (s2_k + f^2)) * (1 + E) / D     (1 / (1 - p) = (1 + E) / D)
 *   v_opac     = v_opac * E / D                                                             ((1 - sigmoid(o)) / (1 - p))
 * f carries no gradient.  Rows with f * f == 0 keep their bits.  Where the forward's floor acted the gradient is that of
 * the unfloored map (finite: D >= exp(-87)), which keeps such a splat trainable. */
int brush_filter3d_backward(const float *log_scales, const float *raw_opacity, const float *filter, uint32_t n,
                            float *v_scales, float *v_opac, brush_stream_t stream);

/* ---- mesh export (build extension; KinectFusion's volumetric fusion, Curless & Levoy 1996, and the TSDF mesh
 *      exports of 2DGS / GOF / nerfstudio are the models) ------------------------------------------------------------ */
/* Rendered depth maps are fused into a dense truncated signed distance volume, and an indexed triangle mesh is cut
 * out of it by marching tetrahedra.  Every sum is an integer that one lane owns: no atomics, no float accumulation
 * across views, so a volume's bits depend on neither the view order, the views per launch nor the launch shape, and
 * the mesh arrays (not only the sets) are the same on every run.
 * The grid: nx ny nz voxels, each side in [1, BRUSH_TSDF_MAX_SIDE], nx ny nz <= BRUSH_TSDF_MAX_VOXELS, x fastest;
 * voxel (i, j, k) has the linear index (k ny + j) nx + i and its centre at origin + (idx + 0.5) voxel, in f32
 *   x = origin[0] + ((float)i + 0.5f) * voxel      (one product, one sum; y z likewise).
 * voxel and trunc must be finite and > 0.
 * The volume: BRUSH_TSDF_PLANES planes of nx ny nz 32-bit words each, one after the other (SoA, so that a wave reads
 * and writes whole lines of one plane), 16-byte aligned:
 *   plane 0  count      u32   the views that observed the voxel
 *   plane 1  sdf_sum    i32   the sum of their truncated distances, each quantised to [-32767, 32767]
 *   plane 2-4 rgb_sum   u32   the sums of the 8-bit colours the views near the surface saw (r, g, b)
 *   plane 5  rgb_count  u32   the number of those views
 * A fresh volume is all zero (the caller's memset). */
#define BRUSH_TSDF_MAX_SIDE 2048u
#define BRUSH_TSDF_MAX_VOXELS (1u << 28)
#define BRUSH_TSDF_PLANES 6u
#define BRUSH_TSDF_MAX_VIEWS 16u /* views of one brush_tsdf_integrate call */
typedef struct BrushTsdfGrid {
    float origin[3];
    float voxel;
    float trunc;
    uint32_t nx, ny, nz;
} BrushTsdfGrid;
/* What one view of brush_tsdf_integrate reads, all DEVICE pointers: the raw render img [h][w][4] f32 (premultiplied
 * colour and alpha, as brush_render_forward_depth leaves it; 16-byte aligned), its accumulated depth [h][w] f32 and a
 * mask [h][w] u8 or NULL (0 = ignore the pixel); h w are the sizes of the view's record. */
typedef struct BrushTsdfViewData {
    const float *img;
    const float *depth;
    const uint8_t *mask;
} BrushTsdfViewData;
/* Fuses num_views views, 1 <= num_views <= BRUSH_TSDF_MAX_VIEWS, into the volume with one launch: one lane owns one
 * voxel, reads its six words once, goes through the views in registers and writes the words it changed once.  views:
 * a DEVICE array of records (staged through LDS); h_data: a HOST array of the views' pointers (copied into the launch).
 * Per voxel centre x and view, every operation one f32 operation, no contraction, IEEE divisions:
 *   p = W x + t, rows summed as brush_filter3d_rates sums them;      skip unless p.z > near_z
 *   u = (fx p.x) / p.z + cx,   v = (fy p.y) / p.z + cy
 *   pixel (floorf(u), floorf(v));                                     skip unless 0 <= floor u < w, 0 <= floor v < h
 *                                                                     skip if the mask is 0 there
 *   a = img.w;                                                        skip unless a >= alpha_min
 *   d = depth / a;                                                    skip unless 0 < d <= max_depth
 *   s = d - p.z;                                                      skip unless s >= -trunc
 *   count += 1;   sdf_sum += (int) rintf(fminf(1.0f, s / trunc) * 32767.0f)
 *   if |s| <= trunc:   rgb_sum[c] += (uint) rintf(255.0f * fminf(fmaxf(img[c] / a, 0.0f), 1.0f));   rgb_count += 1
 * so free space in front of a surface is carved (+32767 per view) and space more than trunc behind it stays
 * unobserved.  alpha_min must be finite and > 0, near_z finite and >= 0, max_depth > 0 (+inf: no limit).  A NULL
 * required pointer, a misaligned one, a grid over the limits, a bad scalar or a view count outside its range return
 * BRUSH_ERR_INVALID_ARG before any device work.  No workspace, no allocation, no synchronisation. */
int brush_tsdf_integrate(const BrushTsdfGrid *h_grid, uint32_t *volume, const BrushFilterView *views,
                         const BrushTsdfViewData *h_data, uint32_t num_views, float alpha_min, float max_depth,
                         float near_z, brush_stream_t stream);
/* brush_tsdf_integrate with flags.  BRUSH_TSDF_DEPTH_METRIC: the view's depth map already holds a distance per pixel
 * (a median depth map of brush_render_median_depth), so the line above reads
 *   d = depth                                                         skip unless 0 < d <= max_depth
 * and nothing else changes: the pixel is still used only where a = img.w >= alpha_min, and the colour is img[c] / a.
 * flags == 0 is brush_tsdf_integrate bit for bit (which forwards here); any other bit returns BRUSH_ERR_INVALID_ARG
 * before any device work. */
#define BRUSH_TSDF_DEPTH_METRIC 1u
int brush_tsdf_integrate_ex(const BrushTsdfGrid *h_grid, uint32_t *volume, const BrushFilterView *views,
                            const BrushTsdfViewData *h_data, uint32_t num_views, float alpha_min, float max_depth,
                            float near_z, uint32_t flags, brush_stream_t stream);
/* The mesh: marching tetrahedra on the lattice of voxel centres.  A cell is the cube between lattice point (i, j, k)
 * and (i+1, j+1, k+1), corner c = bit 0: +x, bit 1: +y, bit 2: +z; it is cut into the six tetrahedra of the Kuhn
 * decomposition around the diagonal corner 0 - corner 7: tetrahedron number t = 0..5 is (0, 1 << a, 1 << a | 1 << b,
 * 7) for the t-th permutation (a, b, c) of the axes in lexicographic order.  The decomposition is the same in every
 * cell, so neighbours agree on the face diagonals and the surface has no cracks.  A lattice point is VALID when
 * count >= min_views and INSIDE when sdf_sum < 0 (0 is outside).  Every lattice point owns the 7 edges to the points
 * at offset code e + 1 (bits as the corners), e = 0..6 its SLOT; an edge is ACTIVE when its far end is in the grid,
 * both ends are valid and exactly one is inside.  Vertices: one per active edge, ordered by owner's linear index,
 * then slot.  With m = (float)sdf_sum / (float)count at both ends and w = m0 / (m0 - m1):
 *   x = fmaf(((float)i + 0.5f) + w * (float)di, voxel, origin[0])    (y z likewise; the one fused operation: a vertex
 *                                                                     is then within 1 ulp or so of its exact position)
 *   colour[c] = (u8) rintf(fminf(fmaxf(c0 + w * (c1 - c0), 0), 255)),  c_e = (float)rgb_sum[c] / (float)rgb_count
 * where an end with rgb_count == 0 takes the other end's colour and two such ends give 128.  Faces: a cell takes part
 * when its 8 corners are valid; faces are ordered by cell (the linear index of its corner 0), then tetrahedron, then
 * triangle.  Of a tetrahedron (t0, t1, t2, t3) with inside vertices I and outside vertices O, both ascending in the
 * position within the tetrahedron, and (p, q) the vertex on the edge between p and q:
 *   |I| = 1: (i, o0) (i, o1) (i, o2)         |I| = 3: (i0, o) (i1, o) (i2, o)
 *   |I| = 2: (i0, o0) (i0, o1) (i1, o1)  and  (i0, o0) (i1, o1) (i1, o0)
 * and the last two vertices of a triangle are swapped when its normal at the edge midpoints points from the outside
 * vertices' centroid to the inside ones': normals point towards positive distance, at the cameras.  The table of the
 * 6 x 16 cases is generated from this rule at compile time.
 * brush_tsdf_mesh_count: four launch groups — the edge masks and counts per lattice point, their scan, the triangle
 * counts per cell, their scan — and totals[0] = V, totals[1] = F (DEVICE, 2 words), which the caller reads back to
 * size the outputs.  brush_tsdf_mesh_emit, with the SAME grid, volume, min_views and workspace contents: the vertex
 * kernel and the face kernel.  vertices [V][3] f32, colors [V][3] u8, faces [F][3] u32, all device; V == 0 or F == 0
 * skips that launch (the pointers may then be NULL).  The workspace (brush_tsdf_mesh_workspace_size, 256-byte aligned)
 * carries the masks and offsets from count to emit.  min_views >= 1.  Invalid arguments as above; a small workspace is
 * BRUSH_ERR_WORKSPACE_SMALL.  No allocation, no synchronisation. */
int brush_tsdf_mesh_workspace_size(uint32_t nx, uint32_t ny, uint32_t nz, size_t *bytes);
int brush_tsdf_mesh_count(const BrushTsdfGrid *h_grid, const uint32_t *volume, uint32_t min_views, uint32_t *totals,
                          void *workspace, size_t workspace_bytes, brush_stream_t stream);
int brush_tsdf_mesh_emit(const BrushTsdfGrid *h_grid, const uint32_t *volume, uint32_t min_views, uint32_t num_vertices,
                         uint32_t num_faces, float *vertices, uint8_t *colors, uint32_t *faces, void *workspace,
                         size_t workspace_bytes, brush_stream_t stream);

/* ---- compressed splats: the chunk-quantised PLY layout, packed and unpacked on the device (build extension) ----- */
/* The layout other trainers and viewers exchange as "compressed PLY": the splats sorted along a Morton curve, cut into
 * chunks of BRUSH_SPLAT_CHUNK = 256 rows, each chunk with the min and max of nine quantities (18 floats:
 * min_x min_y min_z max_x max_y max_z, the same of the scales, the same of the colours), each splat as four 32-bit
 * words (position 11-10-11, rotation 2-10-10-10, scale 11-10-11, colour and opacity 8-8-8-8) plus one byte per
 * higher-order SH value.  16 B + 3K B per splat, K = 0, 3, 8, 15 at SH degree 0..3, against 236 B in float at degree 3.
 * Arithmetic: float32, every operation rounded on its own (no contraction), IEEE division and square root.  Every input
 * value v is read as v + 0.0f (so -0 and +0 pack alike).
 *   order      lo, hi = per-axis min, max of the means; q = 0 where hi == lo, else
 *              min(1023, (uint32)(((x - lo) / (hi - lo)) * 1024.0f)); key = spread(qz) << 2 | spread(qy) << 1 |
 *              spread(qx) (30-bit Morton code); a STABLE sort by key; rows 256 j .. 256 j + 255 form chunk j, the last
 *              chunk holds the remainder and its min / max run over its real rows only.
 *   quantities p = mean; s = clamp(log_scale, -20, 20); c = f_dc * 0.28209479177387814f + 0.5f.
 *   norm(v, lo, hi) = 0 if v <= lo, else 1 if v >= hi, else 0 if hi - lo < 1e-5f, else (v - lo) / (hi - lo)
 *   unorm(t, b)     = (uint32) min(2^b - 1, max(0, floor(t * (2^b - 1) + 0.5f)))
 *   position   unorm(nx, 11) << 21 | unorm(ny, 10) << 11 | unorm(nz, 11); scale: the same over s
 *   colour     unorm(nr, 8) << 24 | unorm(ng, 8) << 16 | unorm(nb, 8) << 8 | unorm(a, 8), a = 1 / (1 + det_expf(-raw))
 *   rotation   a = (w, x, y, z) / sqrt(((w w + x x) + y y) + z z), (1, 0, 0, 0) when the norm is zero or not finite;
 *              L = first index of the largest |a[i]|; all four negated if a[L] < 0; word = L, then for every i != L in
 *              rising order word = word << 10 | unorm(a[i] * 0.70710678f + 0.5f, 10)
 *   SH byte    min(255, max(0, floor((v / 8 + 0.5f) * 256))), stored channel-major: byte c K + (k - 1) of a row
 * Unpacking: t = code / (2^b - 1), value = lo * (1 - t) + hi * t; f_dc = (c - 0.5f) / 0.28209479177387814f;
 * raw_opacity = det_logf(a / (1 - a)) with a = clamp(code, 0.5, 254.5) / 255 (finite at codes 0 and 255); a stored
 * rotation component is (code / 1023 - 0.5f) * 1.41421356f and the largest sqrt(max(0, 1 - ((a a + b b) + c c))), put
 * back at index L; an SH value is ((byte + 0.5f) / 256 - 0.5f) * 8.
 *
 * Tensors are those of Splats: means [n,3], log_scales [n,3], rotation [n,4] (w, x, y, z; 16-byte aligned),
 * raw_opacity [n], sh_coeffs [n,(sh_degree+1)^2,3] (16-byte aligned at degrees 1 and 3, whose rows are read and
 * written as whole 16-byte words); sh_degree 0..3; n in [1, BRUSH_SPLAT_PACK_MAX].  All pointers are device pointers.
 * Anything else, a NULL or misaligned pointer returns BRUSH_ERR_INVALID_ARG before any GPU call.  All three entries
 * enqueue on `stream`, allocate nothing, synchronise nothing and use no atomics: the same inputs give the same bits.
 *
 * brush_splat_pack_keys: keys[n] and vals[n] (= 0 .. n-1) ready for brush_radix_argsort_u32 with sorting_bits = 30 and
 * d_n = state; state[0] = n, state[1] = 1 when any word of any of the five tensors is an infinity or a NaN, else 0.
 * workspace: brush_splat_pack_workspace_size(n) bytes, 256-byte aligned (the partial bounds).
 * brush_splat_pack: `order` [n] is the sorted vals (row i of the output is input splat order[i]).  One workgroup per
 * chunk.  chunks [C][18], C = ceil(n / 256); words [256 C][4] (16-byte aligned) and sh_out [256 C][3K] u8 (4-byte
 * aligned; NULL at sh_degree_out 0) are allocated for whole chunks: the rows behind n are written as zeros, the SH bytes
 * of a chunk leave as whole 32-bit words.  sh_degree_out <= sh_degree drops the bands above it.
 * brush_splat_unpack: chunks [C][18], words [n][4] (16-byte aligned), sh_in [n][3K] u8 (4-byte aligned, n rows exactly)
 * into the five tensors, in packed order, sh_coeffs [n,(sh_degree+1)^2,3]. */
#define BRUSH_SPLAT_CHUNK 256u
#define BRUSH_SPLAT_PACK_MAX (1u << 30)
int brush_splat_pack_workspace_size(uint32_t n, size_t *bytes);
int brush_splat_pack_keys(const float *means, const float *log_scales, const float *rotation,
                          const float *raw_opacity, const float *sh_coeffs, uint32_t n, uint32_t sh_degree,
                          uint32_t *keys, uint32_t *vals, uint32_t *state, void *workspace, size_t workspace_bytes,
                          brush_stream_t stream);
int brush_splat_pack(const float *means, const float *log_scales, const float *rotation, const float *raw_opacity,
                     const float *sh_coeffs, uint32_t n, uint32_t sh_degree, uint32_t sh_degree_out,
                     const uint32_t *order, float *chunks, uint32_t *words, uint8_t *sh_out, brush_stream_t stream);
int brush_splat_unpack(const float *chunks, const uint32_t *words, const uint8_t *sh_in, uint32_t n, uint32_t sh_degree,
                       float *means, float *log_scales, float *rotation, float *raw_opacity, float *sh_coeffs,
                       brush_stream_t stream);

/* ---- opt-in stage timing ---------------------------------------------------------------- */
/* Counterpart of the reference's tracing spans + sync-span layer (render.rs:69-267,474-577;
 * crates/sync-span/src/lib.rs:12-49): when a profiler is attached to the calling host thread,
 * brush_render_forward / brush_render_backward record a hipEvent on `stream` after every
 * stage.  Nothing is recorded (and no event exists) when no profiler is attached, so the
 * default path stays free of events and synchronisation. */
typedef struct BrushProfiler BrushProfiler;
enum {
    BRUSH_STAGE_PROJECT_CULL = 0, /* init + ProjectSplats + compaction          (fwd) */
    BRUSH_STAGE_DEPTH_SORT,       /* radix argsort of depth keys                (fwd) */
    BRUSH_STAGE_PROJECT_VISIBLE,  /* ProjectVisible                             (fwd) */
    BRUSH_STAGE_PREFIX_SUM,       /* cum_tiles_hit                              (fwd) */
    BRUSH_STAGE_MAP_INTERSECTS,   /* MapGaussiansToIntersect                    (fwd) */
    BRUSH_STAGE_TILE_SORT,        /* radix argsort of tile ids                  (fwd) */
    BRUSH_STAGE_TILE_BINS,        /* GetTileBinEdges                            (fwd) */
    BRUSH_STAGE_RASTERIZE,        /* Rasterize                                  (fwd) */
    BRUSH_STAGE_BWD_ZERO,         /* zero compact-order accumulators            (bwd) */
    BRUSH_STAGE_RASTERIZE_BWD,    /* RasterizeBackwards                         (bwd) */
    BRUSH_STAGE_PROJECT_BWD,      /* GatherGrads + ProjectBackwards (fused)     (bwd) */
    BRUSH_NUM_STAGES
};
int brush_profiler_create(BrushProfiler **out);
void brush_profiler_destroy(BrushProfiler *p);
/* Attach (or detach with NULL) a profiler to the calling host thread. */
void brush_profiler_attach(BrushProfiler *p);
/* Blocks until the recorded events have completed, then writes the milliseconds spent in each
 * stage of the LAST forward and LAST backward call recorded (0 for stages not recorded). */
int brush_profiler_read(BrushProfiler *p, float *h_ms /* [BRUSH_NUM_STAGES] */);
/* Measurement only: while `p` is attached, brush_render_forward* / brush_render_backward* return BRUSH_OK right after
 * the launches of `stage` have been enqueued (later stages are not launched and their outputs stay untouched) and
 * record no events; stage = -1 restores the whole pass.  Timing the captured prefixes 0..k of a step and taking
 * differences gives every stage's time IN SITU, without the ~3-5 us an event record adds to each stage of an eager
 * pass (bench.py: `stage_ms`; the event times stay available as `stage_ms_events`). */
int brush_profiler_stop_after(BrushProfiler *p, int stage);
const char *brush_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* BRUSH_HIP_H */
