// view_records.hip — view-sharded data parallelism: per-view gradient records and their deterministic reduction.
//
// A view's parameter gradient is non-zero only for its visible splats and its SH row is rank one,
// v_sh[g] = Y(dir_view(g)) (x) v_rgb[g] (gather_grads.wgsl:186-222): kRecFloats floats per VISIBLE splat describe it,
//   [gid | v_means(3) | v_scales(3) | v_quats(4) | v_opac | v_rgb(3) | |v_xy * (w/2, h/2)|]          (64 bytes)
// k_project_backward_records writes them in compact (depth) order straight from the compositing backward's sums
// (no dense 52+12C bytes/splat arrays at all); the ranks all-gather the records of every view and
// k_reduce_view_records_*, one lane per GLOBAL splat id, adds the <= W records of its splat in view order 0..W-1.
// No atomics: the sum is the same bit pattern on every rank and from run to run, so replicated parameters stay
// replicated.  The sums leave as the single-view backward's do (grad_out.hpp): dense rows, or the per-wave Adam step.
// Compiled with -ffp-contract=off, like project_bwd.hip.  The reduction's ABI entries are at the end of this file
// (brush_render_backward_records: render_bwd.hip, on the backward's shared opening).
#include "det_sums.hpp"
#include "grad_out.hpp"
#include "render_host.hpp"
#include "splat_vjp.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRecFloats = 16;  // floats per record; word 0 = gid (k_build_view_index, sum_view_records)

__global__ __launch_bounds__(kThreads) void k_project_backward_records(
    ViewParams vp, const float *__restrict__ means, const float *__restrict__ log_scales,
    const float *__restrict__ quats, const float *__restrict__ raw_opac, const uint32_t *__restrict__ num_visible,
    const uint32_t *__restrict__ global_from_compact, const float *__restrict__ v_compact,
    float4 *__restrict__ records, uint32_t max_rows, float half_w, float half_h, DetSums det) {
    const uint32_t V = min(min(*num_visible, vp.total_splats), max_rows);
    for (uint32_t c = blockIdx.x * kThreads + threadIdx.x; c < V; c += gridDim.x * kThreads) {
        const uint32_t g = global_from_compact[c];
        float4 r0, r1, r2;
        load_compact_sums(v_compact, det, c, r0, r1, r2);
        const float vxy[2] = {r0.x, r0.y};
        const float vconic[3] = {r0.z, r0.w, r1.x};
        float mean[3], scale[3], quat[4];
        load_splat(means, log_scales, quats, g, mean, scale, quat);
        const float sg = det_sigmoid(raw_opac[g]);
        const float o_opac = r2.x * (sg * (1.0f - sg));  // gather_grads.wgsl:224-227
        float o_mean[3], o_scale[3], o_quat[4];
        splat_projection_vjp(vp, mean, scale, quat, vxy, vconic, o_mean, o_scale, o_quat);
        const float vx = vxy[0] * half_w, vy = vxy[1] * half_h;  // train.rs:300-302
        float4 *out = records + (size_t)c * (kRecFloats / 4);
        out[0] = make_float4(__uint_as_float(g), o_mean[0], o_mean[1], o_mean[2]);
        out[1] = make_float4(o_scale[0], o_scale[1], o_scale[2], o_quat[0]);
        out[2] = make_float4(o_quat[1], o_quat[2], o_quat[3], o_opac);
        out[3] = make_float4(r1.y, r1.z, r1.w, sqrtf(vx * vx + vy * vy));
    }
}

// index[v * n + gid] = row of splat gid in view v's records.  A reader validates an entry by checking
// row < view_rows[v] and records[v][row].gid == gid (a gid appears at most once per view), so stale or uninitialised
// entries are harmless; it clears the entries it consumes, so a buffer that started as all-ones stays clean and the
// check of an entry nobody wrote this step costs no gather.
__global__ __launch_bounds__(kThreads) void k_build_view_index(
    const float4 *__restrict__ records, uint32_t num_views, uint32_t rows_per_view, const uint32_t *__restrict__ view_rows,
    const uint32_t *__restrict__ view_offsets, uint32_t n, uint32_t *__restrict__ index) {
    // view_offsets == nullptr: view v owns rows [v * rows_per_view, + view_rows[v]); otherwise the views are packed,
    // view v owns rows [view_offsets[v], + view_rows[v]) of a buffer of rows_per_view rows in all.
    for (uint32_t v = 0; v < num_views; v++) {  // uniform: a handful of views
        const uint32_t first = view_offsets ? view_offsets[v] : v * rows_per_view;
        const uint32_t room = view_offsets ? (first < rows_per_view ? rows_per_view - first : 0u) : rows_per_view;
        const uint32_t cnt = min(view_rows[v], room);
        for (uint32_t r = blockIdx.x * kThreads + threadIdx.x; r < cnt; r += gridDim.x * kThreads) {
            const uint32_t gid = __float_as_uint(records[(size_t)(first + r) * (kRecFloats / 4)].x);
            if (gid < n) index[(size_t)v * n + gid] = r;
        }
    }
}

// The per-view sums of one splat (fixed view order: the same bits on every rank).  `add_sh(Y, v_rgb)` accumulates the
// splat's v_sh row wherever the caller keeps it (add_sh_row).  A consumed index entry is cleared, so a buffer that was
// all-ones before its first use stays free of stale entries (the record is still checked: correctness never depends on it).
struct ViewSums {
    float mean[3] = {0.f, 0.f, 0.f}, scale[3] = {0.f, 0.f, 0.f}, quat[4] = {0.f, 0.f, 0.f, 0.f};
    float opac = 0.f, stat_norm = 0.f, stat_count = 0.f;
};
template <uint32_t NCOEF>
__device__ __forceinline__ void add_sh_row(float *row, const float *Y, const float4 &v_rgb) {
#pragma unroll
    for (uint32_t k = 0; k < NCOEF; k++) {
        row[k * 3 + 0] += Y[k] * v_rgb.x;
        row[k * 3 + 1] += Y[k] * v_rgb.y;
        row[k * 3 + 2] += Y[k] * v_rgb.z;
    }
}
template <int DEG, typename AddSh>
__device__ __forceinline__ void sum_view_records(
    const float4 *__restrict__ records, uint32_t num_views, uint32_t rows_per_view, const uint32_t *__restrict__ view_rows,
    const uint32_t *__restrict__ view_offsets, const float *__restrict__ campos, uint32_t *__restrict__ index,
    const float *means, uint32_t n, uint32_t g, ViewSums &o, AddSh add_sh) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    constexpr uint32_t kChunk = 8;  // views whose index entries / record heads are in flight together
    const float mean[3] = {means[(size_t)g * 3], means[(size_t)g * 3 + 1], means[(size_t)g * 3 + 2]};
    for (uint32_t v0 = 0; v0 < num_views; v0 += kChunk) {
        // One memory phase for the index entries of up to 8 views, one for the heads of the records they point to
        // (round 2 walked the views one by one: two dependent loads per view, 117 us at 8 views where one view takes 43),
        // then the sums in view order: the same bits on every rank.
        uint32_t r[kChunk];
#pragma unroll
        for (uint32_t j = 0; j < kChunk; j++) r[j] = v0 + j < num_views ? index[(size_t)(v0 + j) * n + g] : kInvalid;
        const float4 *rec[kChunk];
        float4 a[kChunk];
#pragma unroll
        for (uint32_t j = 0; j < kChunk; j++) {
            const uint32_t v = v0 + j;
            rec[j] = nullptr;
            a[j] = make_float4(__uint_as_float(kInvalid), 0.f, 0.f, 0.f);
            if (v < num_views) {
                const uint32_t first = view_offsets ? view_offsets[v] : v * rows_per_view;
                const uint32_t room = view_offsets ? (first < rows_per_view ? rows_per_view - first : 0u) : rows_per_view;
                if (r[j] < min(view_rows[v], room)) {
                    rec[j] = records + ((size_t)first + r[j]) * (kRecFloats / 4);
                    a[j] = rec[j][0];
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kChunk; j++) {
            const uint32_t v = v0 + j;
            if (rec[j] == nullptr || __float_as_uint(a[j].x) != g) continue;  // no entry / stale index entry
            index[(size_t)v * n + g] = kInvalid;
            const float4 b = rec[j][1], c = rec[j][2], d = rec[j][3];
            o.mean[0] += a[j].y, o.mean[1] += a[j].z, o.mean[2] += a[j].w;
            o.scale[0] += b.x, o.scale[1] += b.y, o.scale[2] += b.z;
            o.quat[0] += b.w, o.quat[1] += c.x, o.quat[2] += c.y, o.quat[3] += c.z;
            o.opac += c.w;
            o.stat_norm += d.w;
            o.stat_count += 1.0f;
            // gather_grads.wgsl:182-222 with this view's camera term (viewmat[3].xyz)
            float dir[3] = {mean[0] - campos[v * 3], mean[1] - campos[v * 3 + 1], mean[2] - campos[v * 3 + 2]};
            const float len = sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
            dir[0] = dir[0] / len, dir[1] = dir[1] / len, dir[2] = dir[2] / len;
            float Y[ncoef];
            sh_basis<ncoef>(DEG, dir, Y);
            add_sh(Y, d);
        }
    }
}

// Fused with Adam: the summed rows go through the per-wave LDS staging of adam_step_wave.
template <int DEG>
__global__ __launch_bounds__(kThreads) void k_reduce_view_records_adam(
    const float4 *__restrict__ records, uint32_t num_views, uint32_t rows_per_view,
    const uint32_t *__restrict__ view_rows, const uint32_t *__restrict__ view_offsets,
    const float *__restrict__ campos, uint32_t *__restrict__ index, const float *means, uint32_t n, AdamFuse af) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    constexpr uint32_t kRow = ncoef * 3, kRowPad = kRow | 1u;
    constexpr uint32_t kStageFloats = (kWave * kRowPad > 512u ? kWave * kRowPad : 512u);
    __shared__ float stage_all[kThreads / kWave][kStageFloats];
    const uint32_t wv = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    float *stage = stage_all[wv];
    const uint32_t g0 = blockIdx.x * kThreads + wv * kWave;
    if (g0 >= n) return;  // wave-uniform; the kernel has no workgroup barrier
    const uint32_t g = g0 + lane;
    ViewSums o;
    float *row = stage + lane * kRowPad;
#pragma unroll
    for (uint32_t k = 0; k < kRow; k++) row[k] = 0.f;
    if (g < n)
        sum_view_records<DEG>(records, num_views, rows_per_view, view_rows, view_offsets, campos, index, means, n, g, o,
                              [&](const float *Y, const float4 &d) { add_sh_row<ncoef>(row, Y, d); });
    const float zero2[2] = {0.f, 0.f}, zero3[3] = {0.f, 0.f, 0.f};
    // deferred SH: a splat some view saw (stat_count != 0) has its block caught up and stepped, the others wait
    __shared__ uint32_t row_t0_all[kThreads / kWave][kWave];
    uint32_t *row_t0 = row_t0_all[wv];
    const bool seen = af.lazy.on() && g < n && o.stat_count != 0.0f;
    if (af.lazy.on()) {
        row_t0[lane] = seen ? af.lazy.sh_time[g] : kInvalid;
        __builtin_amdgcn_wave_barrier();
    }
    adam_step_wave<DEG, true>(af, n, g0, lane, stage, row_t0, o.mean, o.scale, o.quat, o.opac, zero2, o.stat_norm,
                              o.stat_count, nullptr, zero3, nullptr);
    if (seen) af.lazy.sh_time[g] = af.lazy.now + 1u;
}

// Dense sum: like the dense backward, the zeros of the splats no view sees are stored straight from registers by the
// lanes that own the addresses, and a splat some view sees keeps its v_sh row in registers and writes its rows itself.
template <int DEG>
__global__ __launch_bounds__(kThreads) void k_reduce_view_records_dense(
    const float4 *__restrict__ records, uint32_t num_views, uint32_t rows_per_view,
    const uint32_t *__restrict__ view_rows, const uint32_t *__restrict__ view_offsets,
    const float *__restrict__ campos, uint32_t *__restrict__ index, const float *means, uint32_t n,
    float *__restrict__ v_means, float *__restrict__ v_scales, float *__restrict__ v_quats, float *__restrict__ v_sh,
    float *__restrict__ v_opac) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    constexpr uint32_t kRow = ncoef * 3;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t g0 = blockIdx.x * kThreads + (threadIdx.x / kWave) * kWave;
    if (g0 >= n) return;  // wave-uniform; the kernel has no workgroup barrier
    const size_t g = (size_t)g0 + lane;
    ViewSums o;
    float row[kRow];
#pragma unroll
    for (uint32_t k = 0; k < kRow; k++) row[k] = 0.f;
    if (g < n)
        sum_view_records<DEG>(records, num_views, rows_per_view, view_rows, view_offsets, campos, index, means, n,
                              (uint32_t)g, o, [&](const float *Y, const float4 &d) { add_sh_row<ncoef>(row, Y, d); });
    const bool seen = o.stat_count != 0.0f;
    zero_invisible_rows<DEG>(n, g0, lane, __ballot(seen), v_means, nullptr, v_scales, v_quats, v_sh, v_opac);
    if (seen) {
        reinterpret_cast<float4 *>(v_quats)[g] = make_float4(o.quat[0], o.quat[1], o.quat[2], o.quat[3]);
        v_opac[g] = o.opac;
#pragma unroll
        for (int k = 0; k < 3; k++) v_means[g * 3 + k] = o.mean[k], v_scales[g * 3 + k] = o.scale[k];
        float *dst = v_sh + g * kRow;
        if constexpr (kRow % 4 == 0) {
#pragma unroll
            for (uint32_t j = 0; j < kRow / 4; j++)
                reinterpret_cast<float4 *>(dst)[j] = make_float4(row[4 * j], row[4 * j + 1], row[4 * j + 2], row[4 * j + 3]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < kRow; e++) dst[e] = row[e];
        }
    }
}

}  // namespace

hipError_t launch_project_backward_records(const ViewParams &vp, const float *means, const float *log_scales,
                                           const float *quats, const float *raw_opac, const uint32_t *num_visible,
                                           const uint32_t *global_from_compact, const float *v_compact,
                                           float *records, uint32_t max_rows, const DetSumsArgs &dargs, hipStream_t s) {
    if (vp.total_splats == 0 || max_rows == 0) return hipSuccess;
    const uint32_t rows = min(vp.total_splats, max_rows);
    const DetSums det = make_det_sums(dargs);
    hipLaunchKernelGGL(k_project_backward_records, dim3(min(ceil_div(rows, kThreads), 2048u)), dim3(kThreads), 0, s, vp,
                       means, log_scales, quats, raw_opac, num_visible, global_from_compact, v_compact,
                       reinterpret_cast<float4 *>(records), max_rows, (float)vp.img_size[0] / 2.0f,
                       (float)vp.img_size[1] / 2.0f, det);
    return hipGetLastError();
}

hipError_t launch_reduce_view_records(const float *records, uint32_t num_views, uint32_t rows_per_view,
                                      const uint32_t *view_rows, const uint32_t *view_offsets, const float *campos,
                                      const float *means, uint32_t n, uint32_t sh_degree, uint32_t *index,
                                      float *v_means, float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                      const AdamFuse *adam, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const float4 *rec4 = reinterpret_cast<const float4 *>(records);
    if (num_views > 0 && rows_per_view > 0)  // (a u32 product would wrap to 0 at 8 views x 2^29 rows and skip the index)
        hipLaunchKernelGGL(k_build_view_index, dim3(min(ceil_div(rows_per_view, kThreads), 2048u)), dim3(kThreads), 0, s,
                           rec4, num_views, rows_per_view, view_rows, view_offsets, n, index);
    const dim3 grid(ceil_div(n, kThreads)), block(kThreads);
    const AdamFuse af = adam ? *adam : AdamFuse{};
    dispatch_degree(sh_degree, [&](auto deg) {
        if (adam)
            hipLaunchKernelGGL(k_reduce_view_records_adam<deg()>, grid, block, 0, s, rec4, num_views, rows_per_view,
                               view_rows, view_offsets, campos, index, means, n, af);
        else
            hipLaunchKernelGGL(k_reduce_view_records_dense<deg()>, grid, block, 0, s, rec4, num_views, rows_per_view,
                               view_rows, view_offsets, campos, index, means, n, v_means, v_scales, v_quats, v_sh, v_opac);
    });
    return hipGetLastError();
}

}  // namespace brush

using namespace brush;

extern "C" int brush_view_index_size(uint32_t n, uint32_t num_views, size_t *bytes) {
    if (!bytes) return BRUSH_ERR_INVALID_ARG;
    *bytes = sizeof(uint32_t) * (size_t)(n ? n : 1) * (num_views ? num_views : 1);
    return BRUSH_OK;
}

static int reduce_views_impl(const float *records, uint32_t num_views, uint32_t rows_per_view, const uint32_t *view_rows,
                             const uint32_t *view_offsets, const float *campos, const float *means, uint32_t n,
                             uint32_t sh_degree, float *v_means, float *v_scales, float *v_quats, float *v_sh,
                             float *v_opac, const AdamFuse *adam, void *view_index, size_t view_index_bytes,
                             brush_stream_t stream) {
    if (sh_degree > 4 || num_views == 0) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;
    if (!means || !view_index || !view_rows || !campos || (rows_per_view > 0 && !records)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(records, 16)) return BRUSH_ERR_INVALID_ARG;
    if (!adam && (!v_means || !v_scales || !v_quats || !v_sh || !v_opac)) return BRUSH_ERR_INVALID_ARG;
    if (view_index_bytes < sizeof(uint32_t) * (size_t)n * num_views) return BRUSH_ERR_WORKSPACE_SMALL;
    if (!view_offsets && (uint64_t)num_views * rows_per_view > 0xFFFFFFFFull) return BRUSH_ERR_INVALID_ARG;
    BRUSH_HIP_CHECK(launch_reduce_view_records(records, num_views, rows_per_view, view_rows, view_offsets, campos, means, n,
                                               sh_degree, static_cast<uint32_t *>(view_index), v_means, v_scales, v_quats,
                                               v_sh, v_opac, adam, static_cast<hipStream_t>(stream)));
    return BRUSH_OK;
}

extern "C" int brush_reduce_view_records(const float *records, uint32_t num_views, uint32_t rows_per_view,
                                         const uint32_t *view_rows, const uint32_t *view_offsets, const float *campos,
                                         const float *means, uint32_t n, uint32_t sh_degree, float *v_means,
                                         float *v_scales, float *v_quats, float *v_sh, float *v_opac, void *view_index,
                                         size_t view_index_bytes, brush_stream_t stream) {
    return reduce_views_impl(records, num_views, rows_per_view, view_rows, view_offsets, campos, means, n, sh_degree, v_means,
                             v_scales, v_quats, v_sh, v_opac, nullptr, view_index, view_index_bytes, stream);
}

extern "C" int brush_reduce_view_records_adam(const float *records, uint32_t num_views, uint32_t rows_per_view,
                                              const uint32_t *view_rows, const uint32_t *view_offsets,
                                              const float *campos, const BrushAdamConfig *cfg, uint32_t width, uint32_t height,
                                              float *means, float *log_scales, float *rotation, float *raw_opacity,
                                              float *sh, uint32_t n, uint32_t sh_degree, float *moment1, float *moment2,
                                              float *next_quats_fed, float *grad_2d_accum, float *xy_grad_counts,
                                              void *view_index, size_t view_index_bytes, brush_stream_t stream) {
    AdamFuse af{};
    if (!fill_adam_fuse(cfg, means, log_scales, rotation, raw_opacity, sh, n, moment1, moment2, next_quats_fed,
                        grad_2d_accum, xy_grad_counts, width, height, sh_degree, &af))
        return BRUSH_ERR_INVALID_ARG;
    return reduce_views_impl(records, num_views, rows_per_view, view_rows, view_offsets, campos, means, n, sh_degree,
                             nullptr, nullptr, nullptr, nullptr, nullptr, &af, view_index, view_index_bytes, stream);
}
