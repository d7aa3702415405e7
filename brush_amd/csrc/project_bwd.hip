// project_bwd.hip — the single-view parameter backward: one launch over GLOBAL splat ids that turns the compositing
// backward's compact-order sums into parameter gradients (dense form) or straight into the Adam update (fused forms).
// Lane g looks up its compact id through the inverse map the forward produced; the visible splats of a workgroup are
// compacted to its first lanes, gather their compact-order gradients and run the per-splat VJP (splat_vjp.hpp; the sums
// come from det_sums.hpp).  How the results leave is grad_out.hpp's: dense rows, or the per-wave Adam step.
// Traffic per splat: 4 B (map) + 40 B params + 36 B compact grads (visible only) read, 52 + 12*C B written (dense):
// HBM-bound.  The per-view records of the data-parallel form and their reduction: view_records.hip.  Compiled with
// -ffp-contract=off (same expression trees as the forward projection).
#include "det_sums.hpp"
#include "grad_out.hpp"
#include "splat_vjp.hpp"
#include "trace.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_zero_compact_grads(const uint32_t *__restrict__ num_visible,
                                                                 uint32_t n, float4 *__restrict__ v_compact) {
    BRUSH_KTRACE(kTrZeroGrads, 0);
    const uint32_t V = min(*num_visible, n);
    BRUSH_KTRACE_MARK(1, V);
    const uint32_t words = V * (kCompactStride / 4);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x)
        v_compact[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(kThreads) void k_sum_isect_rows(
    const float4 *__restrict__ rows, const uint32_t *__restrict__ num_intersections,
    const uint32_t *__restrict__ cum_tiles_hit, uint32_t cap, float4 *__restrict__ v_compact, float4 *__restrict__ partials) {
    const uint32_t I = min(*num_intersections, cap);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t waves = gridDim.x * (kThreads / kWave);
    for (uint32_t k = blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; (uint64_t)k * kWave < I; k += waves) {
        const uint32_t base = k * kWave, u = base + lane;
        const bool valid = u < I;
        float v[12];
        uint32_t c = 0, first = lane, last = lane;
        bool starts_here = true, ends_here = true;
#pragma unroll
        for (uint32_t i = 0; i < 12; i++) v[i] = 0.f;
        if (valid) {
            const float4 a = rows[(size_t)u * kCompactVec], b = rows[(size_t)u * kCompactVec + 1], d = rows[(size_t)u * kCompactVec + 2];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w, v[8] = d.x;
            c = __float_as_uint(d.y);  // kIsectGidWord
            uint32_t u0, u1;
            isect_range(cum_tiles_hit, I, c, u0, u1);
            starts_here = u0 >= base;
            ends_here = u1 <= base + kWave;
            first = max(u0, base) - base;
            last = min(u1, base + kWave) - 1u - base;
        }
        // inclusive scan inside the segment [first, last] (lanes of one splat are contiguous)
#pragma unroll
        for (uint32_t dist = 1; dist < kWave; dist <<= 1) {
#pragma unroll
            for (uint32_t i = 0; i < kSumWords; i++) {
                const float up = __shfl_up(v[i], dist, 64);
                if (lane >= first + dist) v[i] += up;
            }
        }
        if (valid && lane == last) {
            float4 *dst = (starts_here && ends_here) ? v_compact + (size_t)c * kCompactVec
                                                     : partials + ((size_t)k * 2 + (starts_here ? 1 : 0)) * kCompactVec;
            dst[0] = make_float4(v[0], v[1], v[2], v[3]);
            dst[1] = make_float4(v[4], v[5], v[6], v[7]);
            dst[2] = make_float4(v[8], 0.f, 0.f, 0.f);
        }
    }
}

// ---- accumulated depth (brush_render_backward_depth) -------------------------------------------------------------------
// v_z of a visible splat: kCompactDepthWord of its compact row; in deterministic mode the compositing backward leaves it
// in kIsectDepthWord of every intersection row and k_sum_isect_depth sums it exactly as k_sum_isect_rows sums words
// 0..8: same segments, same tree, same chunk-order partials.
__global__ __launch_bounds__(kThreads) void k_sum_isect_depth(
    const float *__restrict__ rows, const uint32_t *__restrict__ num_intersections,
    const uint32_t *__restrict__ cum_tiles_hit, uint32_t cap, float *__restrict__ v_compact, float *__restrict__ partials) {
    const uint32_t I = min(*num_intersections, cap);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t waves = gridDim.x * (kThreads / kWave);
    for (uint32_t k = blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; (uint64_t)k * kWave < I; k += waves) {
        const uint32_t base = k * kWave, u = base + lane;
        const bool valid = u < I;
        float v = 0.0f;
        uint32_t c = 0, first = lane, last = lane;
        bool starts_here = true, ends_here = true;
        if (valid) {
            v = rows[(size_t)u * kCompactStride + kIsectDepthWord];
            c = __float_as_uint(rows[(size_t)u * kCompactStride + kIsectGidWord]);
            // (isect_range, written out: through the helper two of this kernel's instructions change places)
            const uint32_t u0 = c ? min(cum_tiles_hit[c - 1], I) : 0u, u1 = min(cum_tiles_hit[c], I);
            starts_here = u0 >= base;
            ends_here = u1 <= base + kWave;
            first = max(u0, base) - base;
            last = min(u1, base + kWave) - 1u - base;
        }
#pragma unroll
        for (uint32_t dist = 1; dist < kWave; dist <<= 1) {
            const float up = __shfl_up(v, dist, 64);
            if (lane >= first + dist) v += up;
        }
        if (valid && lane == last) {
            float *dst = (starts_here && ends_here) ? v_compact + (size_t)c * kCompactStride
                                                    : partials + ((size_t)k * 2 + (starts_here ? 1 : 0)) * kCompactStride;
            dst[kCompactDepthWord] = v;
        }
    }
}

// v_means[g] += v_z * (d z / d mean) = v_z * viewmat row 2 (p_view = W mean + t, project_forward.wgsl:29-30), one lane
// per visible splat, after the parameter VJP has written v_means.  A zero v_z leaves the row untouched (bitwise).
__global__ __launch_bounds__(kThreads) void k_depth_means_grad(
    const ViewParams vp, const uint32_t *__restrict__ num_visible, uint32_t n,
    const uint32_t *__restrict__ global_from_compact, const float *__restrict__ v_compact, const DetSums det,
    float *__restrict__ v_means) {
    const uint32_t V = min(*num_visible, n);
    for (uint32_t c = blockIdx.x * kThreads + threadIdx.x; c < V; c += gridDim.x * kThreads) {
        const float vz = load_compact_depth(v_compact, det, c);
        if (vz == 0.0f) continue;
        float *m = v_means + (size_t)global_from_compact[c] * 3;
#pragma unroll
        for (int j = 0; j < 3; j++) m[j] += vz * vp.vm[j * 4 + 2];
    }
}

// The dense-gradient rows of visible splat `g`, written by the lane that computed them.
template <int DEG>
__device__ __forceinline__ void store_visible_rows(
    uint32_t g, const float o_mean[3], const float o_scale[3], const float o_quat[4], float o_opac, const float o_xy[2],
    const float vcol[3], const float *Y, float *__restrict__ v_means, float *__restrict__ v_xy,
    float *__restrict__ v_scales, float *__restrict__ v_quats, float *__restrict__ v_sh, float *__restrict__ v_opac) {
    constexpr uint32_t kRow = (DEG + 1) * (DEG + 1) * 3;  // floats per v_sh row
    const size_t gg = g;
    if (v_xy) reinterpret_cast<float2 *>(v_xy)[gg] = make_float2(o_xy[0], o_xy[1]);
    reinterpret_cast<float4 *>(v_quats)[gg] = make_float4(o_quat[0], o_quat[1], o_quat[2], o_quat[3]);
    v_opac[gg] = o_opac;
#pragma unroll
    for (int k = 0; k < 3; k++) v_means[gg * 3 + k] = o_mean[k], v_scales[gg * 3 + k] = o_scale[k];
    float *row = v_sh + gg * kRow;  // v_sh row = Y[k] * v_rgb (gather_grads.wgsl:186-222)
    if constexpr (kRow % 4 == 0) {
#pragma unroll
        for (uint32_t j = 0; j < kRow / 4; j++)
            reinterpret_cast<float4 *>(row)[j] =
                make_float4(Y[(4 * j) / 3] * vcol[(4 * j) % 3], Y[(4 * j + 1) / 3] * vcol[(4 * j + 1) % 3],
                            Y[(4 * j + 2) / 3] * vcol[(4 * j + 2) % 3], Y[(4 * j + 3) / 3] * vcol[(4 * j + 3) % 3]);
    } else {
#pragma unroll
        for (uint32_t e = 0; e < kRow; e++) row[e] = Y[e / 3] * vcol[e % 3];
    }
}

// ADAM: instead of storing the dense parameter gradients, every element goes straight through the optimizer update of
// its parameter (brush_render_backward_adam): the 52+12C bytes per splat of gradients are never written to nor re-read
// from HBM.  v_xy is still stored (refinement statistics).  In this mode `means`/`log_scales`/`raw_opac` alias the
// parameters being updated: each lane reads its own splat before the wave writes the same 64 splats, and no other wave
// touches them.
// (Measured and rejected, round 3: handing the 13 small-array results of a visible splat back through LDS to the lane
// that owns the splat, so that v_means / v_xy / v_scales / v_quats / v_opac leave as whole cache lines, zeros and values
// together: 1.48 vs 1.39 ms at 21 M splats, 52.2 vs 51.7 us at 1 M.  The extra barrier costs more than the partial
// lines.)
// PREZEROED: the compositing backward in front of this launch has already zeroed the dense arrays in passing (ZeroFill,
// internal.hpp): only the visible splats' rows are written here, by the lanes that compute them.  (Still one lane per
// GLOBAL id: a launch over the visible splats in depth order writes the same rows slower at every size measured — 27.5
// vs 25.9 us at 1 M splats, 0.80 vs 0.57 ms at 21 M — because the partial lines of neighbouring splats no longer meet
// in the L2; profiles/r04_zero_fill_in_passing.json.)
// DM = SH degree | kAaMode (internal.hpp): with kAaMode (BRUSH_AUX_ANTIALIASED) the VJP is visible_splat_vjp<DEG, true>.
template <int DM, bool ADAM, bool PREZEROED = false>
__global__ __launch_bounds__(kThreads) void k_project_backward(
    ViewParams vp, const float *means, const float *log_scales, const float *__restrict__ quats, const float *raw_opac,
    const uint32_t *__restrict__ compact_from_global, const float *__restrict__ v_compact, float *__restrict__ v_means,
    float *__restrict__ v_xy, float *__restrict__ v_scales, float *__restrict__ v_quats, float *__restrict__ v_sh,
    float *__restrict__ v_opac, AdamFuse af, DetSums det) {
    constexpr int DEG = DM & kDegMask;
    constexpr bool AA = (DM & kAaMode) != 0;
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    constexpr uint32_t kRow = ncoef * 3;                 // floats per v_sh row
    constexpr uint32_t kRowPad = kRow | 1u;              // odd LDS row stride: conflict-free column access
    constexpr uint32_t kRes = 16 + ncoef;  // per-splat VJP results: mean3 scale3 quat4 opac xy2 vcol3 | Y[ncoef]
    constexpr uint32_t kStageA = (kWave * kRowPad > 512u ? kWave * kRowPad : 512u);
    constexpr uint32_t kStageFloats = kStageA > kWave * kRes ? kStageA : kWave * kRes;
    __shared__ float stage_all[kThreads / kWave][kStageFloats];
    BRUSH_KTRACE(kTrProjectBwd, 0);
    const uint32_t wv = threadIdx.x / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    float *stage = stage_all[wv];
    const uint32_t n = vp.total_splats;
    const uint32_t g0 = blockIdx.x * kThreads + wv * kWave;  // first splat of this wave
    const uint32_t g_own = g0 + lane;
    const bool in_range = g_own < n;
    const uint32_t c_own = in_range ? compact_from_global[g_own] : kInvalid;

    // Only ~10 % of the splats are visible, and the VJP below is ~1500 instructions: the visible splats of the block's
    // 256 are compacted (ballot + LDS) so the arithmetic runs on nearly full waves, and in the Adam form the results
    // travel back to the owning lane through LDS (aliasing the Adam step's staging).  (k_project_backward_lazy compacts
    // the same way, written out there too: through a shared helper the degree-4 Adam kernels come out reordered.)
    __shared__ uint32_t vis_cnt[kThreads / kWave];
    __shared__ uint16_t vis_list[kThreads];
    static_assert(kThreads * kRes <= (kThreads / kWave) * kStageFloats, "result rows must fit the staging buffer");
    float *res = &stage_all[0][0];
    const uint64_t own_vis = __ballot(c_own != kInvalid);
    {
        const uint64_t bal = own_vis;
        if (lane == 0) vis_cnt[wv] = __popcll(bal);
        __syncthreads();
        uint32_t pos = __popcll(bal & lanemask_lt());
        for (uint32_t w2 = 0; w2 < wv; w2++) pos += vis_cnt[w2];
        if (c_own != kInvalid) vis_list[pos] = (uint16_t)threadIdx.x;
        __syncthreads();
    }
    const uint32_t nvis = vis_cnt[0] + vis_cnt[1] + vis_cnt[2] + vis_cnt[3];
    const uint32_t li = threadIdx.x < nvis ? vis_list[threadIdx.x] : 0u;
    const uint32_t g = blockIdx.x * kThreads + li;
    const uint32_t c = threadIdx.x < nvis ? compact_from_global[g] : kInvalid;
    // Dense gradients: the zeros of the invisible splats go out first, so the stores are in flight during the VJP
    if (!ADAM && !PREZEROED && g0 < n) zero_invisible_rows<DEG>(n, g0, lane, own_vis, v_means, v_xy, v_scales, v_quats, v_sh, v_opac);

    float o_mean[3] = {0.f, 0.f, 0.f}, o_scale[3] = {0.f, 0.f, 0.f}, o_quat[4] = {0.f, 0.f, 0.f, 0.f};
    float o_xy[2] = {0.f, 0.f}, o_opac = 0.f;
    float vcol[3] = {0.f, 0.f, 0.f};
    float Y[ncoef];
#pragma unroll
    for (uint32_t k = 0; k < ncoef; k++) Y[k] = 0.f;

    if (c != kInvalid) {
        float4 r0, r1, r2;
        load_compact_sums(v_compact, det, c, r0, r1, r2);
        visible_splat_vjp<DEG, AA>(vp, means, log_scales, quats, raw_opac, g, r0, r1, r2, o_mean, o_scale, o_quat, o_opac,
                                   o_xy, vcol, Y);
        if constexpr (!ADAM) {
            // the computing lane writes the visible splat's rows itself (ordinary stores)
            store_visible_rows<DEG>(g, o_mean, o_scale, o_quat, o_opac, o_xy, vcol, Y, v_means, v_xy, v_scales, v_quats, v_sh,
                                    v_opac);
        } else {
            float *r = res + li * kRes;  // hand the results to the lane that owns splat `li`
            r[0] = o_mean[0], r[1] = o_mean[1], r[2] = o_mean[2];
            r[3] = o_scale[0], r[4] = o_scale[1], r[5] = o_scale[2];
            r[6] = o_quat[0], r[7] = o_quat[1], r[8] = o_quat[2], r[9] = o_quat[3];
            r[10] = o_opac, r[11] = o_xy[0], r[12] = o_xy[1];
            r[13] = vcol[0], r[14] = vcol[1], r[15] = vcol[2];
#pragma unroll
            for (uint32_t k = 0; k < ncoef; k++) r[16 + k] = Y[k];
        }
    }
    if constexpr (!ADAM) return;  // nothing left to exchange: no barrier below is reached by any wave of the block
    __syncthreads();
    {
        const float *r = res + threadIdx.x * kRes;
        const bool vis = c_own != kInvalid;
        o_mean[0] = vis ? r[0] : 0.f, o_mean[1] = vis ? r[1] : 0.f, o_mean[2] = vis ? r[2] : 0.f;
        o_scale[0] = vis ? r[3] : 0.f, o_scale[1] = vis ? r[4] : 0.f, o_scale[2] = vis ? r[5] : 0.f;
        o_quat[0] = vis ? r[6] : 0.f, o_quat[1] = vis ? r[7] : 0.f, o_quat[2] = vis ? r[8] : 0.f, o_quat[3] = vis ? r[9] : 0.f;
        o_opac = vis ? r[10] : 0.f, o_xy[0] = vis ? r[11] : 0.f, o_xy[1] = vis ? r[12] : 0.f;
        vcol[0] = vis ? r[13] : 0.f, vcol[1] = vis ? r[14] : 0.f, vcol[2] = vis ? r[15] : 0.f;
#pragma unroll
        for (uint32_t k = 0; k < ncoef; k++) Y[k] = vis ? r[16 + k] : 0.f;
    }
    __syncthreads();  // `res` aliases the Adam step's staging below
    if (g0 >= n) return;  // wave-uniform; past the last barrier
    float stat_norm = 0.0f;
    if (af.grad_2d_accum) {  // train.rs:300-302
        const float vx = o_xy[0] * af.half_w, vy = o_xy[1] * af.half_h;
        stat_norm = sqrtf(vx * vx + vy * vy);
    }
    adam_step_wave<DEG, false>(af, n, g0, lane, stage, nullptr, o_mean, o_scale, o_quat, o_opac, o_xy, stat_norm,
                               c_own != kInvalid ? 1.0f : 0.0f, Y, vcol, v_xy);
}

// ---- fused backward + Adam with the SH block under deferred Adam (BrushAdamConfig::lazy_sh) ---------------------------
// With the SH block out of the stream the all-in-one kernel above is a chain of small dependent memory phases per wave
// (measured: 155 us at 1 M splats for 0.4 GB).  k_project_backward_lazy is built for what is left: a workgroup owns 256
// CONSECUTIVE global ids (a launch over the visible splats in depth order gathers from nine arrays at random pages per
// lane: no faster) and runs three phases:
//   1. its visible splats, compacted to the first lanes (as in k_project_backward): the projection VJP; the results
//      the other phases need stay in LDS (per visible splat: global id, the time its stored SH block is current for,
//      v_rgb, Y; per owned splat: the 11 small-group gradients and the screen-space statistic);
//   2. the visible splats' SH blocks, kChunks consecutive lanes per row: pending zero-gradient steps replayed, this step
//      applied, sh_time advanced (118 MB of read-modify-write at 1 M splats);
//   3. the workgroup's share of the small-group stream: the 704 16-byte chunks of means / log_scales / rotation /
//      raw_opacity of its 256 splats with their moments (285 MB at 1 M splats), three per lane requested together; the
//      rotation chunks (one splat each) also carry the per-splat duties: chain rule through the normalisation,
//      next_quats_fed, the refinement statistics, v_xy.
// Workgroups in different phases overlap (latency / arithmetic against bandwidth), which two launches — a visible-splat
// kernel (53 us) and a plain small-group stream (60 us at 4.7 TB/s) — could not.  Same expressions as
// adam_step_wave (grad_out.hpp): the same bits as the all-in-one kernel.  Requires n % 4 == 0 and 16-byte aligned
// arrays (AdamFuse::vec_ok).
// DM = SH degree | kAaMode, as k_project_backward.
template <int DM>
__global__ __launch_bounds__(kThreads) void k_project_backward_lazy(
    ViewParams vp, const float *means, const float *log_scales, const float *__restrict__ quats, const float *raw_opac,
    const uint32_t *__restrict__ compact_from_global, const float *__restrict__ v_compact, float *__restrict__ v_xy,
    AdamFuse af, DetSums det) {
    constexpr int DEG = DM & kDegMask;
    constexpr bool AA = (DM & kAaMode) != 0;
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1), kRow = ncoef * 3, kChunks = kRow / 4;
    static_assert(kRow % 4 == 0, "rows of whole 16-byte chunks");
    constexpr uint32_t kFac = (5 + ncoef) | 1u;
    constexpr uint32_t kSmall = 13;  // mean3 scale3 quat4 opac | statistic | visible flag
    __shared__ float fac[kThreads][kFac];
    __shared__ float small_g[kThreads][kSmall];
    __shared__ uint32_t vis_cnt[kThreads / kWave];
    __shared__ uint16_t vis_list[kThreads];
    const uint32_t wv = threadIdx.x / kWave;
    const uint32_t n = vp.total_splats, b0 = blockIdx.x * kThreads;
    const size_t nn = n;
    const uint32_t g_own = b0 + threadIdx.x;
    const uint32_t c_own = g_own < n ? compact_from_global[g_own] : kInvalid;
#pragma unroll
    for (uint32_t k = 0; k < kSmall; k++) small_g[threadIdx.x][k] = 0.0f;  // a splat the view does not see: zero gradient
    {
        const uint64_t bal = __ballot(c_own != kInvalid);
        if (lane_id() == 0) vis_cnt[wv] = __popcll(bal);
        __syncthreads();
        uint32_t pos = __popcll(bal & lanemask_lt());
        for (uint32_t w2 = 0; w2 < wv; w2++) pos += vis_cnt[w2];
        if (c_own != kInvalid) vis_list[pos] = (uint16_t)threadIdx.x;
        __syncthreads();
    }
    const uint32_t nvis = vis_cnt[0] + vis_cnt[1] + vis_cnt[2] + vis_cnt[3];
    // ---- 1. VJP of the visible splats
    uint32_t g = kInvalid;
    if (threadIdx.x < nvis) {
        const uint32_t li = vis_list[threadIdx.x];
        g = b0 + li;
        const uint32_t c = compact_from_global[g];
        float4 r0, r1, r2;
        load_compact_sums(v_compact, det, c, r0, r1, r2);
        float o_mean[3], o_scale[3], o_quat[4], o_xy[2], o_opac, vcol[3], Y[ncoef];
        visible_splat_vjp<DEG, AA>(vp, means, log_scales, quats, raw_opac, g, r0, r1, r2, o_mean, o_scale, o_quat, o_opac,
                                   o_xy, vcol, Y);
        const float vx = o_xy[0] * af.half_w, vy = o_xy[1] * af.half_h;  // train.rs:300-302
        reinterpret_cast<float2 *>(v_xy)[g] = make_float2(o_xy[0], o_xy[1]);
        float *sg = small_g[li];
        sg[0] = o_mean[0], sg[1] = o_mean[1], sg[2] = o_mean[2];
        sg[3] = o_scale[0], sg[4] = o_scale[1], sg[5] = o_scale[2];
        sg[6] = o_quat[0], sg[7] = o_quat[1], sg[8] = o_quat[2], sg[9] = o_quat[3];
        sg[10] = o_opac, sg[11] = sqrtf(vx * vx + vy * vy), sg[12] = 1.0f;
        float *f = fac[threadIdx.x];
        f[0] = __uint_as_float(g), f[1] = __uint_as_float(af.lazy.sh_time[g]);
        f[2] = vcol[0], f[3] = vcol[1], f[4] = vcol[2];
#pragma unroll
        for (uint32_t k = 0; k < ncoef; k++) f[5 + k] = Y[k];
    }
    __syncthreads();
    // ---- 2. the SH blocks: catch up, then this step (gradient row = Y[k] * v_rgb, gather_grads.wgsl:186-222); two
    // chunks per lane are requested together (~25 visible splats x 12 chunks over 256 lanes at 1 M splats)
    const uint32_t total = nvis * kChunks;
    for (uint32_t q0 = threadIdx.x; q0 < total; q0 += 2 * kThreads) {
        float4 x[2], mo[2], vo[2];
        size_t e[2];
        uint32_t r[2], k0[2];
#pragma unroll
        for (uint32_t u = 0; u < 2; u++) {
            const uint32_t q = q0 + u * kThreads;
            if (q < total) {
                r[u] = q / kChunks, k0[u] = (q - r[u] * kChunks) * 4u;
                e[u] = (size_t)__float_as_uint(fac[r[u]][0]) * kRow + k0[u];
                x[u] = *reinterpret_cast<const float4 *>(af.sh + e[u]);
                mo[u] = *reinterpret_cast<const float4 *>(af.m1 + 11 * nn + e[u]);
                vo[u] = *reinterpret_cast<const float4 *>(af.m2 + 11 * nn + e[u]);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 2; u++) {
            if (q0 + u * kThreads >= total) continue;
            const float *f = fac[r[u]];
            lazy_replay4(af.lazy, __float_as_uint(f[1]), k0[u], mo[u], vo[u], x[u]);
            const float4 gr = make_float4(f[5 + (k0[u] + 0) / 3] * f[2 + (k0[u] + 0) % 3], f[5 + (k0[u] + 1) / 3] * f[2 + (k0[u] + 1) % 3],
                                          f[5 + (k0[u] + 2) / 3] * f[2 + (k0[u] + 2) % 3], f[5 + (k0[u] + 3) / 3] * f[2 + (k0[u] + 3) % 3]);
            float4 st = adam_elem4(af, 11 * nn + e[u], gr, x[u], mo[u], vo[u], af.lr[4]);
            sh_rest_lerp(af, k0[u], x[u], st);
            *reinterpret_cast<float4 *>(af.sh + e[u]) = st;
        }
    }
    if (g != kInvalid) af.lazy.sh_time[g] = af.lazy.now + 1u;
    // ---- 3. the small groups of the workgroup's splats, as 16-byte chunks in the order of the moment arrays
    const uint32_t nb = min(kThreads, n - b0);                      // splats owned (a multiple of 4)
    const uint32_t c3 = nb * 3u / 4u, cq = nb, co = nb / 4u;         // chunks of means (= log_scales), rotation, raw_opacity
    const uint32_t chunks = 2u * c3 + cq + co;
    constexpr uint32_t kPer = 3;                                     // 704 chunks over 256 lanes
    float4 x[kPer], mo[kPer], vo[kPer];
    float *p[kPer];
    size_t rel[kPer], e0[kPer];
    uint32_t rowf[kPer], field0[kPer];
    float lr[kPer];
#pragma unroll
    for (uint32_t u = 0; u < kPer; u++) {
        const uint32_t q = threadIdx.x + u * kThreads;
        if (q >= chunks) continue;
        if (q < c3) p[u] = af.means, rel[u] = (size_t)b0 * 3 + q * 4u, e0[u] = rel[u], lr[u] = af.lr[0], rowf[u] = 3, field0[u] = 0;
        else if (q < 2u * c3) p[u] = af.log_scales, rel[u] = (size_t)b0 * 3 + (q - c3) * 4u, e0[u] = 3 * nn + rel[u], lr[u] = af.lr[1], rowf[u] = 3, field0[u] = 3;
        else if (q < 2u * c3 + cq) p[u] = af.rotation, rel[u] = (size_t)b0 * 4 + (q - 2u * c3) * 4u, e0[u] = 6 * nn + rel[u], lr[u] = af.lr[2], rowf[u] = 4, field0[u] = 6;
        else p[u] = af.raw_opac, rel[u] = (size_t)b0 + (q - 2u * c3 - cq) * 4u, e0[u] = 10 * nn + rel[u], lr[u] = af.lr[3], rowf[u] = 1, field0[u] = 10;
        x[u] = nt_load4(p[u] + rel[u]);
        mo[u] = nt_load4(af.m1 + e0[u]);
        vo[u] = nt_load4(af.m2 + e0[u]);
    }
#pragma unroll
    for (uint32_t u = 0; u < kPer; u++) {
        const uint32_t q = threadIdx.x + u * kThreads;
        if (q >= chunks) continue;
        float gr[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t gi = (uint32_t)((rel[u] + i) / rowf[u]);
            gr[i] = small_g[gi - b0][field0[u] + (uint32_t)((rel[u] + i) - (size_t)gi * rowf[u])];
        }
        float4 g4 = make_float4(gr[0], gr[1], gr[2], gr[3]);
        if (rowf[u] == 4) {  // one splat per chunk: the per-splat duties ride here
            const uint32_t gs = (uint32_t)(rel[u] / 4), l = gs - b0;
            const bool vis = small_g[l][12] != 0.0f;
            if (af.quat_vjp) quat_norm_vjp(x[u], g4);
            if (af.grad_2d_accum && vis) {  // train.rs:284-316 (a splat the view does not see adds +0: left alone)
                af.grad_2d_accum[gs] += small_g[l][11] * af.stat_scale;
                af.xy_grad_counts[gs] += 1.0f;
            }
            if (!vis) reinterpret_cast<float2 *>(v_xy)[gs] = make_float2(0.f, 0.f);  // (visible: phase 1)
            const float4 st = adam_elem4(af, e0[u], g4, x[u], mo[u], vo[u], lr[u]);
            nt_store4(p[u] + rel[u], st);
            if (af.norm_rot_out) {  // what the next forward will be fed (gaussian_splats.rs:174-175)
                const float sn = sqrtf(st.x * st.x + st.y * st.y + st.z * st.z + st.w * st.w);
                reinterpret_cast<float4 *>(af.norm_rot_out)[gs] = make_float4(st.x / sn, st.y / sn, st.z / sn, st.w / sn);
            }
        } else {
            nt_store4(p[u] + rel[u], adam_elem4(af, e0[u], g4, x[u], mo[u], vo[u], lr[u]));
        }
    }
}

// brush_lazy_sh_flush: one lane per 16-byte chunk of the SH block; a chunk behind lazy.now replays its pending steps.
// sh_time is only read here (all chunks of a row read the same word); the launcher sets it to `now` afterwards.
__global__ __launch_bounds__(kThreads) void k_lazy_sh_flush(LazySh lazy, float *__restrict__ sh, uint32_t chunks_per_row,
                                                            uint64_t total_chunks) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total_chunks) return;
    const uint32_t g = (uint32_t)(i / chunks_per_row), k0 = (uint32_t)(i - (uint64_t)g * chunks_per_row) * 4u;
    const uint32_t t0 = lazy.sh_time[g];
    if (t0 >= lazy.now) return;
    float4 x = nt_load4(sh + i * 4), m = nt_load4(lazy.m1 + i * 4), v = nt_load4(lazy.m2 + i * 4);
    lazy_replay4(lazy, t0, k0, m, v, x);
    nt_store4(sh + i * 4, x);
    nt_store4(lazy.m1 + i * 4, m);
    nt_store4(lazy.m2 + i * 4, v);
}
__global__ __launch_bounds__(kThreads) void k_fill_u32(uint32_t *__restrict__ dst, uint32_t value, uint32_t n) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dst[i] = value;
}

}  // namespace

hipError_t launch_lazy_sh_flush(const LazySh &lazy, float *sh, uint32_t n, uint32_t row_floats, hipStream_t s) {
    const uint64_t chunks = (uint64_t)n * (row_floats / 4u);
    if (chunks == 0) return hipSuccess;
    if (chunks / kThreads >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lazy_sh_flush, dim3((uint32_t)((chunks + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, lazy, sh,
                       row_floats / 4u, chunks);
    hipLaunchKernelGGL(k_fill_u32, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, lazy.sh_time, lazy.now, n);
    return hipGetLastError();
}

hipError_t launch_zero_compact_grads(const uint32_t *num_visible, uint32_t n, float *v_compact, hipStream_t s) {
    const uint32_t grid = max(1u, min(ceil_div(n * 3u, kThreads), 1024u));
    hipLaunchKernelGGL(k_zero_compact_grads, dim3(grid), dim3(kThreads), 0, s, num_visible, n,
                       reinterpret_cast<float4 *>(v_compact));
    return hipGetLastError();
}

hipError_t launch_project_backward(const ViewParams &vp, const float *means, const float *log_scales,
                                   const float *quats, const float *raw_opac,
                                   const uint32_t *compact_from_global, const float *v_compact, float *v_means,
                                   float *v_xy, float *v_scales, float *v_quats, float *v_sh, float *v_opac,
                                   const AdamFuse *adam, const DetSumsArgs &dargs, bool prezeroed, hipStream_t s,
                                   bool antialiased) {
    const uint32_t n = vp.total_splats;
    if (n == 0) return hipSuccess;
    const dim3 grid(ceil_div(n, kThreads)), block(kThreads);
    const AdamFuse af = adam ? *adam : AdamFuse{};
    const DetSums det = make_det_sums(dargs);
    if (adam && af.lazy.on()) {  // SH block under deferred Adam
        dispatch_dm_lazy(vp.sh_degree, antialiased, [&](auto dm) {
            hipLaunchKernelGGL(k_project_backward_lazy<dm()>, grid, block, 0, s, vp, means, log_scales, quats, raw_opac,
                               compact_from_global, v_compact, v_xy, af, det);
        });
        return hipGetLastError();
    }
    dispatch_dm(vp.sh_degree, antialiased, [&](auto dm) {
        auto k = adam ? k_project_backward<dm(), true> : prezeroed ? k_project_backward<dm(), false, true>
                                                                    : k_project_backward<dm(), false>;
        hipLaunchKernelGGL(k, grid, block, 0, s, vp, means, log_scales, quats, raw_opac, compact_from_global, v_compact,
                           v_means, v_xy, v_scales, v_quats, v_sh, v_opac, af, det);
    });
    return hipGetLastError();
}

hipError_t launch_sum_isect_rows(const float *rows, const uint32_t *num_intersections, const uint32_t *cum_tiles_hit,
                                 uint32_t cap, float *v_compact, float *partials, hipStream_t s) {
    if (cap == 0) return hipSuccess;
    const uint32_t chunks = ceil_div(cap, kWave);
    hipLaunchKernelGGL(k_sum_isect_rows, dim3(min(ceil_div(chunks, kThreads / kWave), 4096u)), dim3(kThreads), 0, s,
                       reinterpret_cast<const float4 *>(rows), num_intersections, cum_tiles_hit, cap,
                       reinterpret_cast<float4 *>(v_compact), reinterpret_cast<float4 *>(partials));
    return hipGetLastError();
}

hipError_t launch_sum_isect_depth(const float *rows, const uint32_t *num_intersections, const uint32_t *cum_tiles_hit,
                                  uint32_t cap, float *v_compact, float *partials, hipStream_t s) {
    if (cap == 0) return hipSuccess;
    const uint32_t chunks = ceil_div(cap, kWave);
    hipLaunchKernelGGL(k_sum_isect_depth, dim3(min(ceil_div(chunks, kThreads / kWave), 4096u)), dim3(kThreads), 0, s,
                       rows, num_intersections, cum_tiles_hit, cap, v_compact, partials);
    return hipGetLastError();
}

hipError_t launch_depth_means_grad(const ViewParams &vp, const uint32_t *num_visible, uint32_t n,
                                   const uint32_t *global_from_compact, const float *v_compact,
                                   const DetSumsArgs &dargs, float *v_means, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const DetSums det = make_det_sums(dargs);
    hipLaunchKernelGGL(k_depth_means_grad, dim3(min(ceil_div(n, kThreads), 2048u)), dim3(kThreads), 0, s, vp,
                       num_visible, n, global_from_compact, v_compact, det, v_means);
    return hipGetLastError();
}

}  // namespace brush

using namespace brush;

// ---- the two entries of the deferred SH Adam (lazy_sh.hpp) that are no render call: the table of its steps' constants
// (host only) and the flush that catches every row up ----------------------------------------------------------------

extern "C" int brush_lazy_sh_fill_table(float beta1, float beta2, float lr_coeffs_dc, float sh_rest_lerp, uint32_t base,
                                        uint32_t capacity, float *host_rows) {
    if (!host_rows || base > 0xFFFFFFFFu - capacity) return BRUSH_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < capacity; i++) {
        adam_bias_corrections(beta1, beta2, base + 1u + i, &host_rows[4 * i], &host_rows[4 * i + 1]);
        host_rows[4 * i + 2] = lr_coeffs_dc;
        host_rows[4 * i + 3] = sh_rest_lerp;
    }
    return BRUSH_OK;
}

extern "C" int brush_lazy_sh_flush(const BrushLazySh *h_lazy, float *sh, uint32_t n, uint32_t sh_degree,
                                   brush_stream_t stream) {
    LazySh lazy;
    if (!h_lazy || sh_degree > 4 || !make_lazy_sh(h_lazy, sh_degree, &lazy)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;
    if (!sh || misaligned(sh, 16)) return BRUSH_ERR_INVALID_ARG;
    BRUSH_HIP_CHECK(launch_lazy_sh_flush(lazy, sh, n, 3u * (sh_degree + 1u) * (sh_degree + 1u),
                                         static_cast<hipStream_t>(stream)));
    return BRUSH_OK;
}
