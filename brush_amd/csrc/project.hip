// project.hip — the first per-splat forward stage: cull + depth key, the survivors' ProjectedSplat record (conic / xy /
// SH colour / opacity) and the order-preserving compaction.  The tile passes that follow it are tile_count.hip and
// tile_emit.hip.
//
// Replaces (paths relative to the reference checkout):
//   ProjectSplats            crates/brush-render/src/shaders/project_forward.wgsl:15-68
//   ProjectVisible           .../project_visible.wgsl:163-258, the record half: computed here in global-id order (see
//                            k_project_cull); tile_count.hip gathers it into compact order and counts the tiles
//
// This translation unit, like the two tile units, is compiled with -ffp-contract=off: every integer decision (cull,
// tile counts, tile lists) is a function of correctly rounded f32 operations in a fixed order, so the visible set,
// depth order and per-tile lists are reproducible bit-for-bit.
//
// Differences from the reference by design:
//   * compaction is order-preserving (ascending global id) instead of an atomicAdd slot
//     (project_forward.wgsl:65), which makes equal-depth order deterministic;
//   * a compact_from_global map is produced so the backward can write dense gradients once,
//     coalesced, instead of zero-filling and scattering.
// All kernels are HBM-streaming (roofline: HBM).
#include "internal.hpp"
#include "lazy_sh.hpp"
#include "splat_math.hpp"
#include "trace.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kCullPerThread = 4;                     // splats per lane in the cull / compact kernels
constexpr uint32_t kCullBlock = kThreads * kCullPerThread;  // splats per cull workgroup
constexpr uint32_t kSelfScanBlocks = 2048;  // up to this many cull workgroups k_compact scans their counts itself

// ---- ProjectSplats: cull + depth key (+ the survivors' ProjectedSplat record) -------------------
// project_forward.wgsl:15-68 and project_visible.wgsl:163-258.  Being the first launch of the forward
// pass it also publishes the uniforms buffer and clears the counters and tile_bins
// (render.rs:102-116,241-244) so that no separate init launch is needed.

// SH -> colour with the WGSL expression tree (project_visible.wgsl:51-147,232-241).
template <int DEG>
__device__ __forceinline__ void sh_colour(const ViewParams &vp, const float mean[3], const float *__restrict__ sh,
                                          float rgb[3]) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);  // compile-time: all SH loads issue together
    float dir[3];
    view_dir(vp, mean, dir);
    float Y[ncoef];
    sh_basis<ncoef>(DEG, dir, Y);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float col = Y[0] * sh[ch];
        if (DEG >= 1) {
            const float inner = ((-dir[1]) * sh[1 * 3 + ch] + dir[2] * sh[2 * 3 + ch]) - dir[0] * sh[3 * 3 + ch];
            col = col + 0.48860251190292f * inner;
        }
        if (DEG >= 2) {
            float acc = Y[4] * sh[4 * 3 + ch];
#pragma unroll
            for (int k = 5; k < 9; k++) acc = acc + Y[k] * sh[k * 3 + ch];
            col = col + acc;
        }
        if (DEG >= 3) {
            float acc = Y[9] * sh[9 * 3 + ch];
#pragma unroll
            for (int k = 10; k < 16; k++) acc = acc + Y[k] * sh[k * 3 + ch];
            col = col + acc;
        }
        if (DEG >= 4) {
            float acc = Y[16] * sh[16 * 3 + ch];
#pragma unroll
            for (int k = 17; k < 25; k++) acc = acc + Y[k] * sh[k * 3 + ch];
            col = col + acc;
        }
        rgb[ch] = col + 0.5f;
    }
}

// The splat's ProjectedSplat record (project_visible.wgsl:163-258) is produced HERE, for every splat
// that passes the cull, while its parameters stream through in global-id order: the reference (and
// an earlier version of this file) recomputes it after the depth sort from seven gathers by global id,
// which on MI355X is bound by address-translation misses (one page per lane per array), not by
// bandwidth or arithmetic.  The record goes to a global-id-indexed staging row of 48 bytes;
// k_project_visible then needs ONE gather per splat.
// LAZY (BrushAux::lazy_sh): the SH block is under deferred Adam (lazy_sh.hpp): a visible splat's colour is evaluated
// from its stored coefficients with the pending zero-gradient steps replayed in registers; nothing is written back.
// (four waves per SIMD: the launch is 4 waves per SIMD at 1 M splats, one round; the LAZY degree-3 form would otherwise
// take 130 registers and a second round; under the cap the two LAZY degree-3 forms, with and without kAaMode, spill
// 6 VGPRs into 28 bytes of scratch, the only spills of this file and the two tile units; what they cost is unmeasured)
// Word 8 of the record: sigmoid(raw), times cov_compensation in the antialiased mode.
template <bool AA>
__device__ __forceinline__ float record_opacity(float raw_opac, const float raw[3], const float cov2d[3]) {
    if constexpr (AA) return det_sigmoid(raw_opac) * cov_compensation(raw, cov2d);
    return det_sigmoid(raw_opac);
}

// DM = SH degree | kAaMode (internal.hpp): with kAaMode (BRUSH_AUX_ANTIALIASED) the record's opacity is
// sigmoid(raw) * cov_compensation (splat_math.hpp), everything else is as without it.  The mode rides in the degree
// argument so that the instantiations without it keep their names and their code.
template <int DM, bool LAZY = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_project_cull(ViewParams vp, BrushUniforms u,
                                                           const float *__restrict__ means,
                                                           const float *__restrict__ log_scales,
                                                           const float *__restrict__ quats,
                                                           const float *__restrict__ sh_coeffs,
                                                           const float *__restrict__ raw_opac,
                                                           float4 *__restrict__ proj_global,
                                                           uint32_t *__restrict__ key_all,
                                                           uint32_t *__restrict__ compact_from_global,
                                                           uint32_t *__restrict__ block_counts,
                                                           uint32_t *__restrict__ uniforms_buffer,
                                                           uint32_t *__restrict__ num_intersections,
                                                           uint32_t *__restrict__ overflow,
                                                           uint32_t *__restrict__ tile_bins, uint32_t num_bin_words,
                                                           uint32_t *__restrict__ bin_edges,
                                                           uint32_t *__restrict__ walk_counter, LazySh lazy) {
    constexpr int DEG = DM & kDegMask;
    constexpr bool AA = (DM & kAaMode) != 0;
    __shared__ uint32_t wave_cnt[kThreads / kWave];
    __shared__ uint32_t vis_list[kThreads / kWave][kCullPerThread * kWave];  // per wave: global ids that passed
    BRUSH_KTRACE(kTrCull, 0);
    // (Measured and rejected, round 3: streaming the raw opacities with Phase A's coalesced loads instead of gathering
    // them in Phase B, where every candidate's 4 bytes cost a 128-byte request: +1.5 us at 1 M splats, no gain at 21 M.)
    const uint32_t gt = blockIdx.x * kThreads + threadIdx.x;
    if (gt < kUniformWords) uniforms_buffer[gt] = reinterpret_cast<const uint32_t *>(&u)[gt];
    if (gt == 0) {
        *num_intersections = 0;
        *overflow = 0;
        *walk_counter = 0;
    }
    for (uint32_t i = gt; i < num_bin_words; i += gridDim.x * kThreads) {
        tile_bins[i] = 0;  // render.rs:241-244
        bin_edges[i] = 0;  // accumulators of the tile sort's last pass (sort_launch: edges)
    }

    // Phase A — every splat of the wave's 4 x 64 (round r covers 256 consecutive splats): the two cheap
    // rejections (behind the camera :32, and a conservative screen-bounds test that never changes a
    // decision).  Only ~1 splat in 8 survives them, so the survivors' ids are queued per wave and the
    // expensive exact projection (Phase B) runs on full waves instead of once per round at 12 % lane
    // occupancy.  The loads of all four rounds are issued up front (one memory phase per wave).
    float mean_r[kCullPerThread][3], smax_r[kCullPerThread];
    const uint32_t last = vp.total_splats ? vp.total_splats - 1 : 0;
#pragma unroll
    for (uint32_t r = 0; r < kCullPerThread; r++) {
        const size_t g = min(blockIdx.x * kCullBlock + r * kThreads + threadIdx.x, last);
        if (vp.total_splats) {  // uniform: an empty cloud has no row 0 to clamp to
#pragma unroll
            for (int k = 0; k < 3; k++) mean_r[r][k] = means[g * 3 + k];
            smax_r[r] = fmaxf(log_scales[g * 3], fmaxf(log_scales[g * 3 + 1], log_scales[g * 3 + 2]));
        } else {
            mean_r[r][0] = mean_r[r][1] = mean_r[r][2] = 0.0f;
            smax_r[r] = 0.0f;
        }
    }
    BRUSH_KTRACE_MARK(1, mean_r[0][0]);
    BRUSH_KTRACE_MARK(2, smax_r[kCullPerThread - 1]);
    uint32_t n_cand = 0;
    uint32_t *list = vis_list[threadIdx.x / kWave];
#pragma unroll
    for (uint32_t r = 0; r < kCullPerThread; r++) {
        const uint32_t g = blockIdx.x * kCullBlock + r * kThreads + threadIdx.x;
        bool maybe = false;
        if (g < vp.total_splats) {
            const float mean[3] = {mean_r[r][0], mean_r[r][1], mean_r[r][2]};
            float p_view[3];
            to_view(vp, mean, p_view);
            maybe = p_view[2] > 0.01f;  // :32
            if (maybe) {
                // radius <= 3*sqrt(lambda_max + quirk slack) + 1 with lambda_max(cov2d) <= trace <=
                // s_max^2 * cull_k / z^2 + 0.6; if even that radius leaves the tile bbox empty, the exact
                // test (:54-62) would reject as well.
                // CONTRACT: the bound takes |V|_2 = s_max^2, i.e. a UNIT quaternion (no load of it here: Phase A is
                // an HBM stream).  quat_to_rotmat does not normalise: for |q| = s it yields
                // R(q) = (1 - s^2) I + s^2 R(q/s), of norm |2 s^2 - 1|, so |V|_2 <= (2 s^2 - 1)^2 s_max^2.  cull_k
                // carries |W|_F^2 = 3 where an orthonormal view rotation needs |W|_2^2 = 1, and 1 % on top: the
                // bound stays safe while (2 s^2 - 1)^2 <= 3.03, s <= 1.17, and for every s <= 1.  Callers are told
                // |q| <= 1.1 (brush_hip.h, render_splats); beyond that a splat whose centre is off-frame may be
                // culled here where the reference keeps it (tests/test_cull_cpu.py asserts that |q| = 2 does it).
                const float smax = det_expf(smax_r[r]) * 1.001f;
                const float rz = 1.0f / p_view[2];
                const float lam = smax * smax * vp.cull_k * rz * rz + 1.0f;
                const float rb = 3.0f * sqrtf(lam) + 2.0f;
                const float cxp = p_view[0] * rz * vp.focal[0] + vp.pixel_center[0];
                const float cyp = p_view[1] * rz * vp.focal[1] + vp.pixel_center[1];
                const float wpx = (float)(vp.tile_bounds[0] * kTileWidth), hpx = (float)(vp.tile_bounds[1] * kTileWidth);
                if (cxp + rb < -1.0f || cxp - rb > wpx + 1.0f || cyp + rb < -1.0f || cyp - rb > hpx + 1.0f) maybe = false;
            }
            if (!maybe) key_all[g] = kInvalid;
            compact_from_global[g] = kInvalid;
        }
        const uint64_t bal = __ballot(maybe);
        if (maybe) list[n_cand + __popcll(bal & lanemask_lt())] = g;
        n_cand += __popcll(bal);
    }
    __builtin_amdgcn_wave_barrier();

    // Phase B — exact cull (project_forward.wgsl:36-66) and, for the splats that pass, the whole
    // ProjectedSplat record (project_visible.wgsl:163-258).
    BRUSH_KTRACE_MARK(3, n_cand);
    uint32_t block_visible = 0;
    for (uint32_t base = 0; base < n_cand; base += kWave) {  // wave-uniform
        const uint32_t i = base + lane_id();
        bool visible = false;
        if (i < n_cand) {
            const uint32_t g = list[i];
            const float mean[3] = {means[(size_t)g * 3], means[(size_t)g * 3 + 1], means[(size_t)g * 3 + 2]};
            const float scale[3] = {det_expf(log_scales[(size_t)g * 3]), det_expf(log_scales[(size_t)g * 3 + 1]),
                                    det_expf(log_scales[(size_t)g * 3 + 2])};
            const float4 q4 = reinterpret_cast<const float4 *>(quats)[g];
            const float quat[4] = {q4.x, q4.y, q4.z, q4.w};
            const float ro = raw_opac[g];
            const float *sh = sh_coeffs + (size_t)g * ((DEG + 1) * (DEG + 1)) * 3;
            float p_view[3], cov2d[3], raw[3];
            to_view(vp, mean, p_view);
            calc_cov2d(vp, p_view, scale, quat, cov2d, AA ? raw : nullptr);
            const float det = cov2d[0] * cov2d[2] - cov2d[1] * cov2d[1];
            if (!(det == 0.0f)) {  // :43
                float conic[3], xy[2];
                cov_to_conic(cov2d, conic);
                project_pix(vp, p_view, xy);
                const uint32_t radius = radius_from_conic(conic);
                uint32_t bb[4];
                get_tile_bbox(xy, radius, vp.tile_bounds, bb);
                if ((bb[2] - bb[0]) != 0u && (bb[3] - bb[1]) != 0u) {  // :60
                    visible = true;
                    // the antialiased opacity before the colour: the covariance terms die here instead of living
                    // through the SH evaluation (the LAZY degree-3 form is at the register cap)
                    float opac_aa = 0.0f;
                    if constexpr (AA) opac_aa = record_opacity<true>(ro, raw, cov2d);
                    float rgb[3];
                    if constexpr (LAZY) {
                        constexpr uint32_t kRow = (DEG + 1) * (DEG + 1) * 3;
                        float cur[kRow];
                        lazy_current_row<kRow>(lazy, sh_coeffs, g, cur);
                        sh_colour<DEG>(vp, mean, cur, rgb);
                    } else {
                        sh_colour<DEG>(vp, mean, sh, rgb);
                    }
                    float4 *row = proj_global + (size_t)g * 3;
                    row[0] = make_float4(xy[0], xy[1], conic[0], conic[1]);
                    row[1] = make_float4(conic[2], AA ? opac_aa : record_opacity<false>(ro, raw, cov2d), 0.0f, 0.0f);
                    row[2] = make_float4(rgb[0], rgb[1], rgb[2], 0.0f);
                }
            }
            key_all[g] = visible ? __float_as_uint(p_view[2]) : kInvalid;
        }
        block_visible += __popcll(__ballot(visible));
    }
    BRUSH_KTRACE_MARK(4, block_visible);
    if (lane_id() == 0) wave_cnt[threadIdx.x / kWave] = block_visible;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// Exclusive scan of block_counts in place; total -> num_visible and uniforms_buffer[25].
__global__ __launch_bounds__(1024) void k_cull_scan(uint32_t *__restrict__ block_counts, uint32_t num_blocks,
                                                    uint32_t *__restrict__ num_visible,
                                                    uint32_t *__restrict__ uniforms_buffer) {
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < num_blocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < num_blocks ? block_counts[i] : 0u;
        const uint32_t incl = wave_inclusive_scan(v);
        if (lane_id() == 63) wave_tot[threadIdx.x / kWave] = incl;
        __syncthreads();
        uint32_t off = carry_s;
        for (uint32_t w = 0; w < threadIdx.x / kWave; w++) off += wave_tot[w];
        if (i < num_blocks) block_counts[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *num_visible = carry_s;
        uniforms_buffer[kNumVisibleWord] = carry_s;
    }
}

// Order-preserving compaction of (depth key, global id); same 1024-splat partition as the cull.
// SELF_SCAN: block_offsets holds the raw per-block counts and every block sums the counts of the
// blocks before it (<= kSelfScanBlocks of them), the last block publishing the total; this saves the
// k_cull_scan launch for clouds up to 2M splats.
template <bool SELF_SCAN>
__global__ __launch_bounds__(kThreads) void k_compact(uint32_t n, const uint32_t *__restrict__ key_all,
                                                      const uint32_t *__restrict__ block_offsets,
                                                      uint32_t *__restrict__ keys, uint32_t *__restrict__ gids,
                                                      uint32_t *__restrict__ num_visible,
                                                      uint32_t *__restrict__ uniforms_buffer) {
    __shared__ uint32_t wave_cnt[kCullPerThread][kThreads / kWave];
    __shared__ uint32_t pre_s[kThreads / kWave];
    const uint32_t wid = threadIdx.x / kWave;
    BRUSH_KTRACE(kTrCompact, 0);
    // the keys do not depend on the block offsets: requested first, so both loads are in flight together
    uint32_t key[kCullPerThread];
#pragma unroll
    for (uint32_t r = 0; r < kCullPerThread; r++) {
        const uint32_t g = blockIdx.x * kCullBlock + r * kThreads + threadIdx.x;
        key[r] = g < n ? key_all[g] : kInvalid;
    }
    uint32_t before = 0;
    if (SELF_SCAN) {
        for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kThreads) before += block_offsets[i];
        BRUSH_KTRACE_MARK(1, before);
        before = wave_sum(before);
        if (lane_id() == 0) pre_s[wid] = before;
    }
    uint64_t bal[kCullPerThread];
#pragma unroll
    for (uint32_t r = 0; r < kCullPerThread; r++) {
        bal[r] = __ballot(key[r] != kInvalid);
        if (lane_id() == 0) wave_cnt[r][wid] = __popcll(bal[r]);
    }
    BRUSH_KTRACE_MARK(2, key[kCullPerThread - 1]);
    __syncthreads();
    uint32_t off;
    if (SELF_SCAN) {
        off = pre_s[0] + pre_s[1] + pre_s[2] + pre_s[3];
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
            const uint32_t total = off + block_offsets[blockIdx.x];
            *num_visible = total;
            uniforms_buffer[kNumVisibleWord] = total;
        }
    } else {
        off = block_offsets[blockIdx.x];
    }
#pragma unroll
    for (uint32_t r = 0; r < kCullPerThread; r++) {
        uint32_t mine = off + __popcll(bal[r] & lanemask_lt());
        for (uint32_t w = 0; w < kThreads / kWave; w++) {
            const uint32_t c = wave_cnt[r][w];
            if (w < wid) mine += c;
            off += c;
        }
        if (key[r] != kInvalid) {
            keys[mine] = key[r];
            gids[mine] = blockIdx.x * kCullBlock + r * kThreads + threadIdx.x;
        }
    }
}

}  // namespace


size_t cull_block_count(uint32_t n) { return ceil_div(n ? n : 1, kCullBlock); }

hipError_t launch_project_cull(const ViewParams &vp, const BrushUniforms &u, const BrushAux &aux,
                               uint32_t num_tiles, const float *means, const float *log_scales,
                               const float *quats, const float *sh, const float *raw_opac, float *proj_global,
                               uint32_t *key_all, uint32_t *block_counts, uint32_t *keys,
                               uint32_t *gids, uint32_t *bin_edges, const WalkWs &walk, const LazySh &lazy,
                               hipStream_t s) {
    const uint32_t n = vp.total_splats;
    const uint32_t blocks = (uint32_t)cull_block_count(n);
    uint32_t *compact_from_global = aux.compact_from_global_gid;
    uint32_t *num_visible = aux.num_visible;
    uint32_t *uniforms_buffer = aux.uniforms_buffer;
    const bool aa = (aux.flags & BRUSH_AUX_ANTIALIASED) != 0;
    auto launch = [&](auto dm, auto deferred) {
        hipLaunchKernelGGL((k_project_cull<dm(), deferred()>), dim3(blocks), dim3(kThreads), 0, s, vp, u, means, log_scales,
                           quats, sh, raw_opac, reinterpret_cast<float4 *>(proj_global), key_all, compact_from_global,
                           block_counts, uniforms_buffer, aux.num_intersections, aux.overflow, aux.tile_bins,
                           num_tiles * 2, bin_edges, walk.counter, lazy);
    };
    if (lazy.on()) dispatch_dm_lazy(vp.sh_degree, aa, [&](auto dm) { launch(dm, std::true_type{}); });
    else dispatch_dm(vp.sh_degree, aa, [&](auto dm) { launch(dm, std::false_type{}); });
    if (blocks <= kSelfScanBlocks) {
        hipLaunchKernelGGL(k_compact<true>, dim3(blocks), dim3(kThreads), 0, s, n, key_all, block_counts, keys, gids,
                           num_visible, uniforms_buffer);
    } else {
        hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(1024), 0, s, block_counts, blocks, num_visible,
                           uniforms_buffer);
        hipLaunchKernelGGL(k_compact<false>, dim3(blocks), dim3(kThreads), 0, s, n, key_all, block_counts, keys, gids,
                           num_visible, uniforms_buffer);
    }
    return hipGetLastError();
}

}  // namespace brush
