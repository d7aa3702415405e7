// grad_out.hpp — how the parameter gradients of a backward leave it, shared by the single-view kernels (project_bwd.hip)
// and the view-sum kernels (view_records.hip):
//   dense  every element of the dense gradient arrays is written exactly once: the zeros of the splats no view sees
//          straight from registers by the lanes that own the addresses (zero_invisible_rows; or, PREZEROED, in passing
//          by the compositing kernel in front), a seen splat's rows by the lane that computed them;
//   Adam   the gradients are never stored: each wave parks the rows of its 64 splats in LDS staging rows and sends every
//          element straight through the optimizer update of its parameter (adam_step_wave).
// Replaces the nine zero-fills of crates/brush-render/src/render.rs:505-507,539-547,573-575.  Built without FMA
// contraction (pragma below and -ffp-contract=off): the fused and the separate optimizer paths give the same bits.
#pragma once
#include "internal.hpp"
#include "splat_math.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
// Streaming 16-byte accesses: data that is touched once per step and is far larger than the caches.
__device__ __forceinline__ float4 nt_load4(const float *p) {
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float *p, float4 v) {
    const v4f nv = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(nv, reinterpret_cast<v4f *>(p));
}

// ---- dense ---------------------------------------------------------------------------------------------------------
// ~90 % of the splats are not visible from the view, so most of the 52 + 12C bytes per splat the backward writes are
// zeros.  The lanes that own the addresses store them straight from registers: consecutive lanes, consecutive 16-byte
// words of the wave's contiguous regions, the rows of visible splats skipped by their bit in the wave's visibility mask
// `vis`; the visible splats' rows are written by the lanes that computed them.  No LDS staging, no transposes (the
// staged form spent 56 % of its LDS cycles in bank conflicts): 65 -> 49 us at 1 M splats.
// The v_sh rows are whole cache lines (192 B at degree 3), so their zeros are streaming stores; the small arrays share
// lines between neighbouring splats, visible or not, and use ordinary stores, which the L2 merges into full lines (a
// streaming store of part of a line costs a whole line at the memory: 92 us).  For the same reason the visible rows are
// written by the workgroup that owns their neighbours: a variant with separate workgroups walking the visible splats in
// depth order wrote the same bytes 35 % slower at 21 M splats (1.73 vs 1.28 ms), the partial lines no longer meeting
// in the L2.
template <int DEG>
__device__ __forceinline__ void zero_invisible_rows(
    uint32_t n, uint32_t g0, uint32_t lane, uint64_t vis, float *__restrict__ v_means, float *__restrict__ v_xy,
    float *__restrict__ v_scales, float *__restrict__ v_quats, float *__restrict__ v_sh, float *__restrict__ v_opac) {
    constexpr uint32_t kRow = (DEG + 1) * (DEG + 1) * 3;  // floats per v_sh row
    const uint32_t rows = min(kWave, n - g0);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float *sh = v_sh + (size_t)g0 * kRow;
    if constexpr (kRow % 16 == 0) {  // rows of whole 64-byte lines
        constexpr uint32_t kPerRow = kRow / 4;
        const uint32_t total = rows * kPerRow;
#pragma unroll
        for (uint32_t it = 0; it < kPerRow; it++) {
            const uint32_t q = it * kWave + lane;
            if (q < total && !((vis >> (q / kPerRow)) & 1ull)) nt_store4(sh + (size_t)q * 4, z4);
        }
    } else {
        const uint32_t total = rows * kRow;
#pragma unroll
        for (uint32_t it = 0; it < kRow; it++) {
            const uint32_t f = it * kWave + lane;
            if (f < total && !((vis >> (f / kRow)) & 1ull)) sh[f] = 0.0f;
        }
    }
    if (lane < rows && !((vis >> lane) & 1ull)) {
        const size_t g = (size_t)g0 + lane;
        if (v_xy) reinterpret_cast<float2 *>(v_xy)[g] = make_float2(0.f, 0.f);
        reinterpret_cast<float4 *>(v_quats)[g] = z4;
        v_opac[g] = 0.0f;
    }
    // v_means / v_scales: 3 floats per splat; 16-byte word `lane` of the wave's region covers floats 4 lane .. 4 lane + 3,
    // i.e. rows (4 lane) / 3 and (4 lane + 3) / 3
    if (lane < 48u) {
        const uint32_t f0 = lane * 4u, ra = f0 / 3u, rb = (f0 + 3u) / 3u;
        const bool a_vis = (vis >> ra) & 1ull, b_vis = (vis >> rb) & 1ull;
        float *m = v_means + (size_t)g0 * 3 + f0, *sc = v_scales + (size_t)g0 * 3 + f0;
        if (rb < rows && !a_vis && !b_vis) {
            *reinterpret_cast<float4 *>(m) = z4;
            *reinterpret_cast<float4 *>(sc) = z4;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t r = (f0 + i) / 3u;
                if (r < rows && !((vis >> r) & 1ull)) m[i] = 0.0f, sc[i] = 0.0f;
            }
        }
    }
}

// ---- Adam ----------------------------------------------------------------------------------------------------------
// One Adam update of burn 0.16 `Adam::step` (see train_step.hip:k_adam) on element `e` of the moment
// arrays; returns the stepped parameter value.
__device__ __forceinline__ float adam_elem(const AdamFuse &a, size_t e, float g, float x, float lr) {
    const float m = a.m1[e] * a.beta1 + g * (1.0f - a.beta1);
    const float v = a.m2[e] * a.beta2 + (g * g) * (1.0f - a.beta2);
    a.m1[e] = m, a.m2[e] = v;
    return adam_stepped(m, v, x, a.rbc1, a.rbc2, a.eps, lr);
}
__device__ __forceinline__ float4 adam_elem4(const AdamFuse &a, size_t e, float4 g, float4 x, float4 mo, float4 vo,
                                             float lr) {
    float4 m, v, r;
#define BRUSH_ADAM_C(c)                                                        \
    m.c = mo.c * a.beta1 + g.c * (1.0f - a.beta1);                             \
    v.c = vo.c * a.beta2 + (g.c * g.c) * (1.0f - a.beta2);                     \
    r.c = adam_stepped(m.c, v.c, x.c, a.rbc1, a.rbc2, a.eps, lr);
    BRUSH_ADAM_C(x) BRUSH_ADAM_C(y) BRUSH_ADAM_C(z) BRUSH_ADAM_C(w)
#undef BRUSH_ADAM_C
    nt_store4(a.m1 + e, m);
    nt_store4(a.m2 + e, v);
    return r;
}
__device__ __forceinline__ float4 adam_elem4(const AdamFuse &a, size_t e, float4 g, float4 x, float lr) {
    return adam_elem4(a, e, g, x, nt_load4(a.m1 + e), nt_load4(a.m2 + e), lr);
}

// (The two pieces below take their float4 by reference: by value the compiler spends register moves on them.)
// SH coefficients >= 1 move only sh_lerp of the way (train.rs:336-351): `st` is the stepped 16-byte chunk at position
// k0 of an SH row (positions 0..2 = the dc coefficient), `x` its value before the step.
__device__ __forceinline__ void sh_rest_lerp(const AdamFuse &af, uint32_t k0, const float4 &x, float4 &st) {
    st.x = k0 + 0 >= 3 ? x.x * (1.0f - af.sh_lerp) + st.x * af.sh_lerp : st.x;
    st.y = k0 + 1 >= 3 ? x.y * (1.0f - af.sh_lerp) + st.y * af.sh_lerp : st.y;
    st.z = k0 + 2 >= 3 ? x.z * (1.0f - af.sh_lerp) + st.z * af.sh_lerp : st.z;
    st.w = k0 + 3 >= 3 ? x.w * (1.0f - af.sh_lerp) + st.w * af.sh_lerp : st.w;
}
// The op was fed r/|r| (gaussian_splats.rs:174-175): chains its gradient `gq` to the raw rotation parameter r.
__device__ __forceinline__ void quat_norm_vjp(const float4 &r, float4 &gq) {
    const float s2 = r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w;
    const float inv_s = 1.0f / sqrtf(s2);
    const float dot = (gq.x * r.x + gq.y * r.y + gq.z * r.z + gq.w * r.w) * (inv_s * inv_s * inv_s);
    gq = make_float4(gq.x * inv_s - r.x * dot, gq.y * inv_s - r.y * dot, gq.z * inv_s - r.z * dot, gq.w * inv_s - r.w * dot);
}
// Last phase of a fused backward + Adam for the 64 splats [g0, g0+64) of one wave: the lane that owns splat g0+lane
// holds its parameter gradients and sends them straight through the optimizer update of their parameter; the rows of
// v_sh / v_means / v_scales travel through the wave's LDS staging rows (odd row stride, so the column writes are
// bank-conflict free) to leave as contiguous 16-byte-per-lane streams.  v_xy (nullable) is still stored: the
// refinement reads it.  `stage`: the wave's private LDS, max(64 * (row floats | 1), 512) floats.
// ROWS_READY: the caller has already summed the v_sh rows of several views in `stage` (Y / vcol unused); `row_t0` then
// holds, per row of the wave, the time its deferred SH block is current for.
template <int DEG, bool ROWS_READY>
__device__ __forceinline__ void adam_step_wave(
    const AdamFuse &af, uint32_t n, uint32_t g0, uint32_t lane, float *stage, const uint32_t *row_t0,
    const float o_mean[3], const float o_scale[3], const float o_quat[4], float o_opac, const float o_xy[2],
    float stat_norm, float stat_count, const float *Y, const float vcol[3], float *__restrict__ v_xy) {
    constexpr uint32_t ncoef = (DEG + 1) * (DEG + 1);
    constexpr uint32_t kRow = ncoef * 3;     // floats per v_sh row
    constexpr uint32_t kRowPad = kRow | 1u;  // odd LDS row stride: conflict-free column access
    const uint32_t g_own = g0 + lane;
    const bool in_range = g_own < n;
    const uint32_t rows = min(kWave, n - g0);  // rows this wave owns (64 except at the tail)
    const size_t nn = n;
    if (in_range) {
        if (v_xy) reinterpret_cast<float2 *>(v_xy)[g_own] = make_float2(o_xy[0], o_xy[1]);
        float4 r = reinterpret_cast<const float4 *>(af.rotation)[g_own];
        float4 gq = make_float4(o_quat[0], o_quat[1], o_quat[2], o_quat[3]);
        if (af.quat_vjp) quat_norm_vjp(r, gq);
        const size_t e = 6 * nn + (size_t)g_own * 4;
        if (af.vec_ok) {
            r = adam_elem4(af, e, gq, r, af.lr[2]);
        } else {
            r.x = adam_elem(af, e + 0, gq.x, r.x, af.lr[2]);
            r.y = adam_elem(af, e + 1, gq.y, r.y, af.lr[2]);
            r.z = adam_elem(af, e + 2, gq.z, r.z, af.lr[2]);
            r.w = adam_elem(af, e + 3, gq.w, r.w, af.lr[2]);
        }
        reinterpret_cast<float4 *>(af.rotation)[g_own] = r;
        if (af.norm_rot_out) {  // what the next forward will be fed (gaussian_splats.rs:174-175)
            const float s = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
            reinterpret_cast<float4 *>(af.norm_rot_out)[g_own] = make_float4(r.x / s, r.y / s, r.z / s, r.w / s);
        }
        if (af.grad_2d_accum) {  // train.rs:284-316
            af.grad_2d_accum[g_own] += stat_norm * af.stat_scale;
            if (stat_count != 0.0f) af.xy_grad_counts[g_own] += stat_count;
        }
        af.raw_opac[g_own] = adam_elem(af, 10 * nn + g_own, o_opac, af.raw_opac[g_own], af.lr[3]);
    }

    // Steps `rows` rows of ROWF floats of the parameter array `dst` in place, contiguous across lanes, with the staged
    // gradients (row r at stage[r*STRIDE]); `seg` is the segment's offset in the moment arrays.
    auto step_rows = [&](float *dst, uint32_t rowf, uint32_t stride, size_t seg, float lr, bool is_sh) {
        const uint32_t total = rows * rowf;  // floats; dst is 16-B aligned when g0*rowf % 4 == 0
        if constexpr (ROWS_READY) {
            if (is_sh && af.lazy.on()) {
                // Deferred Adam of the SH block (lazy_sh.hpp) in the data-parallel reduction: the blocks of splats NO view
                // saw are left alone, their step stays pending; a seen splat's block first replays what is pending, then
                // takes this step.  Rows are whole 16-byte chunks (make_lazy_sh).
                for (uint32_t j = lane * 4; j < total; j += kWave * 4) {
                    const uint32_t r = j / rowf, k0 = j - r * rowf;
                    const uint32_t t0 = row_t0[r];
                    if (t0 == kInvalid) continue;
                    float4 x = *reinterpret_cast<const float4 *>(dst + j);
                    float4 mo = *reinterpret_cast<const float4 *>(af.m1 + seg + j);
                    float4 vo = *reinterpret_cast<const float4 *>(af.m2 + seg + j);
                    lazy_replay4(af.lazy, t0, k0, mo, vo, x);
                    float4 v;
                    float *e = reinterpret_cast<float *>(&v);
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++) e[i] = stage[r * stride + k0 + i];
                    float4 st = adam_elem4(af, seg + j, v, x, mo, vo, lr);
                    sh_rest_lerp(af, k0, x, st);
                    *reinterpret_cast<float4 *>(dst + j) = st;
                }
                return;
            }
        }
        auto one = [&](uint32_t f) {
            const float gv = stage[(f / rowf) * stride + (f % rowf)];
            const float x = dst[f];
            const float st = adam_elem(af, seg + f, gv, x, lr);
            dst[f] = (is_sh && (f % rowf) >= 3) ? x * (1.0f - af.sh_lerp) + st * af.sh_lerp : st;
        };
        if (((rowf & 3u) == 0 || rows == kWave) && af.vec_ok) {
            // float4 path: rowf*64 is a multiple of 4 and the wave's base offset is 16-B aligned.  The three streams
            // of kUnroll chunks are requested before the first one is used — 12 KiB in flight per wave instead of 3
            // (the kernel runs three waves per SIMD and a request takes ~2 us under load: Little's law asks for
            // ~10 MB in flight on the chip at 5 TB/s, one chunk at a time gave 9).
            constexpr uint32_t kUnroll = 4;
            auto staged4 = [&](uint32_t j) {
                float4 v;
                float *e = reinterpret_cast<float *>(&v);
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    const uint32_t f = j + i;
                    e[i] = stage[(f / rowf) * stride + (f % rowf)];
                }
                return v;
            };
            for (uint32_t j0 = lane * 4; j0 < total; j0 += kWave * 4 * kUnroll) {
                float4 x[kUnroll], mo[kUnroll], vo[kUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    const uint32_t j = j0 + u * kWave * 4;
                    if (j + 4 <= total) {
                        x[u] = nt_load4(dst + j);
                        mo[u] = nt_load4(af.m1 + seg + j);
                        vo[u] = nt_load4(af.m2 + seg + j);
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    const uint32_t j = j0 + u * kWave * 4;
                    if (j + 4 <= total) {
                        const float4 v = staged4(j);
                        float4 st = adam_elem4(af, seg + j, v, x[u], mo[u], vo[u], lr);
                        if (is_sh) {
                            const uint32_t k0 = j % rowf;  // position in the SH row; a chunk may straddle rows
                            const float4 xo = x[u];
                            st.x = (k0 + 0) % rowf >= 3 ? xo.x * (1.0f - af.sh_lerp) + st.x * af.sh_lerp : st.x;
                            st.y = (k0 + 1) % rowf >= 3 ? xo.y * (1.0f - af.sh_lerp) + st.y * af.sh_lerp : st.y;
                            st.z = (k0 + 2) % rowf >= 3 ? xo.z * (1.0f - af.sh_lerp) + st.z * af.sh_lerp : st.z;
                            st.w = (k0 + 3) % rowf >= 3 ? xo.w * (1.0f - af.sh_lerp) + st.w * af.sh_lerp : st.w;
                        }
                        nt_store4(dst + j, st);
                    } else if (j < total) {
                        for (uint32_t f = j; f < total; f++) one(f);
                    }
                }
            }
        } else {
            for (uint32_t f = lane; f < total; f += kWave) one(f);
        }
    };

    // v_sh: row = Y[k] * v_rgb
    {
        if (!ROWS_READY) {
            float *row = stage + lane * kRowPad;
#pragma unroll
            for (uint32_t k = 0; k < ncoef; k++) {
                row[k * 3 + 0] = Y[k] * vcol[0];
                row[k * 3 + 1] = Y[k] * vcol[1];
                row[k * 3 + 2] = Y[k] * vcol[2];
            }
        }
        __builtin_amdgcn_wave_barrier();
        step_rows(af.sh + (size_t)g0 * kRow, kRow, kRowPad, 11 * nn + (size_t)g0 * kRow, af.lr[4], true);
        __builtin_amdgcn_wave_barrier();
    }
    // v_means, v_scales: 3 floats per row
    {
        stage[lane * 4 + 0] = o_mean[0];
        stage[lane * 4 + 1] = o_mean[1];
        stage[lane * 4 + 2] = o_mean[2];
        stage[256 + lane * 4 + 0] = o_scale[0];
        stage[256 + lane * 4 + 1] = o_scale[1];
        stage[256 + lane * 4 + 2] = o_scale[2];
        __builtin_amdgcn_wave_barrier();
        step_rows(af.means + (size_t)g0 * 3, 3, 4, (size_t)g0 * 3, af.lr[0], false);
        stage += 256;
        step_rows(af.log_scales + (size_t)g0 * 3, 3, 4, 3 * nn + (size_t)g0 * 3, af.lr[1], false);
    }
}

}  // namespace
}  // namespace brush
