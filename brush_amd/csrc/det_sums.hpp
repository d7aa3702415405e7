// det_sums.hpp — where the compact-order gradient sums of a visible splat come from, and the word layout of the two kinds
// of kCompactStride-float rows that carry them:
//   compact row       v_compact[c], partials[..]:                      [9 sums | v_z | ...]
//   intersection row  rows[u] (deterministic mode, emission order):    [9 sums | compact gid | v_z | ...]
// v_z: the gradient of the accumulated depth (brush_render_backward_depth).
#pragma once
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kSumWords = 9, kCompactDepthWord = 9, kIsectGidWord = 9, kIsectDepthWord = 10;

// Deterministic mode (BRUSH_DETERMINISTIC=1): the compositing backward writes one intersection row per intersection,
// grouped by splat.
//   k_sum_isect_rows   one lane per row, segmented scan inside each 64-row chunk: a splat whose rows lie inside one
//                      chunk gets its sum in v_compact[c]; a splat that crosses chunk borders leaves partial sums
//                      partials[chunk][0] (rows of a splat that began in an earlier chunk) / [1] (rows of a splat
//                      that continues into the next chunk), which its consumer adds in chunk order.
//   k_sum_isect_depth  the same for v_z alone, after that kernel.
// Same rows, same tree, same order every run: bitwise reproducible, no atomics, no zero-fill.
struct DetSums {
    const uint32_t *cum_tiles_hit;      // [N] inclusive (aux)
    const uint32_t *num_intersections;  // [1]
    const float *partials;              // [ceil(cap / 64)][2][kCompactStride]; nullptr = atomic mode
    uint32_t cap;
};
inline DetSums make_det_sums(const DetSumsArgs &a) { return {a.cum_tiles_hit, a.num_intersections, a.partials, a.cap}; }

// The surviving intersection rows [u0, u1) of compact splat c, of I rows in all.
__device__ __forceinline__ void isect_range(const uint32_t *cum_tiles_hit, uint32_t I, uint32_t c, uint32_t &u0,
                                            uint32_t &u1) {
    u0 = c ? min(cum_tiles_hit[c - 1], I) : 0u, u1 = min(cum_tiles_hit[c], I);
}

// The sums of compact splat c: its compact row (atomic mode, or all its rows in one chunk), or its partial rows added in
// chunk order.  (load_compact_depth walks the same way; one walk with the readers as functors changes its kernel's code.)
__device__ __forceinline__ void load_compact_sums(const float *__restrict__ v_compact, const DetSums &det, uint32_t c,
                                                  float4 &r0, float4 &r1, float4 &r2) {
    const float4 *row = reinterpret_cast<const float4 *>(v_compact) + (size_t)c * (kCompactStride / 4);
    if (!det.partials) {
        r0 = row[0], r1 = row[1], r2 = row[2];
        return;
    }
    const uint32_t I = min(*det.num_intersections, det.cap);
    uint32_t u0, u1;
    isect_range(det.cum_tiles_hit, I, c, u0, u1);
    r0 = r1 = r2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u1 <= u0) return;  // no intersection survived (exact tile test / capacity): zero gradient
    const uint32_t k0 = u0 / kWave, k1 = (u1 - 1u) / kWave;
    if (k0 == k1) {
        r0 = row[0], r1 = row[1], r2 = row[2];
        return;
    }
    for (uint32_t k = k0; k <= k1; k++) {  // chunk order
        const float4 *p = reinterpret_cast<const float4 *>(det.partials) + ((size_t)k * 2 + (k == k0 ? 1 : 0)) * kCompactVec;
        const float4 a = p[0], b = p[1], d = p[2];
        r0.x += a.x, r0.y += a.y, r0.z += a.z, r0.w += a.w;
        r1.x += b.x, r1.y += b.y, r1.z += b.z, r1.w += b.w;
        r2.x += d.x;
    }
}

__device__ __forceinline__ float load_compact_depth(const float *__restrict__ v_compact, const DetSums &det, uint32_t c) {
    const float *row = v_compact + (size_t)c * kCompactStride;
    if (!det.partials) return row[kCompactDepthWord];
    const uint32_t I = min(*det.num_intersections, det.cap);
    uint32_t u0, u1;
    isect_range(det.cum_tiles_hit, I, c, u0, u1);
    if (u1 <= u0) return 0.0f;
    const uint32_t k0 = u0 / kWave, k1 = (u1 - 1u) / kWave;
    if (k0 == k1) return row[kCompactDepthWord];
    float v = 0.0f;
    for (uint32_t k = k0; k <= k1; k++)  // chunk order
        v += det.partials[((size_t)k * 2 + (k == k0 ? 1 : 0)) * kCompactStride + kCompactDepthWord];
    return v;
}

}  // namespace
}  // namespace brush
