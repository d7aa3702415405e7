// raster_common.hpp — what the two compositing translation units share: rasterize.hip (forward) and rasterize_bwd.hip
// (backward).  The workgroup shape, the wave-local LDS hand-off, the quadrant bound of the footprint-aware kernels and
// the XCD-contiguous block remap.
#pragma once
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kBatch = kWave;  // 64 splats per LDS batch, one per lane
constexpr float kNegLog2e = -1.44269504088896341f;  // exp(-s) = exp2(kNegLog2e * s)

constexpr uint32_t kTilesPerBlock = 4;  // 4 independent wave64s per 256-thread workgroup
constexpr uint32_t kRasterThreads = kTilesPerBlock * kWave;

// The waves of a workgroup never exchange data: LDS hand-offs are wave-local, the LDS queue of a
// wave is in order, so a compiler-level barrier is all that is needed (no s_barrier).
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

// Workgroups are dealt to the 8 XCDs round-robin; this gives every XCD a contiguous band of the grid instead, so that
// neighbouring tiles gather the same splat records from one L2.  The grid is a multiple of 8 workgroups.
__device__ __forceinline__ uint32_t xcd_contiguous_block() {
    return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

// ---- footprint-aware kernels -----------------------------------------------------------------
//
// Measured on the headline scene (profiles/r02a_footprint_s1.json): only 26 % of the 256 pixel
// evaluations of a (tile, splat) record pass `sigma >= 0 && alpha >= 1/255`; at 8x8 granularity a
// record touches 2.1 of the tile's 4 quadrants on average.  An evaluation that fails the test
// changes nothing (rasterize.wgsl:80-87, rasterize_backwards.wgsl:229-242), so whole quadrants a
// splat provably cannot reach are skipped with wave-uniform (scalar) control flow:
//   * quad_may_pass(): EXACT minimum of the splat's quadratic form over the box of the quadrant's
//     pixel centres (for a positive-definite conic the constrained minimiser lies on the line through
//     the box face nearest to the mean in x or in y, see the derivation at the function), turned
//     into an upper bound of alpha with a slack far above the rounding error of the per-pixel
//     arithmetic.  A quadrant is skipped only when that bound is below 0.99/255; anything not
//     provably positive definite / finite is never skipped.
//   * one lane evaluates the bound for one staged record, a ballot gives the 64-bit hit mask of the
//     batch, and the compositing loop walks its set bits on the scalar unit.
// Lane mask of a predicate straight from the compare (HIP's __ballot() converts the bool to an int and
// compares it again: two VALU instructions per call).
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Largest alpha the splat can reach at any point of the box [bx, bx+7] x [by, by+7] (pixel centres
// of one 8x8 quadrant) >= 1/255 ?  d = mean - pixel ranges over [dxl,dxh] x [dyl,dyh]; q(d) =
// 0.5 (a dx^2 + c dy^2) + b dx dy is convex with its minimum 0 at d = 0.  If the box does not contain 0
// the minimiser d* sits on the boundary, and (KKT + positive definiteness) at least one coordinate
// is at the bound NEAREST to 0 of an axis whose range excludes 0: a minimiser on a far face with
// the other coordinate free would need dx (a - b^2/c) <= 0, and both coordinates on far faces would
// need q(d*) <= 0.  So min q = min( min_dy q(ex, dy), min_dx q(dx, ey) ) with ex, ey the clamps of 0
// into the ranges; each 1-D problem is a clamped parabola vertex.  (If a range contains 0 its line
// runs through the box: a feasible point, so it can only raise that candidate, never the minimum.)
__device__ __forceinline__ bool quad_may_pass(float mx, float my, float ca, float cb, float cc, float opac,
                                              float bx, float by) {
    const float dxl = mx - (bx + 7.0f), dxh = mx - bx;
    const float dyl = my - (by + 7.0f), dyh = my - by;
    const float ex = fminf(fmaxf(0.0f, dxl), dxh), ey = fminf(fmaxf(0.0f, dyl), dyh);
    // parabola vertices with v_rcp_f32 (1 ulp): q is stationary there, so the error is second order
    const float y1 = fminf(fmaxf(-cb * ex * __builtin_amdgcn_rcpf(cc), dyl), dyh);
    const float x2 = fminf(fmaxf(-cb * ey * __builtin_amdgcn_rcpf(ca), dxl), dxh);
    const float s1 = 0.5f * (ca * ex * ex + cc * y1 * y1), c1 = cb * ex * y1;
    const float s2 = 0.5f * (ca * x2 * x2 + cc * ey * ey), c2 = cb * x2 * ey;
    const float qmin = fminf(s1 + c1, s2 + c2);
    // slack: 0.02 absolute plus 4e-6 of the magnitude of the terms (f32 rounding of the per-pixel
    // evaluation is ~1e-7 of the same terms)
    const float slack = 0.02f + 4e-6f * fmaxf(s1 + fabsf(c1), s2 + fabsf(c2));
    const float amax = opac * __builtin_amdgcn_exp2f((qmin - slack) * kNegLog2e);
    const bool pd = ca > 0.0f && cc > 0.0f && ca * cc > cb * cb;
    return !pd || !(amax < 0.99f / 255.0f);  // NaN anywhere -> keep
}

// v_min_f32 without the canonicalising v_max the IEEE-mode lowering of fminf() puts in front of it.
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The one element of an optional trailing argument pack (the depth instantiations' DepthOut / DepthGrad).
template <typename T>
__device__ __forceinline__ const T &only(const T &x) { return x; }

}  // namespace
}  // namespace brush
