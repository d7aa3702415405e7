// bilagrid.hip — per-view bilateral grids: a low-resolution 3D lattice of the 3x4 affine colour maps of exposure.hip,
// indexed by pixel position and by the pixel's own luminance, sliced through the render before the loss
// (brush_bilagrid_forward, _backward, _backward_adam; Wang et al., "Bilateral Guided Radiance Field Processing", 2024;
// gsplat's use_bilateral_grid).  All f32 below, round to nearest, -ffp-contract=off, in the order written.
//
// Grid.  G[GL][GH][GW][12] f32, vertex-major; the 12 words of a vertex are the row-major [A | b] of exposure.hip.
//   2 <= GW, GH <= 64, 2 <= GL <= 8; image sides <= 32768, w h < 2^28.
// Coordinates of pixel (x, y), exact in integers:  w == 1: i0 = 0, fx = 0;  otherwise n = x (GW-1),
//   i0 = min(n div (w-1), GW-2), fx = float(n - i0 (w-1)) / float(w-1) (one f32 division of two exact integers; the last
//   column gets i0 = GW-2, fx = 1).  y, h, GH give j0, fy the same way (align_corners, border clamp).
// Guidance, on the premultiplied render p = (r, g, b, a):  lum = (0.299f r + 0.587f g) + 0.114f b;
//   lc = lum > 0 ? min(lum, 1) : 0 (a NaN gives 0: no float-to-int conversion sees a NaN or a value outside [0, GL-1]);
//   z = lc float(GL-1), k0 = min((int) z, GL-2), fz = z - float(k0);  inside = lum > 0 && lum < 1.
// Slice, lerp(a, b, f) = a + f (b - a), per word and for k in {k0, k0+1}:
//   L_k = lerp(lerp(G[k][j0][i0], G[k][j0][i0+1], fx), lerp(G[k][j0+1][i0], G[k][j0+1][i0+1], fx), fy)
//   M = lerp(L_k0, L_k0+1, fz)      S = L_k0+1 - L_k0
// Forward (the exposure kernel's expression):  out_c = ((M[4c] r + M[4c+1] g) + M[4c+2] b) + a M[4c+3],  out_a = a.
// Backward, v' = d L / d out:
//   q = inside ? float(GL-1) ((t_0 + t_1) + t_2) : 0,  t_c = v'_c (((S[4c] r + S[4c+1] g) + S[4c+2] b) + a S[4c+3])
//   v_r = ((M[0] v'_0 + M[4] v'_1) + M[8] v'_2) + 0.299f q   (v_g, v_b: words 1 / 2 and 0.587f / 0.114f)
//   v_a = v'_a + ((M[3] v'_0 + M[7] v'_1) + M[11] v'_2)
//   v_G[k][j][i][4c+m] = sum_pixels W v'_c p_m,  W = (X Y) Z in float64 from the f32 fx, fy, fz: X = 1 - fx at i = i0,
//   fx at i = i0+1, 0 elsewhere; Y, Z likewise.  The products v'_c p_m are exact in float64; a term is
//   ((X Y) Z) (v'_c p_m), added in float64.  A vertex no pixel reaches gets exactly +0.
// Prior.  TV(G) = sum over the three axes of the mean, over all adjacent vertex pairs along the axis and all 12 words,
//   of (G[v+e] - G[v])^2;  tv dTV/dG is added to v_G in front of Adam (float64), not to any reported loss.
// Consequences of the lerp form: lerp(a, a, f) = a exactly, so the identity grid returns pred bit for bit, and a grid
// whose vertices all hold E gives brush_exposure_forward's bits (S = 0: q = +-0, v_pred equals the exposure backward's).
//
//   k_bilagrid_forward  : one pixel per lane, one 16-byte load and one 16-byte store; the 8 vertices of the pixel come
//       straight from the cache as 24 16-byte loads (the default grid is 98 KB; no LDS staging).
//   k_bilagrid_backward : one workgroup per CELL (i0, j0) of the lattice and per slice of the cell's pixel rows (the
//       pixels of a cell form a rectangle, computable in integers; the slice count is a function of w, h, GW, GH only).
//       Every pixel belongs to exactly one cell, so one workgroup alone reads and writes it: v_pred may alias v_out (a
//       lane reads its pixels in every pass before it writes them in the last).  Eight passes over the slice, one per
//       corner of the cell and half of the levels (0..3, 4..7; the upper half only when GL > 4), each with 4 x 12
//       float64 accumulators per lane (level k gets the tent weight of z at k with compile-time indices; a level no
//       lane of the wave touches is skipped, which changes no bit), finished by block_sum_words<48> (fixed_sum.hpp,
//       waves in order) into the half's 48 doubles of the row of 96 per (cell, slice, corner) with ordinary stores.
//       Lanes stride over the slice's pixels.  (Skipping, behind the pred load, 64 pixels none of which has a weight
//       in the pass's half put the v_out load behind a wait and measured 25 us slower at 1080p.)
//       48 accumulators and not 96: with 96 the kernel needs 406 registers, 150 of them AGPRs that every update copies
//       in and out, at one wave per SIMD (measured: 314 us at 1080p against the figure in DESIGN §8 row 24).  A last
//       pass writes v_pred.  With `prior` (the Adam entry) the workgroups also write
//       tv dTV/dG of the PRE-STEP grid, one double per word, into a second buffer: the prior at a vertex reads its six
//       neighbours, which another workgroup of the finalize launch may already have stepped, so it is taken here, where
//       G is only read.
//   k_bilagrid_finalize<ADAM> : one thread per grid word: adds the rows of the up to four cells around the vertex (cell
//       rows ascending, then cell columns, then slices, a fixed order), writes v_G as f32, zeros included; with ADAM it
//       adds the prior's word and steps G, m1, m2 in place as k_exposure_finalize<true> does (float64 from the stored
//       f32 words, each stored word rounded once).
// No atomics, no counters, no allocation, no synchronisation: graph-capturable, the same inputs give the same bits.
#include <cmath>

#include "fixed_sum.hpp"
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = kSumThreads;
constexpr uint32_t kVertexWords = 12;  // row-major 3x4: [A row c | b_c]
constexpr uint32_t kMaxLevels = 8;
constexpr uint32_t kRowWords = kMaxLevels * kVertexWords;  // one corner of one cell slice: 96 doubles
constexpr uint32_t kCorners = 4;
constexpr uint32_t kHalfLevels = kMaxLevels / 2;
constexpr uint32_t kHalfWords = kHalfLevels * kVertexWords;  // what one pass of the backward accumulates: 48 doubles
// The backward runs two waves per SIMD: two workgroups per CU.
constexpr uint32_t kTargetGroups = 512;
constexpr uint32_t kMinSliceRows = 8;
constexpr uint32_t kMaxSide = 32768;

struct GridDims {
    uint32_t gw, gh, gl, w, h;
};

// First pixel of cell c along an axis of `w` pixels and `g` vertices; cell g-2 runs to w (the border clamp).
__host__ __device__ static inline uint32_t cell_first(uint32_t c, uint32_t w, uint32_t g) {
    if (c >= g - 1) return w;
    if (w == 1) return c == 0 ? 0u : 1u;
    return ceil_div(c * (w - 1), g - 1);
}
__device__ __forceinline__ uint32_t cell_of(uint32_t x, uint32_t w, uint32_t g) {
    return w == 1 ? 0u : min(x * (g - 1) / (w - 1), g - 2);
}
// f of pixel x in its cell i0.
__device__ __forceinline__ float cell_frac(uint32_t x, uint32_t i0, uint32_t w, uint32_t g) {
    if (w == 1) return 0.f;
    return (float)(x * (g - 1) - i0 * (w - 1)) / (float)(w - 1);
}

// Bound on the pixel rows of a cell, and the slices the backward cuts every cell's rows into.
static inline uint32_t slice_count(const GridDims &d) {
    const uint32_t cells = (d.gw - 1) * (d.gh - 1);
    const uint32_t rows_max = min(d.h, ceil_div(d.h - 1, d.gh - 1) + 1);
    return min(max(1u, kTargetGroups / cells), ceil_div(rows_max, kMinSliceRows));
}

struct Guide {
    uint32_t k0;
    float fz;
    bool inside;
};
__device__ __forceinline__ Guide guidance(const float4 p, uint32_t gl) {
    const float lum = (0.299f * p.x + 0.587f * p.y) + 0.114f * p.z;
    const float lc = lum > 0.f ? (lum < 1.f ? lum : 1.f) : 0.f;
    const float z = lc * (float)(gl - 1);
    Guide g;
    g.k0 = min((uint32_t)(int)z, gl - 2);
    g.fz = z - (float)g.k0;
    g.inside = lum > 0.f && lum < 1.f;
    return g;
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

// M (and S when WITH_S) of the pixel with cell (i0, j0, k0) and fractions (fx, fy, fz).
template <bool WITH_S>
__device__ __forceinline__ void slice_grid(const float4 *__restrict__ G, const GridDims &d, uint32_t i0, uint32_t j0,
                                           uint32_t k0, float fx, float fy, float fz, float (&M)[kVertexWords],
                                           float (&S)[kVertexWords]) {
    const float4 *v0 = G + (size_t)((k0 * d.gh + j0) * d.gw + i0) * 3;
    const float4 *v1 = v0 + (size_t)d.gh * d.gw * 3;
#pragma unroll
    for (uint32_t q = 0; q < 3; q++) {
        float L[2][4];
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const float4 *v = k ? v1 : v0;
            const float4 a = v[q], b = v[3 + q], c = v[d.gw * 3 + q], e = v[d.gw * 3 + 3 + q];
            L[k][0] = lerp(lerp(a.x, b.x, fx), lerp(c.x, e.x, fx), fy);
            L[k][1] = lerp(lerp(a.y, b.y, fx), lerp(c.y, e.y, fx), fy);
            L[k][2] = lerp(lerp(a.z, b.z, fx), lerp(c.z, e.z, fx), fy);
            L[k][3] = lerp(lerp(a.w, b.w, fx), lerp(c.w, e.w, fx), fy);
        }
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            M[q * 4 + m] = lerp(L[0][m], L[1][m], fz);
            if constexpr (WITH_S) S[q * 4 + m] = L[1][m] - L[0][m];
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_bilagrid_forward(const float4 *__restrict__ pred,
                                                               const float4 *__restrict__ G, const GridDims d,
                                                               uint32_t npix, float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= npix) return;
    const uint32_t y = i / d.w, x = i - y * d.w;
    const float4 p = pred[i];
    const uint32_t i0 = cell_of(x, d.w, d.gw), j0 = cell_of(y, d.h, d.gh);
    const Guide g = guidance(p, d.gl);
    float M[kVertexWords], S[kVertexWords];
    slice_grid<false>(G, d, i0, j0, g.k0, cell_frac(x, i0, d.w, d.gw), cell_frac(y, j0, d.h, d.gh), g.fz, M, S);
    float4 o;
    o.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + p.w * M[3];
    o.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + p.w * M[7];
    o.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + p.w * M[11];
    o.w = p.w;
    out[i] = o;
}

// tv dTV/dG at word e of the grid, in float64 from the stored words.
__device__ __forceinline__ double tv_gradient(const float *__restrict__ G, const GridDims &d, uint32_t e, double tv) {
    const uint32_t m = e % kVertexWords, vtx = e / kVertexWords;
    const uint32_t i = vtx % d.gw, j = (vtx / d.gw) % d.gh, k = vtx / (d.gw * d.gh);
    const uint32_t sx = kVertexWords, sy = d.gw * kVertexWords, sz = d.gh * d.gw * kVertexWords;
    const double g = (double)G[e];
    const double gx = (i > 0 ? g - (double)G[e - sx] : 0.0) - (i + 1 < d.gw ? (double)G[e + sx] - g : 0.0);
    const double gy = (j > 0 ? g - (double)G[e - sy] : 0.0) - (j + 1 < d.gh ? (double)G[e + sy] - g : 0.0);
    const double gz = (k > 0 ? g - (double)G[e - sz] : 0.0) - (k + 1 < d.gl ? (double)G[e + sz] - g : 0.0);
    const double cx = 2.0 / ((double)d.gl * d.gh * (d.gw - 1) * kVertexWords);
    const double cy = 2.0 / ((double)d.gl * (d.gh - 1) * d.gw * kVertexWords);
    const double cz = 2.0 / ((double)(d.gl - 1) * d.gh * d.gw * kVertexWords);
    (void)m;
    return tv * ((cx * gx + cy * gy) + cz * gz);
}

// v_out and v_pred may be the same array: neither is __restrict__.  rows: [cells x slices][4 corners][96].
__global__ __launch_bounds__(kThreads) void k_bilagrid_backward(const float4 *__restrict__ pred, const float4 *v_out,
                                                                const float *__restrict__ G, const GridDims d,
                                                                uint32_t slices, float4 *v_pred,
                                                                double *__restrict__ rows, double *__restrict__ prior,
                                                                double tv) {
    const uint32_t cell = blockIdx.x / slices, slice = blockIdx.x - cell * slices;
    const uint32_t cj = cell / (d.gw - 1), ci = cell - cj * (d.gw - 1);
    const uint32_t xa = cell_first(ci, d.w, d.gw), cw = cell_first(ci + 1, d.w, d.gw) - xa;
    const uint32_t ya = cell_first(cj, d.h, d.gh), yb = cell_first(cj + 1, d.h, d.gh);
    const uint32_t per = ceil_div(yb - ya, slices);
    const uint32_t ys = min(ya + slice * per, yb), ye = min(ys + per, yb);
    // Lanes stride over the slice's pixels in row-major order.
    const uint32_t count = cw * (ye - ys);  // 0 for a cell without pixels: its rows are written as zeros

    const uint32_t passes = d.gl > kHalfLevels ? 2 * kCorners : kCorners;  // the rows of levels >= GL are never read
#pragma unroll 1
    for (uint32_t pass = 0; pass < passes; pass++) {
        const uint32_t corner = pass % kCorners, first = pass / kCorners * kHalfLevels;
        double acc[kHalfWords];
#pragma unroll
        for (uint32_t i = 0; i < kHalfWords; i++) acc[i] = 0.0;
        for (uint32_t q = threadIdx.x; q < count; q += kThreads) {
            const uint32_t row = q / cw, x = xa + (q - row * cw), y = ys + row;
            const size_t idx = (size_t)y * d.w + x;
            const float4 p = pred[idx];
            const float4 v = v_out[idx];
            const Guide g = guidance(p, d.gl);
            const double fx = (double)cell_frac(x, ci, d.w, d.gw), fy = (double)cell_frac(y, cj, d.h, d.gh);
            const double xy = ((corner & 1u) ? fx : 1.0 - fx) * ((corner & 2u) ? fy : 1.0 - fy);
            const double fz = (double)g.fz;
            const double pk[4] = {(double)p.x, (double)p.y, (double)p.z, (double)p.w};
            const double vc[3] = {(double)v.x, (double)v.y, (double)v.z};
            double t[kVertexWords];
#pragma unroll
            for (int c = 0; c < 3; c++) {
#pragma unroll
                for (int m = 0; m < 4; m++) t[c * 4 + m] = vc[c] * pk[m];
            }
#pragma unroll
            for (uint32_t k = 0; k < kHalfLevels; k++) {
                const double zk = first + k == g.k0 ? 1.0 - fz : (first + k == g.k0 + 1 ? fz : 0.0);
                if (__any(zk != 0.0)) {  // wave-uniform: a skipped level would only have added zeros
                    const double wk = xy * zk;
#pragma unroll
                    for (uint32_t m = 0; m < kVertexWords; m++) acc[k * kVertexWords + m] += wk * t[m];
                }
            }
        }
        double *row = rows + ((size_t)blockIdx.x * kCorners + corner) * kRowWords + first * kVertexWords;
        block_sum_words(acc, [&](uint32_t t, double sum) { row[t] = sum; });
        __syncthreads();  // the next pass stages its wave sums in the same LDS
    }

    const float4 *G4 = reinterpret_cast<const float4 *>(G);
    const float levels = (float)(d.gl - 1);
    for (uint32_t q = threadIdx.x; q < count; q += kThreads) {
        const uint32_t row = q / cw, x = xa + (q - row * cw), y = ys + row;
        const size_t idx = (size_t)y * d.w + x;
        const float4 p = pred[idx];
        const float4 v = v_out[idx];
        const Guide g = guidance(p, d.gl);
        float M[kVertexWords], S[kVertexWords];
        slice_grid<true>(G4, d, ci, cj, g.k0, cell_frac(x, ci, d.w, d.gw), cell_frac(y, cj, d.h, d.gh), g.fz, M, S);
        const float t0 = v.x * (((S[0] * p.x + S[1] * p.y) + S[2] * p.z) + p.w * S[3]);
        const float t1 = v.y * (((S[4] * p.x + S[5] * p.y) + S[6] * p.z) + p.w * S[7]);
        const float t2 = v.z * (((S[8] * p.x + S[9] * p.y) + S[10] * p.z) + p.w * S[11]);
        const float qz = g.inside ? levels * ((t0 + t1) + t2) : 0.f;
        float4 o;
        o.x = ((M[0] * v.x + M[4] * v.y) + M[8] * v.z) + 0.299f * qz;
        o.y = ((M[1] * v.x + M[5] * v.y) + M[9] * v.z) + 0.587f * qz;
        o.z = ((M[2] * v.x + M[6] * v.y) + M[10] * v.z) + 0.114f * qz;
        o.w = v.w + ((M[3] * v.x + M[7] * v.y) + M[11] * v.z);
        v_pred[idx] = o;
    }

    if (prior) {  // the prior of the pre-step grid: this launch only reads G
        const uint32_t words = d.gl * d.gh * d.gw * kVertexWords;
        for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < words; e += gridDim.x * kThreads)
            prior[e] = tv_gradient(G, d, e, tv);
    }
}

struct BilagridAdam {
    float *G, *m1, *m2;  // this view's grid words each, updated in place
    double lr, beta1, beta2, eps, tv, bc1, bc2;  // bc = 1 - beta^time
};

template <bool ADAM>
__global__ __launch_bounds__(kThreads) void k_bilagrid_finalize(const double *__restrict__ rows,
                                                                const double *__restrict__ prior, const GridDims d,
                                                                uint32_t slices, float *__restrict__ v_grid,
                                                                const BilagridAdam a) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= d.gl * d.gh * d.gw * kVertexWords) return;
    const uint32_t m = e % kVertexWords, vtx = e / kVertexWords;
    const uint32_t i = vtx % d.gw, j = (vtx / d.gw) % d.gh, k = vtx / (d.gw * d.gh);
    double sum = 0.0;
    for (uint32_t cj = (j > 0 ? j - 1 : 0); cj <= min(j, d.gh - 2); cj++) {
        for (uint32_t ci = (i > 0 ? i - 1 : 0); ci <= min(i, d.gw - 2); ci++) {
            const uint32_t corner = (i - ci) + 2 * (j - cj);
            const size_t first = (size_t)(cj * (d.gw - 1) + ci) * slices;
            for (uint32_t s = 0; s < slices; s++)
                sum += rows[((first + s) * kCorners + corner) * kRowWords + k * kVertexWords + m];
        }
    }
    v_grid[e] = (float)sum;
    if constexpr (ADAM) {
        const double x = (double)a.G[e];
        const double g = sum + prior[e];
        const double m1 = a.beta1 * (double)a.m1[e] + (1.0 - a.beta1) * g;
        const double m2 = a.beta2 * (double)a.m2[e] + (1.0 - a.beta2) * (g * g);
        a.m1[e] = (float)m1;
        a.m2[e] = (float)m2;
        a.G[e] = (float)(x - a.lr * (m1 / a.bc1) / (sqrt(m2 / a.bc2) + a.eps));
    }
}

// 0 unless the grid and the image are in range; the pixel count otherwise.
uint32_t checked_dims(uint32_t gw, uint32_t gh, uint32_t gl, uint32_t w, uint32_t h) {
    if (gw < 2 || gw > 64 || gh < 2 || gh > 64 || gl < 2 || gl > kMaxLevels) return 0;
    if (w > kMaxSide || h > kMaxSide) return 0;
    return checked_pixels(w, h);
}
size_t rows_bytes(const GridDims &d) {
    return align_up((size_t)(d.gw - 1) * (d.gh - 1) * slice_count(d) * kCorners * kRowWords * sizeof(double), 256);
}
size_t prior_bytes(const GridDims &d) {
    return align_up((size_t)d.gl * d.gh * d.gw * kVertexWords * sizeof(double), 256);
}

int backward_common(const float *pred, const float *v_out, const float *grid, uint32_t gw, uint32_t gh, uint32_t gl,
                    uint32_t w, uint32_t h, float *v_pred, float *v_grid, void *workspace, size_t workspace_bytes,
                    const BilagridAdam *adam, brush_stream_t stream) {
    const uint32_t npix = checked_dims(gw, gh, gl, w, h);
    if (!npix || !pred || !v_out || !grid || !v_pred || !v_grid || !workspace) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(v_out, 16) || misaligned(v_pred, 16) || misaligned(grid, 16) ||
        misaligned(v_grid, 4) || misaligned(workspace, 8) || v_pred == pred)
        return BRUSH_ERR_INVALID_ARG;
    const GridDims d{gw, gh, gl, w, h};
    if (workspace_bytes < rows_bytes(d) + prior_bytes(d)) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *rows = static_cast<double *>(workspace);
    double *prior = reinterpret_cast<double *>(static_cast<char *>(workspace) + rows_bytes(d));
    const uint32_t slices = slice_count(d), groups = (gw - 1) * (gh - 1) * slices;
    const uint32_t word_groups = ceil_div(gl * gh * gw * kVertexWords, kThreads);
    hipLaunchKernelGGL(k_bilagrid_backward, dim3(groups), dim3(kThreads), 0, s, reinterpret_cast<const float4 *>(pred),
                       reinterpret_cast<const float4 *>(v_out), grid, d, slices, reinterpret_cast<float4 *>(v_pred), rows,
                       adam ? prior : nullptr, adam ? adam->tv : 0.0);
    if (adam)
        hipLaunchKernelGGL(k_bilagrid_finalize<true>, dim3(word_groups), dim3(kThreads), 0, s, rows, prior, d, slices,
                           v_grid, *adam);
    else
        hipLaunchKernelGGL(k_bilagrid_finalize<false>, dim3(word_groups), dim3(kThreads), 0, s, rows, prior, d, slices,
                           v_grid, BilagridAdam{});
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_bilagrid_workspace_size(uint32_t w, uint32_t h, uint32_t gw, uint32_t gh, uint32_t gl,
                                             size_t *bytes) {
    if (!bytes || !checked_dims(gw, gh, gl, w, h)) return BRUSH_ERR_INVALID_ARG;
    const GridDims d{gw, gh, gl, w, h};
    *bytes = rows_bytes(d) + prior_bytes(d);
    return BRUSH_OK;
}

extern "C" int brush_bilagrid_forward(const float *pred, const float *grid, uint32_t gw, uint32_t gh, uint32_t gl,
                                      uint32_t w, uint32_t h, float *out, brush_stream_t stream) {
    const uint32_t npix = checked_dims(gw, gh, gl, w, h);
    if (!npix || !pred || !grid || !out || out == pred) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(out, 16) || misaligned(grid, 16)) return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_bilagrid_forward, dim3(ceil_div(npix, kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const float4 *>(pred),
                       reinterpret_cast<const float4 *>(grid), GridDims{gw, gh, gl, w, h}, npix,
                       reinterpret_cast<float4 *>(out));
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_bilagrid_backward(const float *pred, const float *v_out, const float *grid, uint32_t gw,
                                       uint32_t gh, uint32_t gl, uint32_t w, uint32_t h, float *v_pred, float *v_grid,
                                       void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    return backward_common(pred, v_out, grid, gw, gh, gl, w, h, v_pred, v_grid, workspace, workspace_bytes, nullptr,
                           stream);
}

extern "C" int brush_bilagrid_backward_adam(const float *pred, const float *v_out, const BrushBilagridAdam *cfg,
                                            uint32_t gw, uint32_t gh, uint32_t gl, uint32_t w, uint32_t h,
                                            float *v_pred, float *grid, float *moment1, float *moment2, float *v_grid,
                                            void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    if (!cfg || cfg->time == 0 || !moment1 || !moment2 || misaligned(moment1, 4) || misaligned(moment2, 4))
        return BRUSH_ERR_INVALID_ARG;
    BilagridAdam a;
    a.G = grid, a.m1 = moment1, a.m2 = moment2;
    a.lr = (double)cfg->lr, a.beta1 = (double)cfg->beta1, a.beta2 = (double)cfg->beta2;
    a.eps = (double)cfg->epsilon, a.tv = (double)cfg->tv;
    a.bc1 = 1.0 - std::pow(a.beta1, (double)cfg->time);
    a.bc2 = 1.0 - std::pow(a.beta2, (double)cfg->time);
    return backward_common(pred, v_out, grid, gw, gh, gl, w, h, v_pred, v_grid, workspace, workspace_bytes, &a, stream);
}
