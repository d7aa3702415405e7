// normal_loss.hip — normal maps and the depth-normal consistency loss of the surface-oriented splat trainers (2DGS, GOF,
// RaDe-GS, PGSR): L_n = sum_i w_i (1 - n_i . N), n_i the normal of splat i, w_i its blending weight, N the normal of the
// surface the rendered depth map implies.  Three entry points (include/brush_hip.h):
//   brush_splat_normals            one lane per splat: the shortest axis in camera space, turned towards the camera
//   brush_splat_normals_backward   its VJP into the quaternions (ADDED into v_quats)
//   brush_normal_loss              per pixel: depth map -> normals, the loss and its three gradients, one launch + finalize
//
// EVALUATION ORDER.  Everything below is float32, one rounding per written operation (-ffp-contract=off, IEEE / and
// sqrtf), parentheses as written; tests/normal_ref64.py restates it in numpy float32 and is held to the bit.
//   dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
//   cross(a, b) = (a1 b2 - a2 b1,  a2 b0 - a0 b2,  a0 b1 - a1 b0)
// Splat normals, W[r][c] = viewmat[4 c + r], t[r] = viewmat[12 + r]:
//   k = 0; if (l1 < l0) k = 1; if (l2 < l_k) k = 2                      (lowest index among equals; a NaN moves nothing)
//   a = column k of quat_to_rotmat(q)                                    (splat_math.hpp)
//   n_c[r] = (W[r][0] a0 + W[r][1] a1) + W[r][2] a2
//   p_c[r] = ((W[r][0] m0 + W[r][1] m1) + W[r][2] m2) + t[r]             (to_view)
//   s = dot(n_c, p_c) > 0 ? -1 : +1;   out = s n_c
//   backward: v_a[c] = s ((W[0][c] v0 + W[1][c] v1) + W[2][c] v2);  v_R = v_a in column k, +0 elsewhere;
//             v_quats[g] += quat_to_rotmat_vjp(q, v_R)                   (splat_vjp.hpp, the whole formula)
// Pixel kernel, kappa = (float)((double) weight / (w h)), A = pred[q].w, D = depth[q]:
//   counts(q) = A >= alpha_min and D > 0 and A < inf and D < inf          (a NaN fails)
//   z = D / A;  rx(x) = (((float) x + 0.5) - cx) / fx;  ry(y) likewise;  P(x, y) = (z rx(x), z ry(y), z)
//   tx = P(x+1, y) - P(x-1, y);  ty = P(x, y+1) - P(x, y-1);  c = cross(ty, tx);  m = dot(c, c)
//   valid(p) = interior and counts at p and its four edge neighbours and m > 0 and m < inf
//   len = sqrtf(m);  Nd = c / len;  l = A - dot(Nr, Nd);  the loss sums (double) l
//   v_normals_img = (-kappa) Nd;  v_Nd = (-kappa) Nr;  d = dot(Nd, v_Nd);  v_c = (v_Nd - Nd d) / len
//   v_ty = cross(tx, v_c);  v_tx = cross(v_c, ty)                         (+0 at an invalid centre and off the frame)
//   v_P(q) = ((v_tx(x-1, y) - v_tx(x+1, y)) + v_ty(x, y-1)) - v_ty(x, y+1)
//   v_z = (v_P0 rx + v_P1 ry) + v_P2;  v_depth = counts ? v_z / A : 0
//   touched(q) = valid(q) or one of the four centres beside q is valid
//   touched: v_pred[q].w += (valid ? kappa : 0) - (v_z D) / (A A)
//
// LAUNCH FORM: one launch.  A workgroup of 256 lanes takes 16x16 tiles: it stages z and counts of the tile plus a 2-pixel
// halo in LDS (20x20), computes Nd, v_tx, v_ty of the tile plus a 1-pixel halo (18x18 centres) into LDS, and every lane
// GATHERS v_P of its own pixel from there: no float atomics, no HBM scratch between two launches.  14 048 B of LDS per
// workgroup (47 VGPRs): the 32-wave limit (8 workgroups per CU), not LDS, bounds the occupancy.  The centre arrays are
// structure-of-arrays, so consecutive lanes read consecutive words.  The halo centres are computed by two tiles (1.27x
// the centre arithmetic, 1.56x the depth / alpha reads, served by the L2) against a second launch's 40 bytes per pixel
// written and read back through HBM.  The grid is capped as depth_loss.hip's (1024 workgroups, which stride over the
// tiles); the loss goes through the fixed-order sums of fixed_sum.hpp (one float64 accumulator and one exact count per
// lane, tree_sum, sum_waves_in_order, one row per workgroup, block_sum_rows in the finalize kernel).
// Roofline: HBM stream; useful bytes per pixel 16 (pred line) + 4 (D) + 12 (Nr) read, 12 + 4 + 12 written, 16 + 16 for
// the alpha read-modify-write.
#include <cmath>

#include "fixed_sum.hpp"
#include "internal.hpp"
#include "splat_math.hpp"
#include "splat_vjp.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = kSumThreads;
constexpr int kTile = (int)kTileWidth;            // 16: kThreads lanes, one pixel each
constexpr int kCellW = kTile + 4;                 // the tile plus a 2-pixel halo
constexpr int kCells = kCellW * kCellW;           // 400
constexpr int kCenW = kTile + 2;                  // the tile plus a 1-pixel halo
constexpr int kCentres = kCenW * kCenW;           // 324
constexpr uint32_t kMaxNormalRows = 1024;         // four workgroups per CU, as k_depth_loss
constexpr uint32_t kRowWords = 2;                 // {sum l, valid count}
static_assert(kTile * kTile == (int)kThreads, "one lane per pixel of a tile");

struct SplatNormalArgs {
    float vm[16];
};

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ int shortest_axis(const float *__restrict__ log_scales, uint32_t g) {
    const float l[3] = {log_scales[(size_t)g * 3], log_scales[(size_t)g * 3 + 1], log_scales[(size_t)g * 3 + 2]};
    int k = 0;
    if (l[1] < l[0]) k = 1;
    if (l[2] < (k ? l[1] : l[0])) k = 2;  // (selects, not l[k]: a dynamically indexed private array goes to LDS)
    return k;
}

// Column k of quat_to_rotmat(q) in camera space and the sign that turns it towards the camera.
__device__ __forceinline__ float camera_normal(const SplatNormalArgs &a, const float *__restrict__ means,
                                               const float q[4], int k, uint32_t g, float nc[3]) {
    const Mat3 R = quat_to_rotmat(q);
    float ax[3];
#pragma unroll
    for (int r = 0; r < 3; r++) ax[r] = k == 0 ? R.m[r][0] : (k == 1 ? R.m[r][1] : R.m[r][2]);
    const float m[3] = {means[(size_t)g * 3], means[(size_t)g * 3 + 1], means[(size_t)g * 3 + 2]};
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        nc[r] = (a.vm[r] * ax[0] + a.vm[4 + r] * ax[1]) + a.vm[8 + r] * ax[2];
        pc[r] = ((a.vm[r] * m[0] + a.vm[4 + r] * m[1]) + a.vm[8 + r] * m[2]) + a.vm[12 + r];
    }
    return dot3(nc, pc) > 0.0f ? -1.0f : 1.0f;
}

__global__ __launch_bounds__(kThreads) void k_splat_normals(const SplatNormalArgs a, const float *__restrict__ means,
                                                            const float *__restrict__ log_scales,
                                                            const float *__restrict__ quats, uint32_t n,
                                                            float *__restrict__ normals_out) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const float q[4] = {quats[(size_t)g * 4], quats[(size_t)g * 4 + 1], quats[(size_t)g * 4 + 2], quats[(size_t)g * 4 + 3]};
    float nc[3];
    const float s = camera_normal(a, means, q, shortest_axis(log_scales, g), g, nc);
#pragma unroll
    for (int r = 0; r < 3; r++) normals_out[(size_t)g * 3 + r] = s * nc[r];
}

__global__ __launch_bounds__(kThreads) void k_splat_normals_backward(const SplatNormalArgs a,
                                                                     const float *__restrict__ means,
                                                                     const float *__restrict__ log_scales,
                                                                     const float *__restrict__ quats, uint32_t n,
                                                                     const float *__restrict__ v_normals,
                                                                     float *__restrict__ v_quats) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const float q[4] = {quats[(size_t)g * 4], quats[(size_t)g * 4 + 1], quats[(size_t)g * 4 + 2], quats[(size_t)g * 4 + 3]};
    const int k = shortest_axis(log_scales, g);
    float nc[3];
    const float s = camera_normal(a, means, q, k, g, nc);
    const float v[3] = {v_normals[(size_t)g * 3], v_normals[(size_t)g * 3 + 1], v_normals[(size_t)g * 3 + 2]};
    Mat3 vR;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) vR.m[r][c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {  // v_a = s W^T v_n: row c of W^T is column c of W
        const float va = s * ((a.vm[4 * c] * v[0] + a.vm[4 * c + 1] * v[1]) + a.vm[4 * c + 2] * v[2]);
        vR.m[c][0] = k == 0 ? va : 0.0f;
        vR.m[c][1] = k == 1 ? va : 0.0f;
        vR.m[c][2] = k == 2 ? va : 0.0f;
    }
    float o[4];
    quat_to_rotmat_vjp(q, vR, o);
#pragma unroll
    for (int i = 0; i < 4; i++) v_quats[(size_t)g * 4 + i] += o[i];
}

struct NormalLossArgs {
    float kappa, alpha_min, fx, fy, cx, cy;
    int w, h;
    uint32_t tiles_x, num_tiles;
};

__device__ __forceinline__ float ray(int i, float c, float f) { return (((float)i + 0.5f) - c) / f; }

// GRAD = false: the normals-only form (normals_img == NULL): Nd and the valid count alone.
template <bool GRAD>
__global__ __launch_bounds__(kThreads) void k_normal_loss(const float *__restrict__ pred, const float *__restrict__ depth,
                                                          const float *__restrict__ normals_img, const NormalLossArgs a,
                                                          float *__restrict__ depth_normals_out,
                                                          float *__restrict__ v_depth, float *__restrict__ v_normals_img,
                                                          float *__restrict__ v_pred, double *__restrict__ rows) {
    __shared__ float s_z[kCells];
    __shared__ uint8_t s_counts[kCells];
    __shared__ float s_nd[3][kCentres];
    __shared__ float s_vtx[3][kCentres];
    __shared__ float s_vty[3][kCentres];
    __shared__ uint8_t s_valid[kCentres];
    __shared__ double red_sum[kSumWaves];
    __shared__ uint32_t red_cnt[kSumWaves];
    double acc = 0.0;
    uint32_t cnt = 0;
    const float neg_kappa = -a.kappa;
    for (uint32_t tile = blockIdx.x; tile < a.num_tiles; tile += gridDim.x) {  // the same trip count for every lane
        const int x0 = (int)(tile % a.tiles_x) * kTile, y0 = (int)(tile / a.tiles_x) * kTile;
        // 1. z and counts of the tile plus two pixels around it; off the frame nothing counts
        for (int i = (int)threadIdx.x; i < kCells; i += (int)kThreads) {
            const int x = x0 - 2 + i % kCellW, y = y0 - 2 + i / kCellW;
            float z = 0.0f;
            bool c = false;
            if (x >= 0 && x < a.w && y >= 0 && y < a.h) {
                const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
                const float A = pred[p * 4 + 3], D = depth[p];
                c = A >= a.alpha_min && D > 0.0f && A < INFINITY && D < INFINITY;
                if (c) z = D / A;
            }
            s_z[i] = z;
            s_counts[i] = c ? 1 : 0;
        }
        __syncthreads();
        // 2. Nd, v_tx, v_ty of the tile plus one pixel around it
        for (int i = (int)threadIdx.x; i < kCentres; i += (int)kThreads) {
            const int lx = i % kCenW, ly = i / kCenW;
            const int x = x0 - 1 + lx, y = y0 - 1 + ly;
            const int c = (ly + 1) * kCellW + (lx + 1);
            bool valid = x >= 1 && x <= a.w - 2 && y >= 1 && y <= a.h - 2 && s_counts[c] && s_counts[c - 1] &&
                         s_counts[c + 1] && s_counts[c - kCellW] && s_counts[c + kCellW];
            float nd[3] = {0.0f, 0.0f, 0.0f}, vtx[3] = {0.0f, 0.0f, 0.0f}, vty[3] = {0.0f, 0.0f, 0.0f};
            if (valid) {
                const float zl = s_z[c - 1], zr = s_z[c + 1], zu = s_z[c - kCellW], zd = s_z[c + kCellW];
                const float rxl = ray(x - 1, a.cx, a.fx), rxc = ray(x, a.cx, a.fx), rxr = ray(x + 1, a.cx, a.fx);
                const float ryu = ray(y - 1, a.cy, a.fy), ryc = ray(y, a.cy, a.fy), ryd = ray(y + 1, a.cy, a.fy);
                const float tx[3] = {zr * rxr - zl * rxl, zr * ryc - zl * ryc, zr - zl};
                const float ty[3] = {zd * rxc - zu * rxc, zd * ryd - zu * ryu, zd - zu};
                float cr[3];
                cross3(ty, tx, cr);
                const float m = dot3(cr, cr);
                valid = m > 0.0f && m < INFINITY;
                if (valid) {
                    const float len = sqrtf(m);
#pragma unroll
                    for (int k = 0; k < 3; k++) nd[k] = cr[k] / len;
                    if constexpr (GRAD) {
                        const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
                        float vnd[3], vc[3];
#pragma unroll
                        for (int k = 0; k < 3; k++) vnd[k] = neg_kappa * normals_img[p * 3 + k];
                        const float d = dot3(nd, vnd);
#pragma unroll
                        for (int k = 0; k < 3; k++) vc[k] = (vnd[k] - nd[k] * d) / len;
                        cross3(tx, vc, vty);
                        cross3(vc, ty, vtx);
                    }
                }
            }
            s_valid[i] = valid ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s_nd[k][i] = nd[k];
                if constexpr (GRAD) s_vtx[k][i] = vtx[k], s_vty[k][i] = vty[k];
            }
        }
        __syncthreads();
        // 3. the lane's own pixel: outputs, the gather of v_P, the loss term
        {
            const int lx = (int)threadIdx.x % kTile, ly = (int)threadIdx.x / kTile;
            const int x = x0 + lx, y = y0 + ly;
            if (x < a.w && y < a.h) {
                const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
                const int i = (ly + 1) * kCenW + (lx + 1);
                const bool valid = s_valid[i] != 0;
                const float nd[3] = {s_nd[0][i], s_nd[1][i], s_nd[2][i]};
                if (depth_normals_out) {
#pragma unroll
                    for (int k = 0; k < 3; k++) depth_normals_out[p * 3 + k] = nd[k];
                }
                if (valid) cnt += 1u;
                if constexpr (GRAD) {
                    const float A = pred[p * 4 + 3], D = depth[p];
                    if (valid) {
                        const float nr[3] = {normals_img[p * 3], normals_img[p * 3 + 1], normals_img[p * 3 + 2]};
                        const float l = A - dot3(nr, nd);
                        acc += (double)l;
                    }
                    if (v_normals_img) {
#pragma unroll
                        for (int k = 0; k < 3; k++) v_normals_img[p * 3 + k] = valid ? neg_kappa * nd[k] : 0.0f;
                    }
                    float vp[3];
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        vp[k] = ((s_vtx[k][i - 1] - s_vtx[k][i + 1]) + s_vty[k][i - kCenW]) - s_vty[k][i + kCenW];
                    const float vz = (vp[0] * ray(x, a.cx, a.fx) + vp[1] * ray(y, a.cy, a.fy)) + vp[2];
                    const bool counts = s_counts[(ly + 2) * kCellW + (lx + 2)] != 0;
                    if (v_depth) v_depth[p] = counts ? vz / A : 0.0f;
                    const bool touched = valid || s_valid[i - 1] || s_valid[i + 1] || s_valid[i - kCenW] || s_valid[i + kCenW];
                    if (v_pred && touched) v_pred[p * 4 + 3] += (valid ? a.kappa : 0.0f) - (vz * D) / (A * A);
                }
            }
        }
        __syncthreads();  // the next tile's staging overwrites what this one read
    }
    acc = tree_sum(acc);
    cnt = tree_sum(cnt);
    if (lane_id() == 0) red_sum[threadIdx.x / kWave] = acc, red_cnt[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        rows[(size_t)blockIdx.x * kRowWords + 0] = sum_waves_in_order(red_sum);
        rows[(size_t)blockIdx.x * kRowWords + 1] = (double)sum_waves_in_order(red_cnt);  // uint32 until here
    }
}

__global__ __launch_bounds__(kThreads) void k_normal_loss_finalize(const double *__restrict__ rows, uint32_t nrows,
                                                                   float kappa, uint32_t npix, float *__restrict__ stats,
                                                                   float *__restrict__ loss_accum) {
    block_sum_rows<kRowWords>(rows, nrows, [&](uint32_t word, double s) {
        if (word == 0) {
            const float loss = (float)((double)kappa * s);
            stats[0] = loss;
            if (loss_accum) *loss_accum += loss;
        } else {
            stats[1] = (float)(s / (double)npix);
        }
    });
}

uint32_t normal_loss_tiles(uint32_t w, uint32_t h) { return ceil_div(w, kTileWidth) * ceil_div(h, kTileWidth); }
uint32_t normal_loss_rows(uint32_t w, uint32_t h) { return min(normal_loss_tiles(w, h), kMaxNormalRows); }
size_t normal_loss_workspace_bytes(uint32_t w, uint32_t h) { return row_bytes(normal_loss_rows(w, h), kRowWords); }

SplatNormalArgs splat_normal_args(const BrushUniforms &u) {
    SplatNormalArgs a;
    for (int i = 0; i < 16; i++) a.vm[i] = u.viewmat[i];
    return a;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_splat_normals(const BrushUniforms *uniforms, const float *means, const float *log_scales,
                                   const float *quats, uint32_t n, float *normals_out, brush_stream_t stream) {
    if (!uniforms) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;
    if (!means || !log_scales || !quats || !normals_out) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(means, 4) || misaligned(log_scales, 4) || misaligned(quats, 4) || misaligned(normals_out, 4))
        return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_splat_normals, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       splat_normal_args(*uniforms), means, log_scales, quats, n, normals_out);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_splat_normals_backward(const BrushUniforms *uniforms, const float *means, const float *log_scales,
                                            const float *quats, uint32_t n, const float *v_normals, float *v_quats,
                                            brush_stream_t stream) {
    if (!uniforms) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;
    if (!means || !log_scales || !quats || !v_normals || !v_quats) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(means, 4) || misaligned(log_scales, 4) || misaligned(quats, 4) || misaligned(v_normals, 4) ||
        misaligned(v_quats, 4) || v_quats == quats)
        return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_splat_normals_backward, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), splat_normal_args(*uniforms), means, log_scales, quats, n,
                       v_normals, v_quats);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_normal_loss_workspace_size(uint32_t w, uint32_t h, size_t *bytes) {
    if (!bytes || !checked_pixels(w, h)) return BRUSH_ERR_INVALID_ARG;
    *bytes = normal_loss_workspace_bytes(w, h);
    return BRUSH_OK;
}

extern "C" int brush_normal_loss(const BrushUniforms *uniforms, const float *pred, const float *depth,
                                 const float *normals_img, const BrushNormalLoss *cfg, float *depth_normals_out,
                                 float *v_depth, float *v_normals_img, float *v_pred, float *stats, float *loss_accum,
                                 void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    if (!uniforms || !pred || !depth || !cfg || !stats || !workspace) return BRUSH_ERR_INVALID_ARG;
    const uint32_t w = uniforms->img_size[0], h = uniforms->img_size[1];
    const uint32_t npix = checked_pixels(w, h);
    if (!npix) return BRUSH_ERR_INVALID_ARG;
    if (!(cfg->alpha_min > 0.0f) || !(uniforms->focal[0] > 0.0f) || !(uniforms->focal[1] > 0.0f))
        return BRUSH_ERR_INVALID_ARG;
    // the normals-only form has no gradients to write
    if (!normals_img && (v_depth || v_normals_img || v_pred || loss_accum)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(pred, 16) || misaligned(depth, 4) || misaligned(normals_img, 4) || misaligned(depth_normals_out, 4) ||
        misaligned(v_depth, 4) || misaligned(v_normals_img, 4) || misaligned(v_pred, 16) || misaligned(stats, 4) ||
        misaligned(loss_accum, 4) || misaligned(workspace, 8))
        return BRUSH_ERR_INVALID_ARG;
    // every output is read by no lane: the inputs are read across tile seams while other workgroups write
    if (v_pred == pred || (v_depth && v_depth == depth) || (v_normals_img && v_normals_img == normals_img) ||
        (depth_normals_out && (depth_normals_out == normals_img || depth_normals_out == v_normals_img)))
        return BRUSH_ERR_INVALID_ARG;
    if (workspace_bytes < normal_loss_workspace_bytes(w, h)) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *rows = static_cast<double *>(workspace);
    const uint32_t nrows = normal_loss_rows(w, h);
    NormalLossArgs a;
    a.kappa = (float)((double)cfg->weight / (double)npix);
    a.alpha_min = cfg->alpha_min;
    a.fx = uniforms->focal[0], a.fy = uniforms->focal[1];
    a.cx = uniforms->pixel_center[0], a.cy = uniforms->pixel_center[1];
    a.w = (int)w, a.h = (int)h;
    a.tiles_x = ceil_div(w, kTileWidth), a.num_tiles = normal_loss_tiles(w, h);
    if (normals_img)
        hipLaunchKernelGGL(k_normal_loss<true>, dim3(nrows), dim3(kThreads), 0, s, pred, depth, normals_img, a,
                           depth_normals_out, v_depth, v_normals_img, v_pred, rows);
    else
        hipLaunchKernelGGL(k_normal_loss<false>, dim3(nrows), dim3(kThreads), 0, s, pred, depth, normals_img, a,
                           depth_normals_out, v_depth, v_normals_img, v_pred, rows);
    BRUSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_normal_loss_finalize, dim3(1), dim3(kThreads), 0, s, rows, nrows, a.kappa, npix, stats,
                       loss_accum);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
