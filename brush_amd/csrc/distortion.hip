// distortion.hip — the depth-distortion term of surface splatting (2DGS, GOF, RaDe-GS, gsplat's 2DGS path; the
// reference renders colour only) through the compositing walk, both ways.  Two kernels, both replays of a FINISHED
// brush_render_forward_depth's walk over the tile lists it left in the aux (replay_walk.hpp), and their launchers; the
// ABI entries are brush_render_distortion and brush_distortion_compact_grads here and brush_render_backward_distortion
// in render_bwd.hip.
//
// Definitions.  Per pixel p a "hit" is an entry the forward added: the walk of replay_walk.hpp exactly (the 0.999 clamp,
// the 1/255 test, the `next_T <= 1e-4` stop WITHOUT adding).  The hits i = 1..n in list order have
//   alpha_i  the forward's alpha,  T_i  the transmittance the entry meets,  w_i = alpha_i T_i,
//   z_i = compact_depth[cgid_i]   (what brush_render_forward_depth fills),
//   m_i = mu(z_i):  BRUSH_DISTORTION_DEPTH  mu(z) = z
//                   BRUSH_DISTORTION_NDC    mu(z) = A (1 - near / z), A = far / (far - near)   (2DGS's mapping)
//   L(p) = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2                                               (unordered pairs)
// L does not change under m -> m - const: both kernels work with c_i = m_i - m_first(p), m_first the m of the pixel's
// first hit, which keeps c^2 W - 2 c M1 + M2 away from catastrophic cancellation at large depths.  For the same reason
// the NDC mode never forms m ~ A itself: it carries the shifted m~ = -A near / z, whose differences are those of m with
// roundings at the size of A near / z instead of A.
//   running form   L = sum_i w_i (c_i^2 W_{i-1} - 2 c_i M1_{i-1} + M2_{i-1}),   W, M1, M2 the running sums of w, w c, w c^2
//   stats[p]       = (L, W, M1, M2), the pixel's totals; zeros where nothing was added
// Gradient for an upstream v(p) on L(p), per hit, from the pixel's TOTALS:
//   g_i = dL/dw_i = c_i^2 W - 2 c_i M1 + M2            dL/dm_i = 2 w_i (c_i W - M1)
//   sum_i w_i g_i = 2 L, hence dL/dalpha_i = T_i g_i - (2 L - P_i) / (1 - alpha_i), P_i = sum_{j<=i} w_j g_j
// k_distortion_grad_quad walks FRONT TO BACK with the running prefix P_i (no suffix, no second walk): the totals come
// from the stats of k_distortion_quad.  Where alpha_u = opac vis was clamped (alpha_u > 0.999) nothing flows through
// alpha (the derivative of the min); elsewhere v_alpha = v(p) dL/dalpha_i.  Per (record, quadrant), vva = vis v_alpha,
// the record's COMPACT row receives what rasterize_bwd.hip's flush defines for these words (dx = mean.x - pixel.x,
// gx = a dx + b dy, gy = b dx + c dy):
//   words 0, 1    += -opac sum vva gx, -opac sum vva gy
//   words 2, 3, 4 += -opac (1/2 sum vva dx^2, sum vva dx dy, 1/2 sum vva dy^2)
//   word 8        += sum vva
//   word 9        += mu'(z_i) sum v(p) dL/dm_i            (v_z; mu' = 1, or A near / z^2)
// Words 5-7 and 10-15 are not touched; the stopping entry contributes nothing; a non-finite v(p) stays inside the sums
// of its own records.
//
// gfx950 layout: the walk's.  A staged record is the plain ReplayRec (8 KiB of LDS per workgroup): six geometry words
// and two own words, (m, -) in the forward and (z, compact id) in the gradient kernel.  The forward has no atomics: every
// inside pixel is written by one lane, once, bitwise repeatable.  The gradient kernel loads its pixel's totals and v(p)
// once in front of the walk; per walked record with a hit anywhere in the wave eight partial sums (seven used) go through
// transpose_sum<8>, the per-record factors are applied by the lane that holds the sum, and lanes 0-6 issue one no-return
// global_atomic_add_f32 each on words of the record's one 64-byte row, non-zero sums only.  ORDER DEPENDENT in its last
// bits, as every float-atomic accumulation into the compact rows is.
#include "internal.hpp"
#include "replay_walk.hpp"
#include "transpose_sum.hpp"

namespace brush {
namespace {

// mu (up to the constant A in NDC mode, see the header) and mu'.  ndc is wave-uniform, an = A near.  Both kernels evaluate
// mu with this one expression (the division is correctly rounded), so a record has the same m in the forward and in the
// gradient.
__device__ __forceinline__ float mu_of(float z, uint32_t ndc, float an) { return ndc ? -an / z : z; }
__device__ __forceinline__ float dmu_of(float z, uint32_t ndc, float an) { return ndc ? an / (z * z) : 1.0f; }

// ---- k_distortion_quad --------------------------------------------------------------------------------------------------
// The record's first own word is m = mu(z), evaluated once by the lane that stages the record.  Every inside pixel writes
// stats[pix] = (L, W, M1, M2); n_splats == 0 reads no list at all.
__global__ __launch_bounds__(kRasterThreads) void k_distortion_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ compact_depth, uint32_t ndc, float an, float4 *__restrict__ stats) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    BRUSH_REPLAY_WALK_STATE;
    float L = 0.0f, W = 0.0f, M1 = 0.0f, M2 = 0.0f, m0 = 0.0f;
    bool first = true;
    BRUSH_REPLAY_WALK_BEGIN(n_splats != 0u, 7, rec[6] = mu_of(compact_depth[cgid], ndc, an), rec[6], 0.f)
    (void)gid;  // (the walk's second own word is not used here)
    const float fac = alpha * T;
    BRUSH_REPLAY_WALK_DIE(false)
    BRUSH_REPLAY_WALK_ADD(
        if (first) m0 = b.z;
        first = false;
        const float c = b.z - m0;
        // c (c W - 2 M1) + M2 over the sums in front of the entry, then the entry joins them
        const float g = fmaf(c, fmaf(c, W, -2.0f * M1), M2);
        const float wc = fac * c;
        L = fmaf(fac, g, L);
        W += fac;
        M1 += wc;
        M2 = fmaf(wc, c, M2))
    BRUSH_REPLAY_WALK_END
    if (inside) stats[(size_t)px + (size_t)py * w] = make_float4(L, W, M1, M2);
}

// ---- k_distortion_grad_quad ---------------------------------------------------------------------------------------------
// The record's own words are z and its compact id.  v_compact rows are ADDED into.
__global__ __launch_bounds__(kRasterThreads) void k_distortion_grad_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ compact_depth, uint32_t ndc, float an, const float4 *__restrict__ stats,
    const float *__restrict__ v_dist, float *__restrict__ v_compact) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
    float v = 0.0f;
    if (inside) {
        const size_t pix = (size_t)px + (size_t)py * w;
        tot = stats[pix];
        v = v_dist[pix];
    }
    const float L2 = 2.0f * tot.x, W = tot.y, M1 = tot.z, M2 = tot.w;
    BRUSH_REPLAY_WALK_STATE;
    float P = 0.0f, m0 = 0.0f;
    bool first = true;
    BRUSH_REPLAY_WALK_BEGIN(true, 8, (rec[6] = compact_depth[cgid], rec[7] = __uint_as_float(cgid)), rec[6], rec[7])
    (void)gid;  // (the rows are the compact ones)
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; k++) p[k] = 0.0f;
    if (hit) {  // (a pixel without a hit keeps zeros: 0 inf = NaN of another pixel's v stays out of this record's sums)
        const float m = mu_of(b.z, ndc, an);
        if (first) m0 = m;
        first = false;
        const float c = m - m0;
        const float fac = alpha * T;
        const float cwm = fmaf(c, W, -M1);           // c W - M1
        const float g = fmaf(c, cwm - M1, M2);       // c^2 W - 2 c M1 + M2
        P = fmaf(fac, g, P);
        // T g - (2 L - P) / (1 - alpha); 1 - alpha >= 0.001
        const float dalpha = fmaf(T, g, -(L2 - P) / (1.0f - alpha));
        const float vis = __builtin_amdgcn_exp2f(power);
        const float vva = alpha_u > 0.999f ? 0.0f : vis * (v * dalpha);
        const float gx = fmaf(a.z, dx, a.w * dy), gy = fmaf(a.w, dx, b.x * dy);
        const float wx = vva * dx, wy = vva * dy;
        p[0] = vva * gx;
        p[1] = vva * gy;
        p[2] = wx * dx;
        p[3] = wx * dy;
        p[4] = wy * dy;
        p[5] = vva;
        p[6] = v * ((2.0f * fac) * cwm);
    }
    BRUSH_REPLAY_WALK_DIE(false)
    BRUSH_REPLAY_WALK_ADD()
    if (ballot64(hit) != 0ull) {
        const float s = transpose_sum<8>(p, lane);
        // the per-record factors of the flush (rasterize_bwd.hip: reduce_stage), by the lane that holds the sum
        const float nopac = -opac;
        const float scale = lane == 6u ? dmu_of(b.z, ndc, an)
                          : lane == 5u ? 1.0f
                          : (lane == 2u || lane == 4u) ? 0.5f * nopac : nopac;
        const uint32_t word = lane < 5u ? lane : lane + 3u;  // sums 5, 6: words 8, 9
        const uint32_t cgid = __builtin_amdgcn_readfirstlane(__float_as_uint(b.w));  // < nvis <= n_splats: staged only then
        if (lane < 7u && s != 0.0f) unsafeAtomicAdd(v_compact + (size_t)cgid * kCompactStride + word, s * scale);
    }
    BRUSH_REPLAY_WALK_END
}

// The kernels' (ndc, an) of a configuration: an = A near = far / (far - near) near, once, in float32.
bool distortion_cfg(const BrushDistortion *cfg, uint32_t *ndc, float *an) {
    if (!cfg || cfg->mode > BRUSH_DISTORTION_NDC) return false;
    *ndc = cfg->mode == BRUSH_DISTORTION_NDC ? 1u : 0u;
    *an = 0.0f;
    if (*ndc) {
        // (NaNs fail these too)
        if (!(cfg->near_z > 0.0f) || !(cfg->far_z > cfg->near_z) || !(cfg->far_z <= 3.0e38f)) return false;
        *an = cfg->far_z / (cfg->far_z - cfg->near_z) * cfg->near_z;
    }
    return true;
}

}  // namespace

bool distortion_args_ok(const BrushAux *h_aux, const BrushDistortion *cfg, const float *stats, const float *v_distortion) {
    uint32_t ndc;
    float an;
    if (!h_aux || !stats || !v_distortion || !distortion_cfg(cfg, &ndc, &an)) return false;
    // deterministic mode keeps one row per intersection: there is no compact row to add into before the rows' sums
    if (h_aux->flags & BRUSH_AUX_DETERMINISTIC) return false;
    return !misaligned(stats, 16) && !misaligned(v_distortion, 4);
}

// The gradient launch of brush_distortion_compact_grads and brush_render_backward_distortion: validates what is the
// term's own (everything else is the caller's), then launches on `a`.
int launch_distortion_grad(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *compact_depth,
                           const BrushDistortion *cfg, const float *stats, const float *v_distortion, uint32_t n,
                           float *v_compact, brush_stream_t stream) {
    WalkArgs a;
    uint32_t ndc;
    float an;
    if (!compact_depth || !v_compact || !distortion_args_ok(h_aux, cfg, stats, v_distortion) ||
        !distortion_cfg(cfg, &ndc, &an) || !walk_args(h_uniforms, h_aux, n, stream, a))
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(compact_depth, 4) || misaligned(v_compact, 4)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    walk_launch(k_distortion_grad_quad, a, compact_depth, ndc, an, reinterpret_cast<const float4 *>(stats),
                v_distortion, v_compact);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

}  // namespace brush

using namespace brush;

extern "C" int brush_render_distortion(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                       const float *compact_depth, const BrushDistortion *cfg, uint32_t n, float *stats,
                                       brush_stream_t stream) {
    WalkArgs a;
    uint32_t ndc;
    float an;
    if (!compact_depth || !stats || !distortion_cfg(cfg, &ndc, &an) || !walk_args(h_uniforms, h_aux, n, stream, a))
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(compact_depth, 4) || misaligned(stats, 16)) return BRUSH_ERR_INVALID_ARG;
    // n == 0 launches too: every pixel is written on every call
    walk_launch(k_distortion_quad, a, compact_depth, ndc, an, reinterpret_cast<float4 *>(stats));
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_distortion_compact_grads(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                              const float *compact_depth, const BrushDistortion *cfg, const float *stats,
                                              const float *v_distortion, uint32_t n, float *v_compact,
                                              brush_stream_t stream) {
    return launch_distortion_grad(h_uniforms, h_aux, compact_depth, cfg, stats, v_distortion, n, v_compact, stream);
}
