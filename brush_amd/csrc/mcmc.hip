// mcmc.hip — the per-splat kernels of the MCMC densification strategy ("3D Gaussian Splatting as Markov Chain Monte
// Carlo", Kheradmand et al. 2024; gsplat's MCMCStrategy is the model): brush_mcmc_inject_noise (every step),
// brush_mcmc_reg_grads (every step, between the render backward and brush_adam_step) and brush_mcmc_relocation (once per
// refinement, on the gathered rows).  One lane per splat, plain vector loads and stores, no atomics, no workspace; the
// grid is a function of the count alone.  Built WITHOUT FMA contraction like the other per-splat stages.
// Roofline: HBM streams (noise: 44 B read + 24 B written per splat; regulariser: 16 B read, 16 B read-modify-written).
#include "internal.hpp"
#include "splat_math.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

// Philox4x32-10 (Salmon et al. 2011, Random123): counter c, key (k0, k1).
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        c[0] = hi1 ^ c[1] ^ k0, c[1] = lo1, c[2] = hi0 ^ c[3] ^ k1, c[3] = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// ln u of u = ((x >> 8) + 0.5) 2^-24.  With k = x >> 8 below 2^23 the uniform is an f32; above, it needs 25 bits, but
// then 1 - u = ((2^24 - 1 - k) + 0.5) 2^-24 is an f32, and ln u = log1p(-(1 - u)) keeps the draw's last bit.
__device__ __forceinline__ float log_uniform(uint32_t x) {
    const uint32_t k = x >> 8;
    if (k < (1u << 23)) return logf(((float)k + 0.5f) * 0x1p-24f);
    return log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
}
// 2 pi u of the same uniform, rounded to f32 once as (2k + 1) 2^-25 and once in the product.
__device__ __forceinline__ float angle_uniform(uint32_t x) {
    return 6.283185307179586f * ((float)(2u * (x >> 8) + 1u) * 0x1p-25f);
}

__global__ __launch_bounds__(256) void k_mcmc_inject_noise(float *__restrict__ means,
                                                           const float *__restrict__ log_scales,
                                                           const float4 *__restrict__ rotation,
                                                           const float *__restrict__ raw_opacity, uint32_t n,
                                                           float scale, uint32_t key0, uint32_t key1, uint32_t step,
                                                           float *__restrict__ xi_out) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    uint32_t c[4] = {g, step, 0x4D434D43u, 0u};
    philox4x32_10(c, key0, key1);
    const float r01 = sqrtf(-2.0f * log_uniform(c[0])), r2 = sqrtf(-2.0f * log_uniform(c[2]));
    float sn, cs;
    sincosf(angle_uniform(c[1]), &sn, &cs);
    const float xi[3] = {r01 * cs, r01 * sn, r2 * cosf(angle_uniform(c[3]))};
    if (xi_out) {
#pragma unroll
        for (int i = 0; i < 3; i++) xi_out[(size_t)g * 3 + i] = xi[i];
    }
    // gate = sigmoid(100 ((1 - o) - 0.995)) with 1 - o = sigmoid(-raw) formed without the cancellation of 1 - sigmoid
    const float one_minus_o = 1.0f / (1.0f + expf(raw_opacity[g]));
    const float gate = 1.0f / (1.0f + expf(-100.0f * (one_minus_o - 0.995f)));
    const float gs = gate * scale;
    const float4 q4 = rotation[g];
    float q[4] = {q4.x, q4.y, q4.z, q4.w};
    const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = q[i] * inv;
    const Mat3 R = quat_to_rotmat(q);
    // Sigma w = R (diag(exp(2 log_scale)) (R^T w)), w = xi gate scale
    float w[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = xi[i] * gs;
#pragma unroll
    for (int k = 0; k < 3; k++)
        t[k] = (R.m[0][k] * w[0] + R.m[1][k] * w[1] + R.m[2][k] * w[2]) * expf(2.0f * log_scales[(size_t)g * 3 + k]);
#pragma unroll
    for (int i = 0; i < 3; i++)
        means[(size_t)g * 3 + i] += R.m[i][0] * t[0] + R.m[i][1] * t[1] + R.m[i][2] * t[2];
}

// The regulariser terms are formed in float64 and added to the f32 gradient with one rounding.
__global__ __launch_bounds__(256) void k_mcmc_reg_grads(const float *__restrict__ raw_opacity,
                                                        const float *__restrict__ log_scales, uint32_t n, double c_opac,
                                                        double c_scale, float *__restrict__ v_opac,
                                                        float *__restrict__ v_scales) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    if (c_opac != 0.0) {
        const double s = 1.0 / (1.0 + exp(-(double)raw_opacity[g]));
        v_opac[g] = (float)((double)v_opac[g] + c_opac * (s * (1.0 - s)));
    }
    if (c_scale != 0.0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const size_t i = (size_t)g * 3 + k;
            v_scales[i] = (float)((double)v_scales[i] + c_scale * exp((double)log_scales[i]));
        }
    }
}

// Eq. 9 of the paper in float64.  With L = ln(1 - o) = -softplus(raw): o' = -expm1(L / N), and the double sum over
// (i, k) collapses over i (sum_{i=k+1..N} C(i-1, k) = C(N, k+1)) to D = sum_{j=1..N} C(N, j) (-1)^(j-1) o'^j / sqrt(j).
__global__ __launch_bounds__(256) void k_mcmc_relocation(const float *__restrict__ raw_in,
                                                         const float *__restrict__ log_scales_in,
                                                         const int32_t *__restrict__ ratio, uint32_t m,
                                                         double min_opacity, float *__restrict__ raw_out,
                                                         float *__restrict__ log_scales_out) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const int32_t rt = ratio[g];
    const int N = rt < 1 ? 1 : (rt > 51 ? 51 : rt);
    const double raw = (double)raw_in[g];
    const double o = 1.0 / (1.0 + exp(-raw));
    const double softplus = raw > 0.0 ? raw + log1p(exp(-raw)) : log1p(exp(raw));
    const double L = -softplus / (double)N;  // ln(1 - o')
    const double o_new = -expm1(L);
    double term = 1.0, D = 0.0;  // term = C(N, j) o'^j (-1)^(j-1) built by recurrence
    for (int j = 1; j <= N; j++) {
        term = term * ((double)(N - j + 1) / (double)j) * o_new;
        D += (j & 1 ? term : -term) / sqrt((double)j);
    }
    const double shift = log(o / D);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const size_t i = (size_t)g * 3 + k;
        log_scales_out[i] = (float)((double)log_scales_in[i] + shift);
    }
    const double hi = 1.0 - 0x1p-24;
    double logit;
    if (o_new < min_opacity) logit = log(min_opacity / (1.0 - min_opacity));
    else if (o_new > hi) logit = log(hi / 0x1p-24);
    else logit = log(o_new) - L;
    raw_out[g] = (float)logit;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_mcmc_inject_noise(float *means, const float *log_scales, const float *rotation,
                                       const float *raw_opacity, uint32_t n, float scale, size_t seed, uint32_t step,
                                       float *xi_out, brush_stream_t stream) {
    if (n == 0) return BRUSH_OK;
    if (!means || !log_scales || !rotation || !raw_opacity) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(means, 4) || misaligned(log_scales, 4) || misaligned(rotation, 16) || misaligned(raw_opacity, 4) ||
        misaligned(xi_out, 4))
        return BRUSH_ERR_INVALID_ARG;
    const uint64_t s64 = (uint64_t)seed;
    hipLaunchKernelGGL(k_mcmc_inject_noise, dim3(ceil_div(n, 256u)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       means, log_scales, reinterpret_cast<const float4 *>(rotation), raw_opacity, n, scale,
                       (uint32_t)(s64 & 0xFFFFFFFFull), (uint32_t)(s64 >> 32), step, xi_out);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_mcmc_reg_grads(const float *raw_opacity, const float *log_scales, uint32_t n, float opacity_reg,
                                    float scale_reg, float *v_opac, float *v_scales, brush_stream_t stream) {
    if (n == 0) return BRUSH_OK;
    if (!raw_opacity || !log_scales || !v_opac || !v_scales) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(raw_opacity, 4) || misaligned(log_scales, 4) || misaligned(v_opac, 4) || misaligned(v_scales, 4))
        return BRUSH_ERR_INVALID_ARG;
    if (opacity_reg == 0.0f && scale_reg == 0.0f) return BRUSH_OK;  // nothing to add: the arrays keep their bits
    hipLaunchKernelGGL(k_mcmc_reg_grads, dim3(ceil_div(n, 256u)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       raw_opacity, log_scales, n, (double)opacity_reg / (double)n,
                       (double)scale_reg / (3.0 * (double)n), v_opac, v_scales);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_mcmc_relocation(const float *raw_opacity_in, const float *log_scales_in, const int32_t *ratio,
                                     uint32_t m, float min_opacity, float *raw_opacity_out, float *log_scales_out,
                                     brush_stream_t stream) {
    if (m == 0) return BRUSH_OK;
    if (!raw_opacity_in || !log_scales_in || !ratio || !raw_opacity_out || !log_scales_out)
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(raw_opacity_in, 4) || misaligned(log_scales_in, 4) || misaligned(ratio, 4) ||
        misaligned(raw_opacity_out, 4) || misaligned(log_scales_out, 4) || !(min_opacity > 0.0f && min_opacity < 1.0f))
        return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_mcmc_relocation, dim3(ceil_div(m, 256u)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       raw_opacity_in, log_scales_in, ratio, m, (double)min_opacity, raw_opacity_out, log_scales_out);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
