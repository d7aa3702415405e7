// filter3d.hip — the 3D smoothing filter of Mip-Splatting (Yu et al. 2024, "Mip-Splatting: Alias-free 3D Gaussian
// Splatting"): brush_filter3d_rates (every TrainConfig.filter3d_every steps), brush_filter3d_apply (every step, in front
// of the render forward) and brush_filter3d_backward (every step, between the render backward and brush_adam_step).
// One lane per splat, plain vector loads and stores, no atomics, no workspace; the grids are functions of the count
// alone.  Built WITHOUT FMA contraction like the other per-splat stages.
// Roofline: HBM streams for the two per-step maps (apply: 20 B read + 16 B written per splat; transpose: 36 B read,
// 16 B of them written back); the rates are ALU-bound (n x views short iterations on LDS broadcast reads).
#include "detmath.hpp"
#include "internal.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kViewChunk = 64;  // view records staged in LDS at a time: 64 x 96 bytes = 6 KiB
constexpr uint32_t kViewWords = sizeof(BrushFilterView) / 4;
static_assert(sizeof(BrushFilterView) == 96 && kViewWords == 24, "the record is 24 words");
constexpr uint32_t kFillThreads = 1024;

// Pass 1: filter[g] = sd / max over valid views of fx / p.z, or 0 when no view sees the splat.  Every lane of a wave
// reads the same staged record (a broadcast read); max is a float comparison, so the view order does not matter.
__global__ __launch_bounds__(kThreads) void k_filter3d_rates(const float *__restrict__ means, uint32_t n,
                                                             const BrushFilterView *__restrict__ views,
                                                             uint32_t num_views, float near_z, float margin, float sd,
                                                             float *__restrict__ filter) {
    __shared__ BrushFilterView s_views[kViewChunk];
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    const bool live = g < n;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) x = means[(size_t)g * 3], y = means[(size_t)g * 3 + 1], z = means[(size_t)g * 3 + 2];
    float rate = 0.0f;
    for (uint32_t base = 0; base < num_views; base += kViewChunk) {
        const uint32_t cnt = min(kViewChunk, num_views - base);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(views + base);
        uint32_t *dst = reinterpret_cast<uint32_t *>(s_views);
        __syncthreads();  // the previous chunk has been read by every wave
        for (uint32_t i = threadIdx.x; i < cnt * kViewWords; i += kThreads) dst[i] = src[i];
        __syncthreads();
        if (!live) continue;
        for (uint32_t v = 0; v < cnt; v++) {
            const BrushFilterView &r = s_views[v];
            const float *m = r.viewmat;  // column-major: element (row, col) at [col * 4 + row]
            const float pz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
            if (!(pz > near_z)) continue;
            const float px = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
            const float py = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
            const float w = (float)r.width, h = (float)r.height;
            const float u = (r.fx * px) / pz + r.cx, t = (r.fy * py) / pz + r.cy;
            const float hi = 1.0f + margin;
            if (u >= -margin * w && u <= hi * w && t >= -margin * h && t <= hi * h) rate = fmaxf(rate, r.fx / pz);
        }
    }
    if (live) filter[g] = rate > 0.0f ? sd / rate : 0.0f;
}

// Pass 2, one workgroup: the largest filter length of the seen splats, then every unseen splat (0 from pass 1) takes it.
// A 16-byte aligned array goes through float4 accesses, four per lane and trip, to keep enough bytes in flight for one
// compute unit; the rest (a misaligned array, the tail) goes word by word.  max is exact: the order does not matter.
__global__ __launch_bounds__(kFillThreads) void k_filter3d_fill_unseen(float *__restrict__ filter, uint32_t n) {
    __shared__ float s_max[kFillThreads / 64];
    const uint32_t n4 = misaligned(filter, 16) ? 0u : n / 4u;  // float4 groups
    float4 *f4 = reinterpret_cast<float4 *>(filter);
    float top = 0.0f;
    for (uint32_t base = 0; base < n4; base += 4 * kFillThreads) {
        float4 v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t i = base + k * kFillThreads + threadIdx.x;
            v[k] = i < n4 ? f4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) top = fmaxf(top, fmaxf(fmaxf(v[k].x, v[k].y), fmaxf(v[k].z, v[k].w)));
    }
    for (uint32_t i = n4 * 4 + threadIdx.x; i < n; i += kFillThreads) top = fmaxf(top, filter[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = top;
    __syncthreads();
    top = s_max[0];
#pragma unroll
    for (uint32_t k = 1; k < kFillThreads / 64; k++) top = fmaxf(top, s_max[k]);
    if (top == 0.0f) return;  // nothing is seen: every length stays 0
    for (uint32_t base = 0; base < n4; base += 4 * kFillThreads) {
        float4 v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t i = base + k * kFillThreads + threadIdx.x;
            v[k] = i < n4 ? f4[i] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t i = base + k * kFillThreads + threadIdx.x;
            if (v[k].x == 0.0f || v[k].y == 0.0f || v[k].z == 0.0f || v[k].w == 0.0f)  // (never for i >= n4)
                f4[i] = make_float4(v[k].x == 0.0f ? top : v[k].x, v[k].y == 0.0f ? top : v[k].y,
                                    v[k].z == 0.0f ? top : v[k].z, v[k].w == 0.0f ? top : v[k].w);
        }
    }
    for (uint32_t i = n4 * 4 + threadIdx.x; i < n; i += kFillThreads)
        if (filter[i] == 0.0f) filter[i] = top;
}

// What the forward map and its transpose both need of one splat, from one definition so that both see the same bits.
// With s2_k = exp(2 l_k), f2 = f f and sum_k = s2_k + f2:
//   q_k = s2_k / sum_k  (d l'_k / d l_k),   g_k = f2 / sum_k  (d ln c / d l_k),   c = prod_k sqrt(q_k),
//   E = exp(-o) with o read clamped to [-87, 87],   D = (1 - c) + E,
// so that p = sigmoid(o) c = c / (1 + E), 1 - p = D / (1 + E) and logit(p) = ln c - ln D.
struct Filter3dTerms {
    float sum[3], q[3], g[3];
    float c, E, D;
};

__device__ __forceinline__ Filter3dTerms filter3d_terms(const float l[3], float o, float f2) {
    Filter3dTerms t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s2 = det_expf(2.0f * l[k]);
        t.sum[k] = s2 + f2;
        t.q[k] = s2 / t.sum[k];
        t.g[k] = f2 / t.sum[k];
    }
    t.c = (sqrtf(t.q[0]) * sqrtf(t.q[1])) * sqrtf(t.q[2]);
    t.E = det_expf(fminf(fmaxf(-o, -87.0f), 87.0f));
    t.D = (1.0f - t.c) + t.E;
    return t;
}

__global__ __launch_bounds__(kThreads) void k_filter3d_apply(const float *__restrict__ log_scales,
                                                             const float *__restrict__ raw_opacity,
                                                             const float *__restrict__ filter, uint32_t n,
                                                             float *__restrict__ log_scales_out,
                                                             float *__restrict__ raw_opacity_out) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const float f = filter[g], f2 = f * f;
    const float l[3] = {log_scales[(size_t)g * 3], log_scales[(size_t)g * 3 + 1], log_scales[(size_t)g * 3 + 2]};
    const float o = raw_opacity[g];
    if (f2 == 0.0f) {  // no filter: the row goes through bit for bit
#pragma unroll
        for (int k = 0; k < 3; k++) log_scales_out[(size_t)g * 3 + k] = l[k];
        raw_opacity_out[g] = o;
        return;
    }
    const Filter3dTerms t = filter3d_terms(l, o, f2);
#pragma unroll
    for (int k = 0; k < 3; k++) log_scales_out[(size_t)g * 3 + k] = 0.5f * det_logf(t.sum[k]);
    // c == 0 (underflow) gives -inf here: the floor is BRUSH_FILTER3D_MIN_RAW_OPACITY, ln of the smallest normal f32
    raw_opacity_out[g] = fmaxf(det_logf(t.c) - det_logf(t.D), BRUSH_FILTER3D_MIN_RAW_OPACITY);
}

__global__ __launch_bounds__(kThreads) void k_filter3d_backward(const float *__restrict__ log_scales,
                                                                const float *__restrict__ raw_opacity,
                                                                const float *__restrict__ filter, uint32_t n,
                                                                float *__restrict__ v_scales,
                                                                float *__restrict__ v_opac) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const float f = filter[g], f2 = f * f;
    if (f2 == 0.0f) return;  // the identity's transpose: the gradients keep their bits
    const float l[3] = {log_scales[(size_t)g * 3], log_scales[(size_t)g * 3 + 1], log_scales[(size_t)g * 3 + 2]};
    const Filter3dTerms t = filter3d_terms(l, raw_opacity[g], f2);
    const float vo = v_opac[g];
    const float inv_one_minus_p = (1.0f + t.E) / t.D;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const size_t i = (size_t)g * 3 + k;
        v_scales[i] = v_scales[i] * t.q[k] + vo * (t.g[k] * inv_one_minus_p);
    }
    v_opac[g] = vo * (t.E / t.D);
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" uint32_t brush_filter3d_view_chunk(void) { return kViewChunk; }

extern "C" int brush_filter3d_rates(const float *means, uint32_t n, const BrushFilterView *views, uint32_t num_views,
                                    float near_z, float margin, float variance, float *filter,
                                    brush_stream_t stream) {
    if (n == 0) return BRUSH_OK;
    if (!means || !filter || (num_views != 0 && !views)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(means, 4) || misaligned(filter, 4) || misaligned(views, 16)) return BRUSH_ERR_INVALID_ARG;
    if (!(near_z >= 0.0f) || !(margin >= 0.0f) || !(variance >= 0.0f) || variance == __builtin_inff())
        return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float sd = (float)__builtin_sqrt((double)variance);
    hipLaunchKernelGGL(k_filter3d_rates, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, means, n, views, num_views,
                       near_z, margin, sd, filter);
    BRUSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_filter3d_fill_unseen, dim3(1), dim3(kFillThreads), 0, s, filter, n);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_filter3d_apply(const float *log_scales, const float *raw_opacity, const float *filter, uint32_t n,
                                    float *log_scales_out, float *raw_opacity_out, brush_stream_t stream) {
    if (n == 0) return BRUSH_OK;
    if (!log_scales || !raw_opacity || !filter || !log_scales_out || !raw_opacity_out) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(log_scales, 4) || misaligned(raw_opacity, 4) || misaligned(filter, 4) ||
        misaligned(log_scales_out, 4) || misaligned(raw_opacity_out, 4))
        return BRUSH_ERR_INVALID_ARG;
    if (log_scales_out == log_scales || raw_opacity_out == raw_opacity) return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_filter3d_apply, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), log_scales, raw_opacity, filter, n, log_scales_out,
                       raw_opacity_out);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_filter3d_backward(const float *log_scales, const float *raw_opacity, const float *filter,
                                       uint32_t n, float *v_scales, float *v_opac, brush_stream_t stream) {
    if (n == 0) return BRUSH_OK;
    if (!log_scales || !raw_opacity || !filter || !v_scales || !v_opac) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(log_scales, 4) || misaligned(raw_opacity, 4) || misaligned(filter, 4) || misaligned(v_scales, 4) ||
        misaligned(v_opac, 4))
        return BRUSH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_filter3d_backward, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), log_scales, raw_opacity, filter, n, v_scales, v_opac);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
