// splat_pack.hip — the chunk-quantised ("compressed PLY") form of a splat cloud, packed and unpacked on the device:
// brush_splat_pack_keys (bounds of the means, Morton keys and identity values for brush_radix_argsort_u32, the
// non-finite flag), brush_splat_pack (one workgroup per chunk of 256 sorted rows) and brush_splat_unpack (back to the
// five float tensors of Splats).  DESIGN.md §8 row 25 and include/brush_hip.h state the format; every packed word is
// defined operation by operation in float32, so this file is built WITHOUT FMA contraction like the other per-splat
// stages, divisions and square roots are the correctly rounded ones, and tests/compress_ref.py restates it bit for bit.
// No atomics anywhere: the bounds go through per-workgroup partials and one finishing workgroup (min / max do not
// depend on the order, so the bits are those of any order), and every output word has one writer.
// Roofline: HBM streams.  Keys: 236 B read per splat at SH degree 3 (the non-finite check reads every parameter) and
// 8 B written.  Pack: a gather of 12- to 192-byte rows through the permutation, 236 B read and 61 B written per splat.
// Unpack: 61 B read, 236 B written.
#include "detmath.hpp"
#include "internal.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;       // one chunk: BRUSH_SPLAT_CHUNK rows
constexpr uint32_t kWaves = kThreads / kWave;
constexpr uint32_t kMaxPartials = 1024;  // workgroups of the bounds pass
constexpr uint32_t kPartialWords = 8;    // lo[3] hi[3] flag pad
constexpr float kShC0 = 0.28209479177387814f;
static_assert(kThreads == BRUSH_SPLAT_CHUNK, "a workgroup packs one chunk");

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Non-finite words among a[0..count), read by the whole grid in a coalesced stride.
__device__ __forceinline__ uint32_t scan_nonfinite(const float *__restrict__ a, size_t count) {
    uint32_t bad = 0;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += stride) bad |= nonfinite(a[i]) ? 1u : 0u;
    return bad;
}

// Pass 1: per-workgroup bounds of the means (canonical zero: v + 0.0f) and the OR of "this word is not finite" over
// every parameter, one row of kPartialWords per workgroup.
__global__ __launch_bounds__(kThreads) void k_pack_bounds(const float *__restrict__ means,
                                                          const float *__restrict__ log_scales,
                                                          const float *__restrict__ rotation,
                                                          const float *__restrict__ raw_opacity,
                                                          const float *__restrict__ sh, uint32_t n, uint32_t sh_row,
                                                          float *__restrict__ partials) {
    __shared__ float s_red[kWaves][kPartialWords];
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    uint32_t bad = 0;
    const uint32_t stride = gridDim.x * kThreads;
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < n; g += stride) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = means[(size_t)g * 3 + k] + 0.0f;
            bad |= nonfinite(v) ? 1u : 0u;
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    }
    bad |= scan_nonfinite(log_scales, (size_t)n * 3);
    bad |= scan_nonfinite(rotation, (size_t)n * 4);
    bad |= scan_nonfinite(raw_opacity, (size_t)n);
    bad |= scan_nonfinite(sh, (size_t)n * sh_row);
    const uint32_t wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = wave_minf(lo[k]);
        hi[k] = wave_maxf(hi[k]);
    }
    const bool any_bad = __ballot(bad != 0u) != 0ull;
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) s_red[wave][k] = lo[k], s_red[wave][3 + k] = hi[k];
        s_red[wave][6] = any_bad ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const uint32_t k = threadIdx.x;
        float v = s_red[0][k];
#pragma unroll
        for (uint32_t w = 1; w < kWaves; w++) v = k < 3 ? fminf(v, s_red[w][k]) : fmaxf(v, s_red[w][k]);
        partials[(size_t)blockIdx.x * kPartialWords + k] = v;
    }
}

// Pass 2, one workgroup: the partial rows into bounds[0..6) (lo xyz, hi xyz), state[0] = n (the sort's device count)
// and state[1] = the non-finite flag.
__global__ __launch_bounds__(kThreads) void k_pack_bounds_finish(const float *__restrict__ partials, uint32_t rows,
                                                                 uint32_t n, float *__restrict__ bounds,
                                                                 uint32_t *__restrict__ state) {
    __shared__ float s_red[kWaves][kPartialWords];
    const float inf = __builtin_inff();
    float v[7] = {inf, inf, inf, -inf, -inf, -inf, 0.0f};
    for (uint32_t r = threadIdx.x; r < rows; r += kThreads) {
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const float p = partials[(size_t)r * kPartialWords + k];
            v[k] = k < 3 ? fminf(v[k], p) : fmaxf(v[k], p);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) v[k] = k < 3 ? wave_minf(v[k]) : wave_maxf(v[k]);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 7; k++) s_red[threadIdx.x / kWave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const uint32_t k = threadIdx.x;
        float r = s_red[0][k];
#pragma unroll
        for (uint32_t w = 1; w < kWaves; w++) r = k < 3 ? fminf(r, s_red[w][k]) : fmaxf(r, s_red[w][k]);
        if (k < 6) bounds[k] = r;
        else state[1] = r != 0.0f ? 1u : 0u;
    }
    if (threadIdx.x == 7) state[0] = n;
}

// 10 bits -> every third bit (the usual magic-number spread).
__device__ __forceinline__ uint32_t spread10(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__device__ __forceinline__ uint32_t morton_axis(float x, float lo, float hi) {
    if (hi == lo) return 0u;
    const float t = ((x - lo) / (hi - lo)) * 1024.0f;
    if (!(t >= 0.0f)) return 0u;  // a NaN mean (the flag is already up); never negative for a finite one
    return t >= 1023.0f ? 1023u : (uint32_t)t;
}

// Pass 3: one lane per splat.
__global__ __launch_bounds__(kThreads) void k_pack_keys(const float *__restrict__ means, uint32_t n,
                                                        const float *__restrict__ bounds, uint32_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = morton_axis(means[(size_t)g * 3 + k] + 0.0f, bounds[k], bounds[3 + k]);
    keys[g] = (spread10(q[2]) << 2) | (spread10(q[1]) << 1) | spread10(q[0]);
    vals[g] = g;
}

// ---- the words ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float norm01(float v, float lo, float hi) {
    if (v <= lo) return 0.0f;
    if (v >= hi) return 1.0f;
    if (hi - lo < 1e-5f) return 0.0f;
    return (v - lo) / (hi - lo);
}

template <uint32_t BITS>
__device__ __forceinline__ uint32_t unorm(float t) {
    constexpr float top = (float)((1u << BITS) - 1u);
    const float r = floorf(t * top + 0.5f);
    if (!(r > 0.0f)) return 0u;  // negative, zero or NaN
    return r >= top ? (1u << BITS) - 1u : (uint32_t)r;
}

__device__ __forceinline__ uint32_t pack_11_10_11(const float v[3], const float *lo, const float *hi) {
    return (unorm<11>(norm01(v[0], lo[0], hi[0])) << 21) | (unorm<10>(norm01(v[1], lo[1], hi[1])) << 11) |
           unorm<11>(norm01(v[2], lo[2], hi[2]));
}

__device__ __forceinline__ uint32_t pack_rotation(float4 r) {
    float a[4] = {r.x + 0.0f, r.y + 0.0f, r.z + 0.0f, r.w + 0.0f};
    const float len = sqrtf(((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + a[3] * a[3]);
    if (!(len > 0.0f) || nonfinite(len)) {
        a[0] = 1.0f, a[1] = 0.0f, a[2] = 0.0f, a[3] = 0.0f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) a[i] = a[i] / len;
    }
    uint32_t big = 0;
    float best = fabsf(a[0]);
#pragma unroll
    for (uint32_t i = 1; i < 4; i++) {
        const float m = fabsf(a[i]);
        if (m > best) best = m, big = i;
    }
    float top = a[0];
#pragma unroll
    for (uint32_t i = 1; i < 4; i++) top = big == i ? a[i] : top;
    const bool flip = top < 0.0f;
    uint32_t word = big;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        if (i == big) continue;
        const float v = flip ? -a[i] : a[i];
        word = (word << 10) | unorm<10>(v * 0.70710678f + 0.5f);
    }
    return word;
}

__device__ __forceinline__ uint32_t sh_byte(float v) {
    const float r = floorf((v / 8.0f + 0.5f) * 256.0f);
    if (!(r > 0.0f)) return 0u;
    return r >= 255.0f ? 255u : (uint32_t)r;
}

// One input row of CIN * 3 floats: whole 16-byte loads where the row length keeps every row aligned (degrees 1 and 3).
template <uint32_t CIN>
__device__ __forceinline__ void load_sh_row(const float *__restrict__ sh, uint32_t g, float *row) {
    constexpr uint32_t kRow = CIN * 3;
    const float *src = sh + (size_t)g * kRow;
    if constexpr (kRow % 4 == 0) {
        const float4 *src4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
        for (uint32_t i = 0; i < kRow / 4; i++) {
            const float4 v = src4[i];
            row[4 * i] = v.x, row[4 * i + 1] = v.y, row[4 * i + 2] = v.z, row[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kRow; i++) row[i] = src[i];
    }
}

// One workgroup per chunk, one lane per row of the sorted order.  CIN: coefficients per channel of the input
// ((degree + 1)^2), K: higher-order coefficients per channel of the output (0, 3, 8, 15; K + 1 <= CIN).
template <uint32_t CIN, uint32_t K>
__global__ __launch_bounds__(kThreads) void k_splat_pack(const float *__restrict__ means,
                                                         const float *__restrict__ log_scales,
                                                         const float *__restrict__ rotation,
                                                         const float *__restrict__ raw_opacity,
                                                         const float *__restrict__ sh, uint32_t n,
                                                         const uint32_t *__restrict__ order,
                                                         float *__restrict__ chunks, uint4 *__restrict__ words,
                                                         uint32_t *__restrict__ sh_out) {
    constexpr uint32_t kBytes = 3 * K;                      // SH bytes per row
    constexpr uint32_t kChunkDwords = kThreads * kBytes / 4;  // 256 * 3K is a multiple of 4
    __shared__ float s_red[kWaves][18];
    __shared__ uint32_t s_sh[kChunkDwords > 0 ? kChunkDwords : 1];

    const uint32_t row = blockIdx.x * kThreads + threadIdx.x;
    const bool live = row < n;
    const float inf = __builtin_inff();
    float q[9];  // position, clamped log-scale, colour
    float4 rot = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    float opac = 0.0f;
    float coeffs[CIN * 3];
    if (live) {
        const uint32_t g = order[row];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            q[k] = means[(size_t)g * 3 + k] + 0.0f;
            q[3 + k] = fminf(fmaxf(log_scales[(size_t)g * 3 + k] + 0.0f, -20.0f), 20.0f);
        }
        rot = reinterpret_cast<const float4 *>(rotation)[g];
        opac = raw_opacity[g] + 0.0f;
        load_sh_row<CIN>(sh, g, coeffs);
#pragma unroll
        for (int k = 0; k < 3; k++) q[6 + k] = (coeffs[k] + 0.0f) * kShC0 + 0.5f;
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < CIN * 3; k++) coeffs[k] = 0.0f;
    }

    // chunk min / max of the nine quantities over the live rows: shuffles in the wave, LDS across the four waves
    float lo[9], hi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        lo[k] = wave_minf(live ? q[k] : inf);
        hi[k] = wave_maxf(live ? q[k] : -inf);
    }
    const uint32_t wave = threadIdx.x / kWave;
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) s_red[wave][k] = lo[k], s_red[wave][9 + k] = hi[k];
    }

    // the SH bytes of this row into the chunk's staging area, channel-major: byte c K + (k - 1)
    if constexpr (K > 0) {
        uint8_t *stage = reinterpret_cast<uint8_t *>(s_sh) + threadIdx.x * kBytes;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++)
#pragma unroll
            for (uint32_t k = 1; k <= K; k++)
                stage[c * K + (k - 1)] = live ? (uint8_t)sh_byte(coeffs[k * 3 + c] + 0.0f) : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) {
        lo[k] = s_red[0][k], hi[k] = s_red[0][9 + k];
#pragma unroll
        for (uint32_t w = 1; w < kWaves; w++) lo[k] = fminf(lo[k], s_red[w][k]), hi[k] = fmaxf(hi[k], s_red[w][9 + k]);
    }
    if (threadIdx.x == 0) {
        // min_x min_y min_z max_x max_y max_z | the same of the scales | the same of the colours
        float *out = chunks + (size_t)blockIdx.x * 18;
#pragma unroll
        for (int grp = 0; grp < 3; grp++)
#pragma unroll
            for (int k = 0; k < 3; k++) out[grp * 6 + k] = lo[grp * 3 + k], out[grp * 6 + 3 + k] = hi[grp * 3 + k];
    }

    uint4 w4 = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        w4.x = pack_11_10_11(q, lo, hi);
        w4.y = pack_rotation(rot);
        w4.z = pack_11_10_11(q + 3, lo + 3, hi + 3);
        w4.w = (unorm<8>(norm01(q[6], lo[6], hi[6])) << 24) | (unorm<8>(norm01(q[7], lo[7], hi[7])) << 16) |
               (unorm<8>(norm01(q[8], lo[8], hi[8])) << 8) | unorm<8>(det_sigmoid(opac));
    }
    words[row] = w4;  // the arrays hold 256 C rows: rows past n are written as zeros

    if constexpr (K > 0) {
        uint32_t *dst = sh_out + (size_t)blockIdx.x * kChunkDwords;
        for (uint32_t i = threadIdx.x; i < kChunkDwords; i += kThreads) dst[i] = s_sh[i];
    }
}

// ---- unpack ---------------------------------------------------------------------------------------------------------
template <uint32_t BITS>
__device__ __forceinline__ float lerp_code(uint32_t code, float lo, float hi) {
    const float t = (float)code / (float)((1u << BITS) - 1u);
    return lo * (1.0f - t) + hi * t;
}

// One workgroup per chunk, one lane per row; K as above.  The chunk's SH bytes come in as whole dwords through LDS.
template <uint32_t K>
__global__ __launch_bounds__(kThreads) void k_splat_unpack(const float *__restrict__ chunks,
                                                           const uint4 *__restrict__ words,
                                                           const uint8_t *__restrict__ sh_in, uint32_t n,
                                                           float *__restrict__ means, float *__restrict__ log_scales,
                                                           float *__restrict__ rotation,
                                                           float *__restrict__ raw_opacity, float *__restrict__ sh) {
    constexpr uint32_t kBytes = 3 * K;
    constexpr uint32_t kChunkDwords = kThreads * kBytes / 4;
    constexpr uint32_t kRow = (K + 1) * 3;
    __shared__ uint32_t s_sh[kChunkDwords > 0 ? kChunkDwords : 1];
    const uint32_t row = blockIdx.x * kThreads + threadIdx.x;
    if constexpr (K > 0) {
        // the input holds n rows exactly: whole dwords while they end inside it, the last one to three bytes singly
        const size_t total = (size_t)n * kBytes, base = (size_t)blockIdx.x * kThreads * kBytes;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(sh_in + base);
        for (uint32_t i = threadIdx.x; i < kChunkDwords; i += kThreads) {
            const size_t at = base + (size_t)i * 4;
            uint32_t v = 0;
            if (at + 4 <= total) {
                v = src[i];
            } else {
                for (uint32_t b = 0; b < 4; b++)
                    if (at + b < total) v |= (uint32_t)sh_in[at + b] << (8 * b);
            }
            s_sh[i] = v;
        }
        __syncthreads();
    }
    if (row >= n) return;
    const float *ch = chunks + (size_t)blockIdx.x * 18;  // row >> 8
    const uint4 w4 = words[row];
    means[(size_t)row * 3] = lerp_code<11>(w4.x >> 21, ch[0], ch[3]);
    means[(size_t)row * 3 + 1] = lerp_code<10>((w4.x >> 11) & 0x3ffu, ch[1], ch[4]);
    means[(size_t)row * 3 + 2] = lerp_code<11>(w4.x & 0x7ffu, ch[2], ch[5]);
    log_scales[(size_t)row * 3] = lerp_code<11>(w4.z >> 21, ch[6], ch[9]);
    log_scales[(size_t)row * 3 + 1] = lerp_code<10>((w4.z >> 11) & 0x3ffu, ch[7], ch[10]);
    log_scales[(size_t)row * 3 + 2] = lerp_code<11>(w4.z & 0x7ffu, ch[8], ch[11]);

    float rest[3];
    float sumsq = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t code = (w4.y >> (10 * (2 - i))) & 0x3ffu;
        rest[i] = ((float)code / 1023.0f - 0.5f) * 1.41421356f;
        sumsq = i == 0 ? rest[0] * rest[0] : sumsq + rest[i] * rest[i];
    }
    const float top = sqrtf(fmaxf(0.0f, 1.0f - sumsq));
    const uint32_t big = w4.y >> 30;
    float a[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        // the three stored components are those of the indices other than `big`, in rising order
        const uint32_t j = i < big ? i : i - 1;
        a[i] = i == big ? top : (j == 0 ? rest[0] : (j == 1 ? rest[1] : rest[2]));
    }
    reinterpret_cast<float4 *>(rotation)[row] = make_float4(a[0], a[1], a[2], a[3]);

    const float alpha = fminf(fmaxf((float)(w4.w & 0xffu), 0.5f), 254.5f) / 255.0f;
    raw_opacity[row] = det_logf(alpha / (1.0f - alpha));

    float out[kRow];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t code = (w4.w >> (24 - 8 * c)) & 0xffu;
        out[c] = (lerp_code<8>(code, ch[12 + c], ch[15 + c]) - 0.5f) / kShC0;
    }
    if constexpr (K > 0) {
        const uint8_t *stage = reinterpret_cast<const uint8_t *>(s_sh) + threadIdx.x * kBytes;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++)
#pragma unroll
            for (uint32_t k = 1; k <= K; k++)
                out[k * 3 + c] = (((float)stage[c * K + (k - 1)] + 0.5f) / 256.0f - 0.5f) * 8.0f;
    }
    float *dst = sh + (size_t)row * kRow;
    if constexpr (kRow % 4 == 0) {
#pragma unroll
        for (uint32_t i = 0; i < kRow / 4; i++)
            reinterpret_cast<float4 *>(dst)[i] = make_float4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kRow; i++) dst[i] = out[i];
    }
}

uint32_t bounds_rows(uint32_t n) { return min(ceil_div(n, kThreads), kMaxPartials); }

struct PackWs {
    float *partials;  // [bounds_rows][kPartialWords]
    float *bounds;    // [8]
    size_t bytes;
};
PackWs carve_pack(void *ws, uint32_t n) {
    Carver c(ws);
    PackWs p;
    p.partials = c.take<float>((size_t)bounds_rows(n) * kPartialWords);
    p.bounds = c.take<float>(8);
    p.bytes = c.bytes();
    return p;
}

// coefficients per channel of a degree, or 0 for a degree the format does not have
uint32_t coeffs_of_degree(uint32_t degree) { return degree <= 3 ? (degree + 1) * (degree + 1) : 0u; }

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_splat_pack_workspace_size(uint32_t n, size_t *bytes) {
    if (!bytes || n == 0 || n > BRUSH_SPLAT_PACK_MAX) return BRUSH_ERR_INVALID_ARG;
    *bytes = carve_pack(nullptr, n).bytes;
    return BRUSH_OK;
}

extern "C" int brush_splat_pack_keys(const float *means, const float *log_scales, const float *rotation,
                                     const float *raw_opacity, const float *sh_coeffs, uint32_t n, uint32_t sh_degree,
                                     uint32_t *keys, uint32_t *vals, uint32_t *state, void *workspace,
                                     size_t workspace_bytes, brush_stream_t stream) {
    const uint32_t cin = coeffs_of_degree(sh_degree);
    if (n == 0 || n > BRUSH_SPLAT_PACK_MAX || cin == 0) return BRUSH_ERR_INVALID_ARG;
    if (!means || !log_scales || !rotation || !raw_opacity || !sh_coeffs || !keys || !vals || !state || !workspace)
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(means, 4) || misaligned(log_scales, 4) || misaligned(rotation, 4) || misaligned(raw_opacity, 4) ||
        misaligned(sh_coeffs, 4) || misaligned(keys, 4) || misaligned(vals, 4) || misaligned(state, 4) ||
        misaligned(workspace, 256))
        return BRUSH_ERR_INVALID_ARG;
    const PackWs ws = carve_pack(workspace, n);
    if (workspace_bytes < ws.bytes) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t rows = bounds_rows(n);
    hipLaunchKernelGGL(k_pack_bounds, dim3(rows), dim3(kThreads), 0, s, means, log_scales, rotation, raw_opacity,
                       sh_coeffs, n, cin * 3, ws.partials);
    BRUSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pack_bounds_finish, dim3(1), dim3(kThreads), 0, s, ws.partials, rows, n, ws.bounds, state);
    BRUSH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pack_keys, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, means, n, ws.bounds, keys, vals);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_splat_pack(const float *means, const float *log_scales, const float *rotation,
                                const float *raw_opacity, const float *sh_coeffs, uint32_t n, uint32_t sh_degree,
                                uint32_t sh_degree_out, const uint32_t *order, float *chunks, uint32_t *words,
                                uint8_t *sh_out, brush_stream_t stream) {
    const uint32_t cin = coeffs_of_degree(sh_degree);
    if (n == 0 || n > BRUSH_SPLAT_PACK_MAX || cin == 0 || sh_degree_out > sh_degree) return BRUSH_ERR_INVALID_ARG;
    if (!means || !log_scales || !rotation || !raw_opacity || !sh_coeffs || !order || !chunks || !words ||
        (sh_degree_out > 0 && !sh_out))
        return BRUSH_ERR_INVALID_ARG;
    // the SH rows of degrees 1 and 3 are read as whole 16-byte loads
    const uintptr_t sh_align = (cin * 3) % 4 == 0 ? 16 : 4;
    if (misaligned(means, 4) || misaligned(log_scales, 4) || misaligned(rotation, 16) || misaligned(raw_opacity, 4) ||
        misaligned(sh_coeffs, sh_align) || misaligned(order, 4) || misaligned(chunks, 4) || misaligned(words, 16) ||
        misaligned(sh_out, 4))
        return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(n, kThreads)), block(kThreads);
    uint4 *w4 = reinterpret_cast<uint4 *>(words);
    uint32_t *sh32 = reinterpret_cast<uint32_t *>(sh_out);
#define BRUSH_PACK_CASE(DIN, DOUT)                                                                                  \
    if (sh_degree == DIN && sh_degree_out == DOUT)                                                                  \
        hipLaunchKernelGGL((k_splat_pack<(DIN + 1) * (DIN + 1), (DOUT + 1) * (DOUT + 1) - 1>), grid, block, 0, s, means, \
                           log_scales, rotation, raw_opacity, sh_coeffs, n, order, chunks, w4, sh32);
    BRUSH_PACK_CASE(0, 0)
    BRUSH_PACK_CASE(1, 0) BRUSH_PACK_CASE(1, 1)
    BRUSH_PACK_CASE(2, 0) BRUSH_PACK_CASE(2, 1) BRUSH_PACK_CASE(2, 2)
    BRUSH_PACK_CASE(3, 0) BRUSH_PACK_CASE(3, 1) BRUSH_PACK_CASE(3, 2) BRUSH_PACK_CASE(3, 3)
#undef BRUSH_PACK_CASE
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_splat_unpack(const float *chunks, const uint32_t *words, const uint8_t *sh_in, uint32_t n,
                                  uint32_t sh_degree, float *means, float *log_scales, float *rotation,
                                  float *raw_opacity, float *sh_coeffs, brush_stream_t stream) {
    if (n == 0 || n > BRUSH_SPLAT_PACK_MAX || sh_degree > 3) return BRUSH_ERR_INVALID_ARG;
    if (!chunks || !words || (sh_degree > 0 && !sh_in) || !means || !log_scales || !rotation || !raw_opacity ||
        !sh_coeffs)
        return BRUSH_ERR_INVALID_ARG;
    const uintptr_t sh_align = (coeffs_of_degree(sh_degree) * 3) % 4 == 0 ? 16 : 4;
    if (misaligned(chunks, 4) || misaligned(words, 16) || misaligned(sh_in, 4) || misaligned(means, 4) ||
        misaligned(log_scales, 4) || misaligned(rotation, 16) || misaligned(raw_opacity, 4) ||
        misaligned(sh_coeffs, sh_align))
        return BRUSH_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(n, kThreads)), block(kThreads);
    const uint4 *w4 = reinterpret_cast<const uint4 *>(words);
#define BRUSH_UNPACK_CASE(D)                                                                                        \
    if (sh_degree == D)                                                                                             \
        hipLaunchKernelGGL((k_splat_unpack<(D + 1) * (D + 1) - 1>), grid, block, 0, s, chunks, w4, sh_in, n, means,  \
                           log_scales, rotation, raw_opacity, sh_coeffs);
    BRUSH_UNPACK_CASE(0) BRUSH_UNPACK_CASE(1) BRUSH_UNPACK_CASE(2) BRUSH_UNPACK_CASE(3)
#undef BRUSH_UNPACK_CASE
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
