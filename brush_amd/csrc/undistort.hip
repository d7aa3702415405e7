// undistort.hip — resamples a distorted COLMAP view into the pinhole camera the rasterizer assumes
// (brush_amd/undistort.py): brush_undistort_u8 for the u8 training images, brush_undistort_nearest for depth maps.
//
// The definition.  All float operations are float32, round to nearest, never contracted (the Makefile's EXACT flags);
// pixel centres are at +0.5.  For output pixel (X, Y) of an ow x oh pinhole image with principal point (ocx, ocy) and
// inverse focal (iofx, iofy), and a w x h source with focal (fx, fy), principal point (cx, cy) and the coefficients
// k1..k6, p1, p2 of OpenCV's rational model (a model's missing coefficients are zero: SIMPLE_RADIAL has k1, RADIAL k1
// k2, OPENCV k1 k2 p1 p2, FULL_OPENCV all eight):
//   x  = ((float)X + 0.5f - ocx) * iofx            y likewise
//   r2 = x*x + y*y
//   num = 1 + r2*(k1 + r2*(k2 + r2*k3))            den = 1 + r2*(k4 + r2*(k5 + r2*k6))
//   rad = num / den                                 (always divided; IEEE division)
//   a  = x*y
//   xd = x*rad + ((2*p1)*a + p2*(r2 + (2*x)*x))
//   yd = y*rad + (p1*(r2 + (2*y)*y) + (2*p2)*a)
//   u  = (fx*xd + cx) - 0.5f                        v = (fy*yd + cy) - 0.5f      (source index space)
//   qx = (int32) rintf(u * 256.0f)                  qy likewise                  (Q8; NaN or |.| >= 2^30 -> invalid)
// A pixel is valid iff 0 <= qx <= (w-1) 256 and 0 <= qy <= (h-1) 256.
// Image (u8, 3 or 4 channels): x0 = qx >> 8, ax = qx & 255, x1 = min(x0+1, w-1), the same in y; every channel on its
//   own, dst = (sum over the four taps of (256-ax | ax) (256-ay | ay) src + 32768) >> 16: one rounding, in integers,
//   the sum stays below 2^24.  An invalid pixel is 0 in every channel; the optional u8 [oh][ow] mask gets 1 | 0.
// Depth map (16- or 32-bit elements [h][w]): the element at ((qx+128)>>8, (qy+128)>>8), each clamped to the image,
//   moved as a word (NaN payloads survive, as in k_nearest_resize); an invalid pixel is 0, "no measurement": a zero
//   never blends into a neighbour.
//
//   k_undistort_u8<CH>: one output pixel (all channels) per lane, consecutive lanes consecutive X of one output row, a
//       workgroup of 256 lanes: a wave stores 64 CH contiguous bytes.  The four taps are gathered from global memory
//       (the map is smooth: the lanes of a wave read a short run of two source rows, which the vector cache serves).
//   k_undistort_nearest<T>: the same map, one element per lane.
// No atomics, no allocation, no synchronisation: graph-capturable, and the same inputs give the same bits.
// Roofline: HBM stream.  Per output pixel CH bytes written and, at a magnification near 1, CH bytes of source read
// once (each source byte is a tap of about four output pixels, from the caches); about 60 float and integer
// instructions per pixel beside them.
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
// Above this the float32 recipe no longer resolves 1/256 px comfortably (8192 * 256 = 2^21 of the 2^24 integers).
constexpr uint32_t kMaxSide = 8192;

struct Q8 {
    int32_t x, y;
    bool valid;
};

// The definition's qx, qy and validity for output pixel (X, Y).
__device__ __forceinline__ Q8 source_q8(uint32_t X, uint32_t Y, uint32_t w, uint32_t h, const BrushUndistort &m) {
    const float x = ((float)X + 0.5f - m.ocx) * m.iofx, y = ((float)Y + 0.5f - m.ocy) * m.iofy;
    const float r2 = x * x + y * y;
    const float num = 1.0f + r2 * (m.k1 + r2 * (m.k2 + r2 * m.k3));
    const float den = 1.0f + r2 * (m.k4 + r2 * (m.k5 + r2 * m.k6));
    const float rad = num / den;
    const float a = x * y;
    const float xd = x * rad + ((2.0f * m.p1) * a + m.p2 * (r2 + (2.0f * x) * x));
    const float yd = y * rad + (m.p1 * (r2 + (2.0f * y) * y) + (2.0f * m.p2) * a);
    const float u = (m.fx * xd + m.cx) - 0.5f, v = (m.fy * yd + m.cy) - 0.5f;
    const float ru = __builtin_rintf(u * 256.0f), rv = __builtin_rintf(v * 256.0f);
    Q8 q;
    // (a NaN fails both comparisons; inside the bound the conversions are exact)
    const bool finite = __builtin_fabsf(ru) < 1073741824.0f && __builtin_fabsf(rv) < 1073741824.0f;
    q.x = finite ? (int32_t)ru : -1;
    q.y = finite ? (int32_t)rv : -1;
    q.valid = q.x >= 0 && q.x <= (int32_t)((w - 1u) * 256u) && q.y >= 0 && q.y <= (int32_t)((h - 1u) * 256u);
    return q;
}

template <uint32_t CH>
__global__ __launch_bounds__(kThreads) void k_undistort_u8(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                           uint8_t *__restrict__ valid, uint32_t w, uint32_t h,
                                                           uint32_t ow, const BrushUndistort m) {
    const uint32_t X = blockIdx.x * kThreads + threadIdx.x, Y = blockIdx.y;
    if (X >= ow) return;
    const Q8 q = source_q8(X, Y, w, h, m);
    uint32_t out[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) out[c] = 0u;
    if (q.valid) {
        const uint32_t x0 = (uint32_t)q.x >> 8, ax = (uint32_t)q.x & 255u, x1 = min(x0 + 1u, w - 1u);
        const uint32_t y0 = (uint32_t)q.y >> 8, ay = (uint32_t)q.y & 255u, y1 = min(y0 + 1u, h - 1u);
        const uint8_t *r0 = src + (size_t)y0 * w * CH, *r1 = src + (size_t)y1 * w * CH;
        // the sixteen (twelve) bytes are read before the first is used
        uint32_t t00[CH], t01[CH], t10[CH], t11[CH];
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) {
            t00[c] = r0[x0 * CH + c], t01[c] = r0[x1 * CH + c];
            t10[c] = r1[x0 * CH + c], t11[c] = r1[x1 * CH + c];
        }
        const uint32_t bx = 256u - ax, by = 256u - ay;
        const uint32_t w00 = bx * by, w01 = ax * by, w10 = bx * ay, w11 = ax * ay;
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c)
            out[c] = (w00 * t00[c] + w01 * t01[c] + w10 * t10[c] + w11 * t11[c] + 32768u) >> 16;
    }
    uint8_t *p = dst + ((size_t)Y * ow + X) * CH;
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) p[c] = (uint8_t)out[c];
    if (valid) valid[(size_t)Y * ow + X] = q.valid ? 1u : 0u;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_undistort_nearest(const T *__restrict__ src, T *__restrict__ dst,
                                                                uint32_t w, uint32_t h, uint32_t ow,
                                                                const BrushUndistort m) {
    const uint32_t X = blockIdx.x * kThreads + threadIdx.x, Y = blockIdx.y;
    if (X >= ow) return;
    const Q8 q = source_q8(X, Y, w, h, m);
    T e = 0;
    if (q.valid) {
        const uint32_t s = min((uint32_t)(q.x + 128) >> 8, w - 1u), r = min((uint32_t)(q.y + 128) >> 8, h - 1u);
        e = src[(size_t)r * w + s];
    }
    dst[(size_t)Y * ow + X] = e;
}

inline bool bad_sizes(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh) {
    return w == 0 || h == 0 || ow == 0 || oh == 0 || w > kMaxSide || h > kMaxSide || ow > kMaxSide || oh > kMaxSide;
}
inline bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_undistort_u8(const uint8_t *src, uint32_t w, uint32_t h, uint32_t channels, uint8_t *dst,
                                  uint32_t ow, uint32_t oh, uint8_t *valid, const BrushUndistort *map,
                                  brush_stream_t stream) {
    if (!src || !dst || !map || bad_sizes(w, h, ow, oh) || (channels != 3 && channels != 4))
        return BRUSH_ERR_INVALID_ARG;
    const size_t src_bytes = (size_t)w * h * channels, dst_bytes = (size_t)ow * oh * channels;
    if (overlap(src, src_bytes, dst, dst_bytes)) return BRUSH_ERR_INVALID_ARG;
    if (valid && (overlap(valid, (size_t)ow * oh, src, src_bytes) || overlap(valid, (size_t)ow * oh, dst, dst_bytes)))
        return BRUSH_ERR_INVALID_ARG;
    const dim3 grid(ceil_div(ow, kThreads), oh);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (channels == 3)
        hipLaunchKernelGGL(k_undistort_u8<3>, grid, dim3(kThreads), 0, s, src, dst, valid, w, h, ow, *map);
    else
        hipLaunchKernelGGL(k_undistort_u8<4>, grid, dim3(kThreads), 0, s, src, dst, valid, w, h, ow, *map);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_undistort_nearest(const void *src, uint32_t elem_bytes, uint32_t w, uint32_t h, void *dst,
                                       uint32_t ow, uint32_t oh, const BrushUndistort *map, brush_stream_t stream) {
    if (!src || !dst || !map || bad_sizes(w, h, ow, oh) || (elem_bytes != 2 && elem_bytes != 4))
        return BRUSH_ERR_INVALID_ARG;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & (elem_bytes - 1u)) != 0)
        return BRUSH_ERR_INVALID_ARG;
    if (overlap(src, (size_t)w * h * elem_bytes, dst, (size_t)ow * oh * elem_bytes)) return BRUSH_ERR_INVALID_ARG;
    const dim3 grid(ceil_div(ow, kThreads), oh);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(k_undistort_nearest<uint16_t>, grid, dim3(kThreads), 0, s,
                           static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), w, h, ow, *map);
    else
        hipLaunchKernelGGL(k_undistort_nearest<uint32_t>, grid, dim3(kThreads), 0, s,
                           static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), w, h, ow, *map);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
