// resize.hip — the two resamplers behind the device image pyramid (brush_amd/pyramid.py): an exact area (box) filter
// for the u8 training images (brush_area_resize_u8) and a nearest-neighbour pick for depth maps (brush_nearest_resize).
//
// Area filter, in integers.  x is measured in units where a source pixel is ow wide and an output pixel w wide (y: oh
// and h), so output column X covers [X w, (X+1) w), source column s covers [s ow, (s+1) ow) and
//   wx(X,s) = max(0, min((X+1) w, (s+1) ow) - max(X w, s ow)),   wy(Y,r) likewise,   sum_s wx = w,  sum_r wy = h,
//   dst[Y,X,c] = floor((sum_r sum_s wy wx src[r,s,c] + floor(D / 2)) / D),   D = w h.
// One rounding, at the end; no floating point.  The sum is separable without being rounded in between: per source row
// the horizontal sum hs = sum_s wx src (at most 255 w < 2^22) is formed once and enters the accumulator as wy hs.  The
// accumulator reaches 255 w h: the entry point picks the 32-bit kernel while 255 D + D / 2 < 2^32 and the 64-bit one
// above (just over 4096^2); both divide exactly.
//
//   k_area_resize<CH, ACC>: a workgroup of 256 lanes (64 when the image gives few workgroups) owns as many output
//       columns of a strip of output rows, one output pixel (all channels) per lane.  It walks the strip's source rows
//       once, top to bottom.  The rows' bytes are staged into LDS with 16-byte loads at lane-contiguous, 16-byte aligned
//       addresses (RGB rows are byte-addressed: a row's first byte is aligned down, and the lanes read their taps from
//       LDS at the remainder), a strip's rows in one barrier round while they fit in 32 KiB, one row in chunks when
//       the columns under the workgroup do not.  A source row is at most as high as an output row, so
//       it ends at most one output row and begins at most one: the lanes finish that row (divide, store) and start the
//       next from the same hs.  Every branch around a barrier is uniform in the workgroup.
//   k_area_resize_int<CH>: w / ow and h / oh integers (a pyramid level of an image whose sides the factor divides): all
//       weights are equal, so the lanes add plain bytes and divide by 2 fx fy with one multiply-high; same staging.
//   k_nearest_resize<T>: one output element per lane, dst[Y,X] = src[min(((2Y+1) h) / (2 oh), h-1), the same in x]:
//       dataset.resize_nearest bit for bit (elements are moved as 16- or 32-bit words, so NaN payloads survive).
// No atomics, no allocation, no synchronisation: graph-capturable, and the same inputs give the same bits.
// Roofline: HBM stream.  Per output pixel the area filter reads (w h) / (ow oh) source pixels of CH bytes once and
// writes CH bytes: 4 CH + CH = 15 | 20 bytes at a halving, 16 CH + CH = 51 | 68 at a quartering.  Where h / oh is not an
// integer the first source row of a strip is also the last of the strip above (read twice; strips of up to kMaxStripRows rows bound it).
// The nearest pick reads one element per output element, at a stride of w / ow elements: it uses 1 / (w / ow) of the
// lines it fetches; depth maps are a sixth of an RGB image's traffic at most and are resized once per level switch.
#include "internal.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxSide = 16384;
// LDS of one workgroup, in 16-byte vectors: what its rounds need (the kernel waits on memory latency, so the launch
// asks for no more and keeps the CU's wave slots filled), between 1 KiB and 32 KiB.
constexpr uint32_t kMinLdsVecs = 64, kMaxLdsVecs = 2048;
// Source rows staged per barrier round, at most, when they fit: their loads are in flight together.
constexpr uint32_t kMaxBatchRows = 16;
// Output rows of one workgroup's strip, at most: a strip re-reads one source row of the strip above.
constexpr uint32_t kMaxStripRows = 8;
constexpr uint32_t kWantWorkgroups = 2048;
// Below this many 256-lane workgroups the columns are cut into 64-lane (one wave) workgroups instead.
constexpr uint32_t kFewWorkgroups = 1024;
constexpr uint32_t kStageUnroll = 4, kTapUnroll = 2;
// k_area_resize_int: fx fy at most this, so that its sums and its multiply-shift division stay exact in 32 bits.
constexpr uint32_t kMaxIntBlock = 256;

struct AreaArgs {
    uint32_t w, h, ow, oh, strip_rows, lds_vecs;
};

// blockDim.x (64 or 256) output columns of a strip of output rows per workgroup.
template <uint32_t CH, typename ACC>
__global__ __launch_bounds__(kThreads) void k_area_resize(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          const AreaArgs a) {
    extern __shared__ uint4 stage[];  // a.lds_vecs vectors
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(stage);
    const uint32_t w = a.w, h = a.h, ow = a.ow, oh = a.oh, T = blockDim.x;
    // this workgroup: output columns [X0, X1), output rows [Y0, Y1), source columns [c_lo, c_hi), rows [r_lo, r_hi)
    const uint32_t X0 = blockIdx.x * T, X1 = min(X0 + T, ow);
    const uint32_t Y0 = blockIdx.y * a.strip_rows, Y1 = min(Y0 + a.strip_rows, oh);
    const uint32_t c_lo = (X0 * w) / ow, c_hi = (X1 * w - 1u) / ow + 1u;
    const uint32_t r_lo = (Y0 * h) / oh, r_hi = (Y1 * h - 1u) / oh + 1u;
    // this lane: output column X, source columns [sa, sb]
    const uint32_t X = X0 + threadIdx.x;
    const bool live = X < X1;
    const uint32_t xl = X * w, xr = xl + w;
    const uint32_t sa = live ? xl / ow : 1u, sb = live ? (xr - 1u) / ow : 0u;
    const ACC D = (ACC)w * (ACC)h, half = D / 2;
    // A staged row starts at its first byte aligned down to 16 and ends at most 15 bytes behind its last: both ends lie
    // in 16-byte words that hold a byte of the image, so inside its pages.  A row of `bytes` bytes takes at most
    // ceil(bytes / 16) + 1 vectors.  When the columns under the workgroup fit, a round stages several rows, one slot
    // each; else one row in chunks that leave room for the 15 + 15 bytes of slack.
    const uint32_t slot = ((c_hi - c_lo) * CH + 15u) / 16u + 1u;
    const bool fits = slot <= a.lds_vecs;
    const uint32_t batch = fits ? min(a.lds_vecs / slot, kMaxBatchRows) : 1u;
    const uint32_t chunk_cols = fits ? c_hi - c_lo : (a.lds_vecs * 16u - 32u) / CH;
    const uintptr_t src0 = reinterpret_cast<uintptr_t>(src);

    uint32_t Y = Y0;
    ACC acc[CH];
    uint32_t hs[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) acc[c] = 0, hs[c] = 0;
    for (uint32_t r0 = r_lo; r0 < r_hi; r0 += batch) {
        const uint32_t nr = min(batch, r_hi - r0);
        for (uint32_t cs = c_lo; cs < c_hi; cs += chunk_cols) {
            const uint32_t ce = min(cs + chunk_cols, c_hi);
            const uint32_t bytes = (ce - cs) * CH;
            __syncthreads();  // the previous round has been read
            // kStageUnroll rows' loads are issued before the first is stored
            for (uint32_t i = threadIdx.x; i < slot; i += T) {
                for (uint32_t j0 = 0; j0 < nr; j0 += kStageUnroll) {
                    uint4 v[kStageUnroll];
                    bool ok[kStageUnroll];
#pragma unroll
                    for (uint32_t u = 0; u < kStageUnroll; ++u) {
                        const uintptr_t first = src0 + ((size_t)(r0 + j0 + u) * w + cs) * CH;
                        const uint32_t pad = (uint32_t)(first & 15u);
                        ok[u] = j0 + u < nr && i < (pad + bytes + 15u) / 16u;
                        if (ok[u]) v[u] = reinterpret_cast<const uint4 *>(first - pad)[i];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kStageUnroll; ++u)
                        if (ok[u]) stage[(j0 + u) * slot + i] = v[u];
                }
            }
            __syncthreads();
            for (uint32_t j = 0; j < nr; ++j) {
                const uint32_t r = r0 + j;
                if (cs == c_lo) {
#pragma unroll
                    for (uint32_t c = 0; c < CH; ++c) hs[c] = 0;
                }
                if (live) {
                    const uint32_t pad = (uint32_t)((src0 + ((size_t)r * w + cs) * CH) & 15u);
                    const uint8_t *row = lds + (size_t)j * slot * 16u + pad;
                    const uint32_t s0 = max(sa, cs), s1 = min(sb + 1u, ce);
                    // kTapUnroll taps' bytes are read before the first is used; a tap past the last weighs 0
                    for (uint32_t s = s0; s < s1; s += kTapUnroll) {
                        uint32_t wx[kTapUnroll], px[kTapUnroll][CH];
#pragma unroll
                        for (uint32_t u = 0; u < kTapUnroll; ++u) {
                            const bool in = s + u < s1;
                            const uint32_t su = in ? s + u : s;
                            wx[u] = in ? min(xr, (su + 1u) * ow) - max(xl, su * ow) : 0u;
                            const uint8_t *p = row + (su - cs) * CH;
#pragma unroll
                            for (uint32_t c = 0; c < CH; ++c) px[u][c] = p[c];
                        }
#pragma unroll
                        for (uint32_t u = 0; u < kTapUnroll; ++u)
#pragma unroll
                            for (uint32_t c = 0; c < CH; ++c) hs[c] += wx[u] * px[u][c];
                    }
                }
                if (ce != c_hi) continue;  // (one row per round here) more chunks of row r to come
                // row r covers [r oh, (r+1) oh); output row Y covers [Y h, (Y+1) h)
                const uint32_t rt = r * oh, rb = rt + oh, yb = (Y + 1u) * h;
                const uint32_t wy = min(rb, yb) - max(rt, Y * h);
#pragma unroll
                for (uint32_t c = 0; c < CH; ++c) acc[c] += (ACC)wy * (ACC)hs[c];
                if (rb >= yb) {  // row r is the last of output row Y
                    if (live) {
                        uint8_t *q = dst + ((size_t)Y * ow + X) * CH;
#pragma unroll
                        for (uint32_t c = 0; c < CH; ++c) q[c] = (uint8_t)((acc[c] + half) / D);
                    }
                    ++Y;
                    const uint32_t wy2 = (rb > yb && Y < Y1) ? rb - yb : 0u;  // and the first of the next one
#pragma unroll
                    for (uint32_t c = 0; c < CH; ++c) acc[c] = (ACC)wy2 * (ACC)hs[c];
                }
            }
        }
    }
}

struct IntArgs {
    uint32_t w, ow, oh, fx, fy, lds_vecs, magic;
};

// w = fx ow and h = fy oh: every non-zero weight is ow oh, so with S the plain sum of an fy x fx block and n = fx fy the
// definition reads floor((S ow oh + floor(D / 2)) / D) = floor((2 S + n) / (2 n)) (for odd D the two numerators differ
// by less than one unit of 1 / (2 D) and (2 S + n) / (2 n) is no integer, n being odd).  With a = 2 S + n < 2^17 and
// d = 2 n <= 512 the division is (a magic) >> 32 for magic = ceil(2^32 / d), exactly: the excess a e / (d 2^32), e < d,
// stays below 1 / d.  One output row and blockDim.x output columns per workgroup, its fy source rows staged as above.
template <uint32_t CH>
__global__ __launch_bounds__(kThreads) void k_area_resize_int(const uint8_t *__restrict__ src,
                                                              uint8_t *__restrict__ dst, const IntArgs a) {
    extern __shared__ uint4 stage[];  // a.lds_vecs vectors
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(stage);
    const uint32_t T = blockDim.x, X0 = blockIdx.x * T, X1 = min(X0 + T, a.ow), Y = blockIdx.y;
    const uint32_t X = X0 + threadIdx.x;
    const bool live = X < X1;
    const uint32_t cs = X0 * a.fx, bytes = (X1 - X0) * a.fx * CH;
    const uint32_t slot = (bytes + 15u) / 16u + 1u;  // <= a.lds_vecs (entry point)
    const uint32_t batch = min(a.lds_vecs / slot, kMaxBatchRows);
    const uintptr_t src0 = reinterpret_cast<uintptr_t>(src);
    uint32_t sum[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) sum[c] = 0;
    for (uint32_t j00 = 0; j00 < a.fy; j00 += batch) {
        const uint32_t nr = min(batch, a.fy - j00), r0 = Y * a.fy + j00;
        __syncthreads();  // the previous round has been read
        for (uint32_t i = threadIdx.x; i < slot; i += T) {
            for (uint32_t j0 = 0; j0 < nr; j0 += kStageUnroll) {
                uint4 v[kStageUnroll];
                bool ok[kStageUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kStageUnroll; ++u) {
                    const uintptr_t first = src0 + ((size_t)(r0 + j0 + u) * a.w + cs) * CH;
                    const uint32_t pad = (uint32_t)(first & 15u);
                    ok[u] = j0 + u < nr && i < (pad + bytes + 15u) / 16u;
                    if (ok[u]) v[u] = reinterpret_cast<const uint4 *>(first - pad)[i];
                }
#pragma unroll
                for (uint32_t u = 0; u < kStageUnroll; ++u)
                    if (ok[u]) stage[(j0 + u) * slot + i] = v[u];
            }
        }
        __syncthreads();
        if (live) {
            for (uint32_t j = 0; j < nr; ++j) {
                const uint32_t pad = (uint32_t)((src0 + ((size_t)(r0 + j) * a.w + cs) * CH) & 15u);
                const uint8_t *p = lds + (size_t)j * slot * 16u + pad + threadIdx.x * a.fx * CH;
#pragma unroll 4
                for (uint32_t t = 0; t < a.fx; ++t) {
#pragma unroll
                    for (uint32_t c = 0; c < CH; ++c) sum[c] += p[t * CH + c];
                }
            }
        }
    }
    if (live) {
        const uint32_t n = a.fx * a.fy;
        uint8_t *q = dst + ((size_t)Y * a.ow + X) * CH;
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) q[c] = (uint8_t)__umulhi(2u * sum[c] + n, a.magic);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_nearest_resize(const T *__restrict__ src, T *__restrict__ dst, uint32_t w,
                                                             uint32_t h, uint32_t ow, uint32_t oh) {
    const uint32_t X = blockIdx.x * kThreads + threadIdx.x, Y = blockIdx.y;
    if (X >= ow) return;
    const uint32_t r = min(((2u * Y + 1u) * h) / (2u * oh), h - 1u);
    const uint32_t s = min(((2u * X + 1u) * w) / (2u * ow), w - 1u);
    dst[(size_t)Y * ow + X] = src[(size_t)r * w + s];
}

inline bool bad_sizes(uint32_t w, uint32_t h, uint32_t ow, uint32_t oh) {
    return w == 0 || h == 0 || ow == 0 || oh == 0 || w > kMaxSide || h > kMaxSide || ow > w || oh > h;
}
inline bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <uint32_t CH>
void launch_area(const uint8_t *src, uint8_t *dst, const AreaArgs &a, dim3 grid, uint32_t threads, bool wide,
                 hipStream_t s) {
    const size_t lds = (size_t)a.lds_vecs * 16;
    if (wide)
        hipLaunchKernelGGL((k_area_resize<CH, uint64_t>), grid, dim3(threads), lds, s, src, dst, a);
    else
        hipLaunchKernelGGL((k_area_resize<CH, uint32_t>), grid, dim3(threads), lds, s, src, dst, a);
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_area_resize_u8(const uint8_t *src, uint32_t w, uint32_t h, uint32_t channels, uint8_t *dst,
                                    uint32_t ow, uint32_t oh, brush_stream_t stream) {
    if (!src || !dst || bad_sizes(w, h, ow, oh) || (channels != 3 && channels != 4)) return BRUSH_ERR_INVALID_ARG;
    if (overlap(src, (size_t)w * h * channels, dst, (size_t)ow * oh * channels)) return BRUSH_ERR_INVALID_ARG;
    const uint32_t threads = (uint64_t)ceil_div(ow, kThreads) * oh < kFewWorkgroups ? kWave : kThreads;
    const uint32_t col_groups = ceil_div(ow, threads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // integer ratios with blocks of at most kMaxIntBlock pixels whose rows fit the staging buffer: the plain-sum kernel
    const uint32_t fx = w / ow, fy = h / oh;
    const uint32_t int_slot = (threads * fx * channels + 15u) / 16u + 1u;
    if (fx * ow == w && fy * oh == h && (uint64_t)fx * fy <= kMaxIntBlock && int_slot <= kMaxLdsVecs) {
        IntArgs ia;
        ia.w = w, ia.ow = ow, ia.oh = oh, ia.fx = fx, ia.fy = fy;
        ia.lds_vecs = min(max(int_slot * min(fy, kMaxBatchRows), kMinLdsVecs), kMaxLdsVecs);
        ia.magic = (uint32_t)(((1ull << 32) + 2ull * fx * fy - 1ull) / (2ull * fx * fy));
        const dim3 grid(col_groups, oh);
        if (channels == 3)
            hipLaunchKernelGGL(k_area_resize_int<3>, grid, dim3(threads), (size_t)ia.lds_vecs * 16, s, src, dst, ia);
        else
            hipLaunchKernelGGL(k_area_resize_int<4>, grid, dim3(threads), (size_t)ia.lds_vecs * 16, s, src, dst, ia);
        BRUSH_HIP_CHECK(hipGetLastError());
        return BRUSH_OK;
    }
    AreaArgs a;
    a.w = w, a.h = h, a.ow = ow, a.oh = oh;
    // enough workgroups to fill the chip first, then strips as high as kMaxStripRows
    a.strip_rows = min(max((uint32_t)(((uint64_t)oh * col_groups) / kWantWorkgroups), 1u), kMaxStripRows);
    const dim3 grid(col_groups, ceil_div(oh, a.strip_rows));
    // LDS for one round of a strip's source rows: bounds of the kernel's `slot` and of a strip's row count
    const uint32_t slot = (((threads * w) / ow + 2u) * channels + 15u) / 16u + 1u;
    const uint32_t rows = min((a.strip_rows * h) / oh + 2u, kMaxBatchRows);
    a.lds_vecs = (uint32_t)min(max((uint64_t)slot * rows, (uint64_t)kMinLdsVecs), (uint64_t)kMaxLdsVecs);
    const uint64_t D = (uint64_t)w * h;
    const bool wide = 255ull * D + D / 2 >= (1ull << 32);
    if (channels == 3)
        launch_area<3>(src, dst, a, grid, threads, wide, s);
    else
        launch_area<4>(src, dst, a, grid, threads, wide, s);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_nearest_resize(const void *src, uint32_t elem_bytes, uint32_t w, uint32_t h, void *dst,
                                    uint32_t ow, uint32_t oh, brush_stream_t stream) {
    if (!src || !dst || bad_sizes(w, h, ow, oh) || (elem_bytes != 2 && elem_bytes != 4)) return BRUSH_ERR_INVALID_ARG;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & (elem_bytes - 1u)) != 0)
        return BRUSH_ERR_INVALID_ARG;
    if (overlap(src, (size_t)w * h * elem_bytes, dst, (size_t)ow * oh * elem_bytes)) return BRUSH_ERR_INVALID_ARG;
    const dim3 grid(ceil_div(ow, kThreads), oh);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(k_nearest_resize<uint16_t>, grid, dim3(kThreads), 0, s, static_cast<const uint16_t *>(src),
                           static_cast<uint16_t *>(dst), w, h, ow, oh);
    else
        hipLaunchKernelGGL(k_nearest_resize<uint32_t>, grid, dim3(kThreads), 0, s, static_cast<const uint32_t *>(src),
                           static_cast<uint32_t *>(dst), w, h, ow, oh);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
