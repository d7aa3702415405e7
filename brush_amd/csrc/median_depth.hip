// median_depth.hip — median depth and the splat under every pixel: a replay of the forward's compositing walk over the
// tile lists a finished brush_render_forward_depth left behind, ending in a per-pixel PICK instead of a reduction.
// Kernel, launcher and ABI entry (brush_render_median_depth) live here; what the walk shares with rasterize.hip is
// raster_common.hpp.
//
// The reference has no depth output at all; the definition is the one 2DGS, GOF, RaDe-GS and gsplat's 2DGS path fuse
// into their meshes: the depth of the splat at which the accumulated opacity 1 - T first reaches `level` (one half for
// the median), on the forward's own arithmetic (rasterize.wgsl:57-101).
//
// gfx950 layout: the forward's, as contribution.hip has it.  One wave64 per 8x8 quadrant, four waves per tile, the
// XCD-contiguous block remap, records staged per wave in LDS in batches of 64 and read back as wave-uniform
// broadcasts, quad_may_pass() skipping a (record, quadrant) on the scalar unit, no s_barrier, no atomics.  A staged
// record carries xy, conic, opacity, the splat's camera-space z (compact_depth) and its GLOBAL id; colour is not read.
// A pixel is live until it has crossed the level or stopped; the wave leaves the list as soon as no pixel is live, so an
// opaque scene walks the front of every list only.  Every pixel is written by exactly one lane, once: the result is
// bitwise repeatable.
#include "raster_common.hpp"

namespace brush {
namespace {

// One staged record: 32 bytes, read back as wave-uniform broadcasts.
struct MedianRec {
    float4 a;  // mean.x, mean.y, conic.x, conic.y
    float4 b;  // conic.z, opacity, z, global id (bits)
};
// static LDS of a workgroup: what the kernel descriptor of a build reports (tests/test_median_depth_cpu.py)
static_assert(sizeof(MedianRec) * kTilesPerBlock * kBatch == 8192, "one MedianRec per wave and batch slot");

// The forward's walk (k_rasterize_quad, float image) with the same expressions per pixel, as k_contribution_quad
// restates them: sigma, power, alpha_u, the 0.999 clamp, the test `power <= 0 && alpha_u >= 1/255`, next_T and the
// `next_T <= 1e-4` stop WITHOUT adding the entry.  The median entry of a pixel is the first ADDED entry whose next_T is
// <= t_level (= 1.0f - level, rounded once on the host); an entry that stops the pixel is never the median.  A pixel
// that crossed or stopped takes a NaN centre, which fails every later alpha test: it keeps its first crossing and
// counts as not live.
//
// Every inside pixel writes out_depth[pix] = the bits of compact_depth[cgid] of its median entry (0.0f: none) and, with
// out_id, out_id[pix] = that entry's global id (-1: none); n_splats == 0 reads no list at all.
__global__ __launch_bounds__(kRasterThreads) void k_median_depth_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ compact_depth, float t_level, float *__restrict__ out_depth,
    int32_t *__restrict__ out_id) {
    __shared__ MedianRec lds_all[kTilesPerBlock][kBatch];
    const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    MedianRec *lds = lds_all[q];
    const uint32_t tile_id = xcd_contiguous_block();
    if (tile_id >= num_tiles) return;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t qx0 = (tile_id % tbx) * kTileWidth + (q & 1u) * 8u, qy0 = (tile_id / tbx) * kTileWidth + (q >> 1) * 8u;
    if (qx0 >= w || qy0 >= h) return;  // quadrant entirely outside a ragged frame
    const uint32_t px = qx0 + (lane & 7u), py = qy0 + (lane >> 3);
    const float bx = (float)qx0 + 0.5f, by = (float)qy0 + 0.5f;
    const bool inside = px < w && py < h;
    const float pcy = (float)py + 0.5f;  // rasterize.wgsl:32
    float pcx = inside ? (float)px + 0.5f : __builtin_nanf("");

    const uint64_t inside_mask = ballot64(inside);
    uint64_t live = inside_mask;
    uint32_t walked = 0;
    float T = 1.0f;
    float med_z = 0.0f;
    uint32_t med_id = 0xFFFFFFFFu;
    uint32_t nvis = 0, r0 = 0, r1 = 0;
    if (n_splats != 0u) {
        nvis = min(*num_visible, n_splats);
        // a finished forward leaves r0 <= r1 <= min(num_intersections, cap); nothing beyond the list's capacity is read
        r0 = tile_bins[tile_id * 2];
        r1 = min(tile_bins[tile_id * 2 + 1], cap);
    }
    for (uint32_t batch_start = r0; batch_start < r1 && live != 0ull; batch_start += kBatch) {
        const uint32_t remaining = min(kBatch, r1 - batch_start);
        bool may = false;
        float rec[7];
        uint32_t gid = kInvalid;
        if (lane < remaining) {
            const uint32_t cgid = gid_from_isect[batch_start + lane];
            if (cgid < nvis) {  // every entry of a finished forward's list is
                const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;
#pragma unroll
                for (int k = 0; k < 5; k++) rec[k] = p[k];
                rec[5] = p[8];  // the opacity the splat is drawn with (antialiased mode: already compensated)
                rec[6] = compact_depth[cgid];
                gid = global_from_compact[cgid];
                may = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], bx, by);
            }
        }
        uint64_t mask = ballot64(may);
        if (mask == 0ull) continue;
        wave_sync();  // the previous batch's broadcasts are done (LDS is in order per wave)
        if (may) {
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds[lane].b = make_float4(rec[4], rec[5], rec[6], __uint_as_float(gid));
        }
        wave_sync();
        while (mask != 0ull) {
            const uint32_t t = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const float4 a = lds[t].a;
            const float4 b = lds[t].b;
            const float opac = b.y;
            // rasterize.wgsl:80-99, the forward's association (rasterize.hip)
            const float dx = a.x - pcx, dy = a.y - pcy;
            const float sigma = fmaf(0.5f, fmaf(a.z * dx, dx, (b.x * dy) * dy), (a.w * dy) * dx);
            const float power = sigma * kNegLog2e;
            const float alpha_u = opac * __builtin_amdgcn_exp2f(power);
            const bool pass = power <= 0.0f && alpha_u >= 1.0f / 255.0f;  // never true for a dead pixel (NaN)
            const float alpha = vmin(0.999f, alpha_u);
            const float next_T = T * (1.0f - alpha);
            const bool stop = pass && next_T <= 1e-4f;  // :88-91: stop WITHOUT adding this entry
            const bool hit = pass && !stop;
            const bool cross = hit && next_T <= t_level;
            if (hit) T = next_T;
            if (cross) {
                med_z = b.z;
                med_id = __float_as_uint(b.w);
            }
            if (stop || cross) pcx = __builtin_nanf("");
            // no pixel live?  one compare every 4th record, as the forward
            if ((++walked & 3u) == 0u) {
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;
                if (live == 0ull) break;
            }
        }
    }
    if (inside) {
        const size_t pix = (size_t)px + (size_t)py * w;
        out_depth[pix] = med_z;
        if (out_id) out_id[pix] = (int32_t)med_id;
    }
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_render_median_depth(const BrushUniforms *h_uniforms, const BrushAux *h_aux,
                                         const float *compact_depth, float level, float *out_depth, int32_t *out_id,
                                         uint32_t n, brush_stream_t stream) {
    if (!h_uniforms || !h_aux || !compact_depth || !out_depth) return BRUSH_ERR_INVALID_ARG;
    if (!(level > 0.0f && level < 1.0f)) return BRUSH_ERR_INVALID_ARG;  // (a NaN fails too)
    const BrushUniforms &u = *h_uniforms;
    const BrushAux &aux = *h_aux;
    const uint32_t w = u.img_size[0], h = u.img_size[1], tbx = u.tile_bounds[0], tby = u.tile_bounds[1];
    if (!checked_pixels(w, h) || tbx != ceil_div(w, kTileWidth) || tby != ceil_div(h, kTileWidth))
        return BRUSH_ERR_INVALID_ARG;
    if (!aux.projected_splats || !aux.tile_bins || !aux.compact_gid_from_isect || !aux.global_from_compact_gid ||
        !aux.num_visible || aux.max_intersects == 0)
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(compact_depth, 4) || misaligned(out_depth, 4) || misaligned(out_id, 4)) return BRUSH_ERR_INVALID_ARG;
    const float t_level = 1.0f - level;  // once, in float32: what every pixel compares its next_T with
    const uint32_t tiles = tbx * tby;
    // one workgroup (4 quadrant waves) per tile; a multiple of 8 for the XCD remap.  n == 0 launches too: every pixel
    // is written on every call.
    hipLaunchKernelGGL(k_median_depth_quad, dim3(ceil_div(tiles, 8u) * 8u), dim3(kRasterThreads), 0,
                       static_cast<hipStream_t>(stream), w, h, tbx, tiles, aux.compact_gid_from_isect, aux.tile_bins,
                       aux.max_intersects, aux.projected_splats, aux.global_from_compact_gid, aux.num_visible, n,
                       compact_depth, t_level, out_depth, out_id);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
