// rasterize.hip — per-tile front-to-back alpha compositing: the forward kernel and its launcher.  Its backward pass
// is rasterize_bwd.hip; what both share is raster_common.hpp.
//
// Replaces:
//   Rasterize           crates/brush-render/src/shaders/rasterize.wgsl:20-115
//
// gfx950 layout: pixels of an 8x8 QUADRANT of a 16x16 tile map to the 64 lanes of a wave (lane = x + 8 y), the tile's
// depth-sorted splat list is staged in LDS in batches of 64 records (one gathered 36-byte record per lane) and read back
// as wave-uniform broadcasts, and a (record, quadrant) pair whose alpha provably stays below 1/255 on the whole quadrant
// is skipped by a scalar branch (see "footprint-aware kernels", raster_common.hpp).  Workgroups are dealt to XCDs
// round-robin, so block ids are remapped to give every XCD a contiguous band of tiles: neighbouring tiles gather the
// same splat records from one L2.  Waves of a workgroup never exchange data: no s_barrier, no LDS atomics.
//
// One wave per quadrant (4 waves = 1 tile per workgroup); identical arithmetic to the reference per pixel; the wave
// leaves the list as soon as all of its pixels have saturated (the reference walks every batch, rasterize.wgsl:57-101;
// same result).
//
// Roofline: bound by fp32 VALU issue, not by HBM; DESIGN.md states the ceilings and the measurements.
#include "raster_common.hpp"
#include "trace.hpp"

namespace brush {
namespace {

// One staged record of the footprint-aware kernels: 48 bytes, read back as wave-uniform broadcasts.
struct QuadRec {
    float4 a;  // mean.x, mean.y, conic.x, conic.y
    float4 b;  // conic.z, r, g, b
    float4 c;  // opacity, -, -, -
};
// static LDS of a forward workgroup: what the kernel descriptors of a build report (tests/test_host_cpu.py)
static_assert(sizeof(QuadRec) * kTilesPerBlock * kBatch == 12288, "one QuadRec per wave and batch slot");

// Forward: ONE wave64 per 8x8 quadrant, one pixel per lane; the four waves of a workgroup are the four
// quadrants of one tile (they gather the same records, so three of the four gathers hit L1/L2).
// A pixel that has saturated gets a NaN pixel centre: every later `power <= 0` test fails for it, so the
// per-record path carries no separate "live" predicate.
//
// DEPTH (brush_render_forward_depth): the accumulated depth D = sum T alpha z of the same entries is carried beside the
// colour; z (camera-space z of the splat's mean, the depth sort's key, compact order) rides in the record's spare lanes.
// Everything else, the RGBA image included, is computed exactly as without it.
// The depth instantiation takes one more argument, a DepthOut; without it the kernel's signature is the plain one.
struct DepthOut {
    const float *compact_depth;  // [N] z, compact order
    float *out_depth;            // [h][w]
};

template <bool RASTER_U32, typename... Depth>
__global__ __launch_bounds__(kRasterThreads) void k_rasterize_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    uint32_t *__restrict__ tile_bins, const uint32_t *__restrict__ bin_edges, const float *__restrict__ projected,
    void *__restrict__ out_img, uint32_t *__restrict__ final_index, uint32_t u32_pitch,
    float4 *__restrict__ zero_rows, const uint32_t *__restrict__ num_visible, uint32_t n_splats, const Depth... depth) {
    constexpr bool DEPTH = sizeof...(Depth) != 0;
    static_assert(sizeof...(Depth) <= 1 && !(RASTER_U32 && DEPTH), "depth: one DepthOut, float image");
    __shared__ QuadRec lds_all[kTilesPerBlock][kBatch];
    BRUSH_KTRACE(kTrRasterize, 0);
    if (zero_rows) {
        // BrushAux::bwd_accum: the backward's compact-order accumulator rows of this render, zeroed here so that the
        // backward needs no zero-fill launch (fire-and-forget stores beside a kernel that is bound by VALU issue)
        const uint32_t words = min(*num_visible, n_splats) * kCompactVec;
        for (uint32_t i = blockIdx.x * kRasterThreads + threadIdx.x; i < words; i += gridDim.x * kRasterThreads)
            zero_rows[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    QuadRec *lds = lds_all[q];
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
    float T = 1.0f, cr = 0.0f, cg = 0.0f, cb_ = 0.0f;
    float cd = 0.0f;  // DEPTH: accumulated depth
    uint32_t fin = 0;
    uint32_t r0, r1;
    if (bin_edges) {
        // GetTileBinEdges (get_tile_bin_edges.wgsl:15-42) without its launch: the tile sort's last pass left
        // (max ~start, max end) of this tile's run; (0, 0) = the tile id does not occur.  Quadrant 0 (always inside
        // the frame) publishes the decoded pair for the aux and the backward.
        const uint32_t ns = bin_edges[tile_id * 2];
        r1 = bin_edges[tile_id * 2 + 1];
        r0 = r1 ? ~ns : 0u;
        if (q == 0u && lane == 0u) {
            tile_bins[tile_id * 2] = r0;
            tile_bins[tile_id * 2 + 1] = r1;
        }
    } else {
        r0 = tile_bins[tile_id * 2], r1 = tile_bins[tile_id * 2 + 1];
    }
    for (uint32_t batch_start = r0; batch_start < r1 && live != 0ull; batch_start += kBatch) {
        const uint32_t remaining = min(kBatch, r1 - batch_start);
        bool hit = false;
        float rec[9];
        float z = 0.0f;
        if (lane < remaining) {
            const uint32_t cgid = gid_from_isect[batch_start + lane];
            const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;
#pragma unroll
            for (int k = 0; k < 9; k++) rec[k] = p[k];
            if constexpr (DEPTH) z = only(depth...).compact_depth[cgid];
            hit = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[8], bx, by);
        }
        uint64_t mask = ballot64(hit);
        if (mask == 0ull) continue;
        wave_sync();  // the previous batch's broadcasts are done (LDS is in order per wave)
        if (hit) {
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds[lane].b = make_float4(rec[4], rec[5], rec[6], rec[7]);
            lds[lane].c = make_float4(rec[8], z, 0.f, 0.f);
        }
        wave_sync();
        while (mask != 0ull) {
            const uint32_t t = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const float4 a = lds[t].a;
            const float4 b = lds[t].b;
            const float opac = lds[t].c.x;
            // rasterize.wgsl:80-99
            const float dx = a.x - pcx, dy = a.y - pcy;
            // The reference's association, 0.5 (a dx^2 + c dy^2) + b dx dy: folding -log2(e)/2 into the conic saves
            // three instructions but moves alpha by ~1e-5 relative on correlated conics, enough to flip
            // `alpha >= 1/255` outside the oracle's guard band on a 20 M-splat frame (measured: 3.7e-4 pixel error).
            const float sigma = fmaf(0.5f, fmaf(a.z * dx, dx, (b.x * dy) * dy), (a.w * dy) * dx);
            const float power = sigma * kNegLog2e;
            const float alpha_u = opac * __builtin_amdgcn_exp2f(power);
            if (power <= 0.0f && alpha_u >= 1.0f / 255.0f) {  // never true for a saturated pixel (NaN)
                const float alpha = vmin(0.999f, alpha_u);
                const float next_T = T * (1.0f - alpha);
                if (next_T <= 1e-4f) {  // :88-91: stop WITHOUT adding this entry
                    pcx = __builtin_nanf("");
                } else {
                    const float fac = alpha * T;
                    cr = fmaf(b.y, fac, cr);
                    cg = fmaf(b.z, fac, cg);
                    cb_ = fmaf(b.w, fac, cb_);
                    if constexpr (DEPTH) cd = fmaf(lds[t].c.y, fac, cd);
                    T = next_T;
                    fin = batch_start + t;
                }
            }
            // all pixels saturated?  one compare every 4th record (the lane mask comes straight out of it)
            if ((++walked & 3u) == 0u) {
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;
                if (live == 0ull) break;
            }
        }
    }
    if (inside) {
        const float al = 1.0f - T;
        if (RASTER_U32) {
            // rasterize.wgsl:106-109; rows `u32_pitch` pixels apart (burn_texture.rs:17-26)
            const uint32_t r8 = (uint32_t)fminf(fmaxf(cr * 255.0f, 0.0f), 255.0f);
            const uint32_t g8 = (uint32_t)fminf(fmaxf(cg * 255.0f, 0.0f), 255.0f);
            const uint32_t b8 = (uint32_t)fminf(fmaxf(cb_ * 255.0f, 0.0f), 255.0f);
            const uint32_t a8 = (uint32_t)fminf(fmaxf(al * 255.0f, 0.0f), 255.0f);
            static_cast<uint32_t *>(out_img)[(size_t)px + (size_t)py * u32_pitch] = r8 | (g8 << 8) | (b8 << 16) | (a8 << 24);
        } else {
            const size_t pix = (size_t)px + (size_t)py * w;
            static_cast<float4 *>(out_img)[pix] = make_float4(cr, cg, cb_, al);
            final_index[pix] = fin;
            if constexpr (DEPTH) only(depth...).out_depth[pix] = cd;
        }
    }
}

}  // namespace

hipError_t launch_rasterize(const RasterFrame &f, const RasterOut &out, const uint32_t *bin_edges, float *zero_rows,
                            const uint32_t *num_visible, uint32_t n, hipStream_t s) {
    const uint32_t tiles = f.tbx * f.tby;
    if (tiles == 0) return hipSuccess;
    // one workgroup (4 quadrant waves) per tile
    const dim3 grid(ceil_div(tiles, 8u) * 8u), block(kRasterThreads);
    if (out.out_depth && (out.raster_u32 || !out.compact_depth)) return hipErrorInvalidValue;
    auto launch = [&](auto u32, const auto... depth) {
        hipLaunchKernelGGL((k_rasterize_quad<u32(), std::decay_t<decltype(depth)>...>), grid, block, 0, s, f.w, f.h,
                           f.tbx, tiles, f.compact_gid_from_isect, f.tile_bins, bin_edges, f.projected, out.img,
                           f.final_index, out.u32_pitch, reinterpret_cast<float4 *>(zero_rows), num_visible, n, depth...);
    };
    if (out.out_depth) launch(std::false_type{}, DepthOut{out.compact_depth, out.out_depth});
    else if (out.raster_u32) launch(std::true_type{});
    else launch(std::false_type{});
    return hipGetLastError();
}

}  // namespace brush
