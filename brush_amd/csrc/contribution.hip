// contribution.hip — per-splat rendered contribution: a replay of the forward's compositing walk over the tile lists a
// finished forward left behind, ending in per-splat reductions instead of a pixel store.  Kernel, launcher and ABI
// entry (brush_render_contributions) live here; what the walk shares with rasterize.hip is raster_common.hpp.
//
// The reference has no such pass (its refinement prunes on sigmoid(raw_opacity) and scale alone, train.rs:395-470);
// the statistic is RadSplat's max blending weight and LightGaussian's summed weight, defined on the forward's own
// arithmetic (rasterize.wgsl:57-101).
//
// gfx950 layout: the forward's.  One wave64 per 8x8 quadrant, four waves per tile, the XCD-contiguous block remap,
// records staged per wave in LDS in batches of 64 and read back as wave-uniform broadcasts, quad_may_pass() skipping a
// (record, quadrant) on the scalar unit, no s_barrier, no LDS atomics.  A staged record carries xy, conic, opacity and
// the splat's GLOBAL id; colour is not read.  Per walked (record, quadrant) that changed a pixel, the wave reduces
// max(fac), sum(rint(fac 2^24)), popcount(added), popcount(stopped) on the VALU (DPP) and lanes 0..2 send them to the
// splat's row with no-return integer atomics: max on the bits of a non-negative float and 64-bit adds, all of them
// order independent, so the result is bitwise repeatable in either aux mode.
#include "raster_common.hpp"

namespace brush {
namespace {

// One staged record: 32 bytes, read back as wave-uniform broadcasts.
struct ContribRec {
    float4 a;  // mean.x, mean.y, conic.x, conic.y
    float4 b;  // conic.z, opacity, global id (bits), -
};
// static LDS of a workgroup: what the kernel descriptor of a build reports (tests/test_contribution_cpu.py)
static_assert(sizeof(ContribRec) * kTilesPerBlock * kBatch == 8192, "one ContribRec per wave and batch slot");

constexpr float kQ24 = 16777216.0f;  // the fixed point of the summed weight: 2^24

// Max over the wave of an unsigned value, in every lane: the DPP ladder of wave_inclusive_scan (lanes without a source
// take 0, the identity), then lane 63 through the scalar unit.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = dpp_max_u32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_max_u32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_max_u32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_max_u32<0x118, 0xf>(v);  // row_shr:8
    v = dpp_max_u32<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
    v = dpp_max_u32<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3
    return wave_bcast(v, 63u);
}

// The forward's walk (k_rasterize_quad, float image) with the same expressions per pixel: sigma, power, alpha_u, the
// 0.999 clamp, the test `power <= 0 && alpha_u >= 1/255`, next_T, the `next_T <= 1e-4` stop and the NaN pixel centre
// after a stop.  It walks until every pixel of the wave has stopped or the list ends, not up to final_index: it must
// see the entry that stops a pixel.
//
// Per walked (record, quadrant) and lane:
//   fac  = alpha * T where the forward added the entry, else 0
//   hit  : the forward added the entry
//   stop : the entry passed the alpha test and ended the pixel WITHOUT being added (rasterize.wgsl:88-91)
// and the splat's row g = global_from_compact_gid[cgid] receives
//   max_bits[g]    = max(max_bits[g], bits(max over lanes of fac))
//   counts[g][0]  += sum over lanes of (uint32) rint(fac 2^24)   (ties to even; at most 64 2^24 per record)
//   counts[g][1]  += popcount(hit),  counts[g][2] += popcount(stop)
// when hit | stop is set in any lane (a scalar branch).  Nothing else is written unless the self-check is on
// (out_img != nullptr): every inside pixel then compares the bits of its replayed 1 - T with out_img[pix].w and its
// last added entry with final_index[pix]; the wave adds the count of differing pixels to mismatch[0].
__global__ __launch_bounds__(kRasterThreads) void k_contribution_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const uint32_t *__restrict__ final_index, const float4 *__restrict__ out_img, uint32_t *__restrict__ max_bits,
    unsigned long long *__restrict__ counts, uint32_t *__restrict__ mismatch) {
    __shared__ ContribRec lds_all[kTilesPerBlock][kBatch];
    const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    ContribRec *lds = lds_all[q];
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
    uint32_t fin = 0;
    const uint32_t nvis = min(*num_visible, n_splats);
    // a finished forward leaves r0 <= r1 <= min(num_intersections, cap); nothing beyond the list's capacity is read
    const uint32_t r0 = tile_bins[tile_id * 2], r1 = min(tile_bins[tile_id * 2 + 1], cap);
    for (uint32_t batch_start = r0; batch_start < r1 && live != 0ull; batch_start += kBatch) {
        const uint32_t remaining = min(kBatch, r1 - batch_start);
        bool may = false;
        float rec[6];
        uint32_t gid = kInvalid;
        if (lane < remaining) {
            const uint32_t cgid = gid_from_isect[batch_start + lane];
            if (cgid < nvis) {  // every entry of a finished forward's list is
                const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;
#pragma unroll
                for (int k = 0; k < 5; k++) rec[k] = p[k];
                rec[5] = p[8];  // the opacity the splat is drawn with (antialiased mode: already compensated)
                gid = global_from_compact[cgid];
                may = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], bx, by);
            }
        }
        uint64_t mask = ballot64(may);
        if (mask == 0ull) continue;
        wave_sync();  // the previous batch's broadcasts are done (LDS is in order per wave)
        if (may) {
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds[lane].b = make_float4(rec[4], rec[5], __uint_as_float(gid), 0.f);
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
            const bool pass = power <= 0.0f && alpha_u >= 1.0f / 255.0f;  // never true for a stopped pixel (NaN)
            const float alpha = vmin(0.999f, alpha_u);
            const float next_T = T * (1.0f - alpha);
            const bool stop = pass && next_T <= 1e-4f;  // :88-91: stop WITHOUT adding this entry
            const bool hit = pass && !stop;
            const float fac = hit ? alpha * T : 0.0f;
            if (stop) pcx = __builtin_nanf("");
            if (hit) {
                T = next_T;
                fin = batch_start + t;
            }
            const uint64_t hit_mask = ballot64(hit), stop_mask = ballot64(stop);
            if ((hit_mask | stop_mask) != 0ull) {
                const uint32_t fac_max = wave_max_u32(__float_as_uint(fac));  // fac >= 0: its bits order as it does
                const uint32_t q24 = wave_sum((uint32_t)__builtin_rintf(fac * kQ24));
                const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(b.z));
                if (g < n_splats) {
                    if (lane < 3u) {
                        const uint32_t v = lane == 0u   ? q24
                                           : lane == 1u ? (uint32_t)__builtin_popcountll(hit_mask)
                                                        : (uint32_t)__builtin_popcountll(stop_mask);
                        atomicAdd(counts + (size_t)g * 3u + lane, (unsigned long long)v);
                    }
                    if (lane == 0u) atomicMax(max_bits + g, fac_max);
                }
            }
            // all pixels stopped?  one compare every 4th record, as the forward
            if ((++walked & 3u) == 0u) {
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;
                if (live == 0ull) break;
            }
        }
    }
    if (out_img) {
        bool differs = false;
        if (inside) {
            const size_t pix = (size_t)px + (size_t)py * w;
            differs = __float_as_uint(1.0f - T) != __float_as_uint(out_img[pix].w) || fin != final_index[pix];
        }
        const uint32_t bad = (uint32_t)__builtin_popcountll(ballot64(differs));
        if (bad != 0u && lane == 0u) atomicAdd(mismatch, bad);
    }
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_render_contributions(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *out_img,
                                          uint32_t *max_bits, uint64_t *counts, uint32_t *mismatch, uint32_t n,
                                          brush_stream_t stream) {
    if (!h_uniforms || !h_aux || !max_bits || !counts) return BRUSH_ERR_INVALID_ARG;
    if ((out_img != nullptr) != (mismatch != nullptr)) return BRUSH_ERR_INVALID_ARG;
    const BrushUniforms &u = *h_uniforms;
    const BrushAux &aux = *h_aux;
    const uint32_t w = u.img_size[0], h = u.img_size[1], tbx = u.tile_bounds[0], tby = u.tile_bounds[1];
    if (!checked_pixels(w, h) || tbx != ceil_div(w, kTileWidth) || tby != ceil_div(h, kTileWidth))
        return BRUSH_ERR_INVALID_ARG;
    if (!aux.projected_splats || !aux.tile_bins || !aux.compact_gid_from_isect || !aux.global_from_compact_gid ||
        !aux.num_visible || aux.max_intersects == 0 || (out_img && !aux.final_index))
        return BRUSH_ERR_INVALID_ARG;
    if (misaligned(out_img, 16) || misaligned(max_bits, 4) || misaligned(counts, 8) || misaligned(mismatch, 4))
        return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    const uint32_t tiles = tbx * tby;
    // one workgroup (4 quadrant waves) per tile; a multiple of 8 for the XCD remap
    hipLaunchKernelGGL(k_contribution_quad, dim3(ceil_div(tiles, 8u) * 8u), dim3(kRasterThreads), 0,
                       static_cast<hipStream_t>(stream), w, h, tbx, tiles, aux.compact_gid_from_isect, aux.tile_bins,
                       aux.max_intersects, aux.projected_splats, aux.global_from_compact_gid, aux.num_visible, n,
                       aux.final_index, reinterpret_cast<const float4 *>(out_img), max_bits,
                       reinterpret_cast<unsigned long long *>(counts), mismatch);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
