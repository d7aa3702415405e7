// replay_walk.hpp — the compositing replay: one walk over the tile lists a FINISHED forward left in its aux, run by
// k_contribution_quad, k_error_quad, k_median_depth_quad and k_feature_grad_quad, and what every replay kernel
// (k_feature_quad too, which keeps its walk written out) shares beside it: the staged record, the quadrant prologue, the
// fixed point of the sums and the host-side checks and launch geometry of the six entries.  What the walk shares with
// the compositing kernels themselves is raster_common.hpp.
//
// The walk is the forward's (k_rasterize_quad, float image; rasterize.wgsl:57-101) with the same expressions per pixel:
// sigma, power, alpha_u, the 0.999 clamp, the test `power <= 0 && alpha_u >= 1/255`, next_T, the `next_T <= 1e-4` stop
// WITHOUT adding the entry and the NaN pixel centre after a stop, so that T evolves as it did in the forward.  It walks
// until no pixel of the wave is live or the list ends, not up to final_index: it must see the entry that stops a pixel.
//
// gfx950 layout: the forward's.  One wave64 per 8x8 quadrant, four waves per tile, the XCD-contiguous block remap,
// records staged per wave in LDS in batches of 64 and read back as wave-uniform broadcasts, quad_may_pass() skipping a
// (record, quadrant) on the scalar unit, no s_barrier, no LDS atomics.
#pragma once
#include "raster_common.hpp"

namespace brush {
namespace {

constexpr float kQ24 = 16777216.0f;  // the fixed point of the summed weights and products: 2^24

// One staged record's geometry: 32 bytes, read back as wave-uniform broadcasts.
struct ReplayRec {
    float4 a;  // mean.x, mean.y, conic.x, conic.y
    float4 b;  // conic.z, opacity, and two words of the kernel's own
};
// static LDS of a workgroup: what the kernel descriptor of a build reports (tests/test_*_cpu.py)
static_assert(sizeof(ReplayRec) * kTilesPerBlock * kBatch == 8192, "one ReplayRec per wave and batch slot");

// The quadrant and pixel prologue, from the kernel parameters w, h, tbx and num_tiles.  A macro: the two early exits
// have to be `return`s of the kernel body itself (a helper that reports them as a bool compiles to other scalar code).
#define BRUSH_REPLAY_PROLOGUE(REC)                                                                                      \
    __shared__ REC lds_all[kTilesPerBlock][kBatch];                                                                     \
    const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);                                             \
    REC *lds = lds_all[q];                                                                                              \
    const uint32_t tile_id = xcd_contiguous_block();                                                                    \
    if (tile_id >= num_tiles) return;                                                                                   \
    const uint32_t lane = threadIdx.x & (kWave - 1);                                                                    \
    const uint32_t qx0 = (tile_id % tbx) * kTileWidth + (q & 1u) * 8u, qy0 = (tile_id / tbx) * kTileWidth + (q >> 1) * 8u; \
    if (qx0 >= w || qy0 >= h) return; /* quadrant entirely outside a ragged frame */                                    \
    const uint32_t px = qx0 + (lane & 7u), py = qy0 + (lane >> 3);                                                      \
    const float bx = (float)qx0 + 0.5f, by = (float)qy0 + 0.5f;                                                         \
    const bool inside = px < w && py < h;                                                                               \
    const float pcy = (float)py + 0.5f; /* rasterize.wgsl:32 */                                                         \
    float pcx = inside ? (float)px + 0.5f : __builtin_nanf("")

// The walk of one quadrant wave, after BRUSH_REPLAY_PROLOGUE, around the kernel's own code per walked (record,
// quadrant).  Macros, like the prologue: a function template with hooks compiled every kernel to other machine code than
// the written-out walk (equal descriptors, other instruction order, one instantiation measurably slower); this form
// gives the same bytes.  It reads the kernel parameters gid_from_isect, tile_bins, cap, projected, global_from_compact,
// num_visible and n_splats.
//   BRUSH_REPLAY_WALK_STATE  the walk's state, declared behind the kernel's own loads and in front of its accumulators:
//     T, 1 at the start and the pixel's final T at the end
//   BRUSH_REPLAY_WALK_BEGIN(READS_LISTS, REC_WORDS, OWN_LOAD, b.z, b.w)  the batch loop, the staging and the hand-off,
//     and per walked (record, quadrant) the forward's arithmetic
//     READS_LISTS  false reads no list at all (n_splats == 0 in a kernel whose entry launches on it)
//     REC_WORDS    6, or 7 when OWN_LOAD, a statement of the staging lane next to the loads of the geometry, fills
//                  rec[6] from cgid
//     b.z, b.w     the record's two own words, from rec[6] and gid
//   It leaves, for the kernel's code: b (the record's second half), batch_start + t (its place in the list), T (the
//   transmittance the entry meets), alpha, next_T and
//     hit  : the forward added the entry
//     stop : the entry passed the alpha test and ended the pixel WITHOUT being added (rasterize.wgsl:88-91)
//   BRUSH_REPLAY_WALK_DIE(ALSO_DIES)  a stopped pixel, and one for which ALSO_DIES holds, takes a NaN centre, which
//     fails every later alpha test: it counts as not live
//   BRUSH_REPLAY_WALK_ADD(what the kernel records with it)  T becomes next_T on a hit
//   BRUSH_REPLAY_WALK_END  the liveness check every fourth record, and the end of both loops
#define BRUSH_REPLAY_WALK_STATE                                                                                         \
    const uint64_t inside_mask = ballot64(inside);                                                                      \
    uint64_t live = inside_mask;                                                                                        \
    uint32_t walked = 0;                                                                                                \
    float T = 1.0f

#define BRUSH_REPLAY_WALK_BEGIN(READS_LISTS, REC_WORDS, OWN_LOAD, ...)                                                     \
    uint32_t nvis = 0, r0 = 0, r1 = 0;                                                                                     \
    if (READS_LISTS) {                                                                                                     \
        nvis = min(*num_visible, n_splats);                                                                                \
        /* a finished forward leaves r0 <= r1 <= min(num_intersections, cap); nothing beyond the capacity is read */       \
        r0 = tile_bins[tile_id * 2];                                                                                       \
        r1 = min(tile_bins[tile_id * 2 + 1], cap);                                                                         \
    }                                                                                                                      \
    for (uint32_t batch_start = r0; batch_start < r1 && live != 0ull; batch_start += kBatch) {                             \
        const uint32_t remaining = min(kBatch, r1 - batch_start);                                                          \
        bool may = false;                                                                                                  \
        float rec[REC_WORDS];                                                                                              \
        uint32_t gid = kInvalid;                                                                                           \
        if (lane < remaining) {                                                                                            \
            const uint32_t cgid = gid_from_isect[batch_start + lane];                                                      \
            if (cgid < nvis) { /* every entry of a finished forward's list is */                                           \
                const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;                                        \
                _Pragma("unroll") for (int k = 0; k < 5; k++) rec[k] = p[k];                                               \
                rec[5] = p[8]; /* the opacity the splat is drawn with (antialiased mode: already compensated) */           \
                OWN_LOAD;                                                                                                  \
                gid = global_from_compact[cgid];                                                                           \
                may = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], bx, by);                               \
            }                                                                                                              \
        }                                                                                                                  \
        uint64_t mask = ballot64(may);                                                                                     \
        if (mask == 0ull) continue;                                                                                        \
        wave_sync(); /* the previous batch's broadcasts are done (LDS is in order per wave) */                             \
        if (may) {                                                                                                         \
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);                                                     \
            lds[lane].b = make_float4(rec[4], rec[5], __VA_ARGS__);                                                        \
        }                                                                                                                  \
        wave_sync();                                                                                                       \
        while (mask != 0ull) {                                                                                             \
            const uint32_t t = (uint32_t)__builtin_ctzll(mask);                                                            \
            mask &= mask - 1ull;                                                                                           \
            const float4 a = lds[t].a;                                                                                     \
            const float4 b = lds[t].b;                                                                                     \
            const float opac = b.y;                                                                                        \
            /* rasterize.wgsl:80-99, the forward's association (rasterize.hip) */                                          \
            const float dx = a.x - pcx, dy = a.y - pcy;                                                                    \
            const float sigma = fmaf(0.5f, fmaf(a.z * dx, dx, (b.x * dy) * dy), (a.w * dy) * dx);                          \
            const float power = sigma * kNegLog2e;                                                                         \
            const float alpha_u = opac * __builtin_amdgcn_exp2f(power);                                                    \
            const bool pass = power <= 0.0f && alpha_u >= 1.0f / 255.0f; /* never true for a dead pixel (NaN) */           \
            const float alpha = vmin(0.999f, alpha_u);                                                                     \
            const float next_T = T * (1.0f - alpha);                                                                       \
            const bool stop = pass && next_T <= 1e-4f; /* :88-91: stop WITHOUT adding this entry */                        \
            const bool hit = pass && !stop;

#define BRUSH_REPLAY_WALK_ADD(...) if (hit) { T = next_T; __VA_ARGS__; }
#define BRUSH_REPLAY_WALK_DIE(ALSO_DIES) if (stop || (ALSO_DIES)) pcx = __builtin_nanf("");

#define BRUSH_REPLAY_WALK_END                                                                                              \
            /* no pixel live?  one compare every 4th record, as the forward */                                             \
            if ((++walked & 3u) == 0u) {                                                                                   \
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;                                   \
                if (live == 0ull) break;                                                                                   \
            }                                                                                                              \
        }                                                                                                                  \
    }

// ---- host side ----------------------------------------------------------------------------------------------------------
struct WalkArgs {
    uint32_t w, h, tbx, tiles, n;
    const BrushAux *aux;
    hipStream_t s;
};

// The checks every replay entry makes of its uniforms and aux (final_index, channel counts and alignments are the
// entries' own).
inline bool walk_args(const BrushUniforms *h_uniforms, const BrushAux *h_aux, uint32_t n, brush_stream_t stream,
                      WalkArgs &o) {
    if (!h_uniforms || !h_aux) return false;
    const BrushUniforms &u = *h_uniforms;
    const BrushAux &aux = *h_aux;
    const uint32_t w = u.img_size[0], h = u.img_size[1], tbx = u.tile_bounds[0], tby = u.tile_bounds[1];
    if (!checked_pixels(w, h) || tbx != ceil_div(w, kTileWidth) || tby != ceil_div(h, kTileWidth)) return false;
    if (!aux.projected_splats || !aux.tile_bins || !aux.compact_gid_from_isect || !aux.global_from_compact_gid ||
        !aux.num_visible || aux.max_intersects == 0)
        return false;
    o = WalkArgs{w, h, tbx, tbx * tby, n, h_aux, static_cast<hipStream_t>(stream)};
    return true;
}

// One workgroup (4 quadrant waves) per tile, a multiple of 8 for the XCD remap; the walk's eleven arguments, then the
// kernel's own.
template <typename Kernel, typename... Own>
void walk_launch(Kernel kernel, const WalkArgs &a, Own... own) {
    const BrushAux &x = *a.aux;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(a.tiles, 8u) * 8u), dim3(kRasterThreads), 0, a.s, a.w, a.h, a.tbx, a.tiles,
                       x.compact_gid_from_isect, x.tile_bins, x.max_intersects, x.projected_splats,
                       x.global_from_compact_gid, x.num_visible, a.n, own...);
}

}  // namespace
}  // namespace brush
