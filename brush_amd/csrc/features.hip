// features.hip — per-splat feature vectors through the compositing walk, both ways (gsplat's N-channel rasterisation is
// the model; the reference renders colour only).  Three entries (include/brush_hip.h), all replays of a FINISHED
// forward's walk over the tile lists it left in the aux:
//   brush_render_features           k_feature_quad<CP>: out[p,c] = sum over the entries the forward added to pixel p of
//                                   fac f[g,c], fac = alpha T, in list order, on the forward's own association
//                                   (rasterize.hip: c = fmaf(colour, fac, c)).
//   brush_render_features_backward  k_feature_grad_quad<CP, kGradF32>: the transpose, v_f[g,c] += sum_p fac v[p,c], with
//                                   hardware float atomics.  ORDER DEPENDENT in its last bits: the partial sums of a
//                                   row arrive in the order the waves reach them.
//   brush_render_feature_sums       k_feature_grad_quad<CP, kSumsF32 | kSumsLabelU8>: the exact transpose of a map in
//                                   [0, 1], sums[g,c] += sum_p (uint32) rint((fac m[p,c]) 2^24), the generalisation of
//                                   k_error_quad (error_score.hip): 64-bit integer adds, order independent, bitwise
//                                   repeatable in both aux modes.  The map is an f32 image or a u8 label image whose
//                                   channel c is `label == c`.
//
// gfx950 layout: the walk's (replay_walk.hpp).  Channels go in passes of CP = 4, 8 or 16 (one launch per pass, the entry
// picks the widths): the pass's accumulators (forward) or pixel values (transpose) live in VGPRs.  The forward's staged
// record grows by the pass's feature slice, gathered by the lane that stages the record; the transpose reduces the
// pass's CP products over the wave with the transposing tree of transpose_sum.hpp (permlane32_swap, permlane16_swap, DPP
// row rotates) that leaves channel c in lane c, and one no-return atomic instruction with the pass's lanes active on
// consecutive words of the splat's row sends them: the L2 executes a contiguous segment at full rate.
#include "replay_walk.hpp"
#include "transpose_sum.hpp"

namespace brush {
namespace {

// One staged record of the forward replay: the walk's 32 bytes of geometry (its own two words unused) and the pass's CP
// features.  The transpose stages the plain ReplayRec with the global id in b.z, through the shared walk.
template <int CP>
struct FeatRec : ReplayRec {
    float4 f[CP / 4];
};
static_assert(sizeof(FeatRec<16>) * kTilesPerBlock * kBatch == 24576, "the widest pass: 24 KB of LDS per workgroup");

// ---- k_feature_quad ---------------------------------------------------------------------------------------------------
// The walk of replay_walk.hpp, written out: the staged record grows by the feature slice and a splat can be vetoed.
// Per added entry and channel k of the pass, acc[k] = fmaf(features[g, c0 + k], fac, acc[k]) under the pixel's own predicate, as
// the forward accumulates its colour.  Every inside pixel stores out[p, c0 .. c0 + cn) once (zeros where nothing was
// added); nothing outside a ragged frame is read or written.  VEC: C is a multiple of 4 and both bases are 16-byte
// aligned, so slices move as float4.
template <int CP, bool VEC>
__global__ __launch_bounds__(kRasterThreads) void k_feature_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const float *__restrict__ features, uint32_t C, uint32_t c0, uint32_t cn, float *__restrict__ out) {
    BRUSH_REPLAY_PROLOGUE(FeatRec<CP>);
    BRUSH_REPLAY_WALK_STATE;
    float acc[CP];
#pragma unroll
    for (int k = 0; k < CP; k++) acc[k] = 0.0f;
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
        float rec[6];
        float4 f[CP / 4];
#pragma unroll
        for (int k = 0; k < CP / 4; k++) f[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < remaining) {
            const uint32_t cgid = gid_from_isect[batch_start + lane];
            if (cgid < nvis) {  // every entry of a finished forward's list is
                const float *p = projected + (size_t)cgid * BRUSH_PROJECTED_FLOATS;
#pragma unroll
                for (int k = 0; k < 5; k++) rec[k] = p[k];
                rec[5] = p[8];  // the opacity the splat is drawn with (antialiased mode: already compensated)
                const uint32_t gid = global_from_compact[cgid];
                may = gid < n_splats && quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], bx, by);
                if (may) {  // the record's slice of its feature row, with the record
                    const float *row = features + (size_t)gid * C + c0;
                    if constexpr (VEC) {
#pragma unroll
                        for (int k = 0; k < CP / 4; k++)
                            if ((uint32_t)(4 * k) < cn) f[k] = reinterpret_cast<const float4 *>(row)[k];
                    } else {
                        float s[CP];
#pragma unroll
                        for (int k = 0; k < CP; k++) s[k] = (uint32_t)k < cn ? row[k] : 0.0f;
#pragma unroll
                        for (int k = 0; k < CP / 4; k++) f[k] = make_float4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
                    }
                }
            }
        }
        uint64_t mask = ballot64(may);
        if (mask == 0ull) continue;
        wave_sync();  // the previous batch's broadcasts are done (LDS is in order per wave)
        if (may) {
            lds[lane].a = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds[lane].b = make_float4(rec[4], rec[5], 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < CP / 4; k++) lds[lane].f[k] = f[k];
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
            if (power <= 0.0f && alpha_u >= 1.0f / 255.0f) {  // never true for a stopped pixel (NaN)
                const float alpha = vmin(0.999f, alpha_u);
                const float next_T = T * (1.0f - alpha);
                if (next_T <= 1e-4f) {  // :88-91: stop WITHOUT adding this entry
                    pcx = __builtin_nanf("");
                } else {
                    const float fac = alpha * T;
#pragma unroll
                    for (int k = 0; k < CP / 4; k++) {
                        const float4 fk = lds[t].f[k];
                        acc[4 * k] = fmaf(fk.x, fac, acc[4 * k]);
                        acc[4 * k + 1] = fmaf(fk.y, fac, acc[4 * k + 1]);
                        acc[4 * k + 2] = fmaf(fk.z, fac, acc[4 * k + 2]);
                        acc[4 * k + 3] = fmaf(fk.w, fac, acc[4 * k + 3]);
                    }
                    T = next_T;
                }
            }
            // all pixels stopped?  one compare every 4th record, as the forward
            if ((++walked & 3u) == 0u) {
                live = ~__builtin_amdgcn_fcmp(pcx, pcx, 8 /* FCMP_UNO */) & inside_mask;
                if (live == 0ull) break;
            }
        }
    }
    if (inside) {
        // w h < 2^28 and C <= 64: the element index needs 64 bits
        float *dst = out + ((size_t)py * w + px) * C + c0;
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < CP / 4; k++)
                if ((uint32_t)(4 * k) < cn)
                    reinterpret_cast<float4 *>(dst)[k] = make_float4(acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < CP; k++)
                if ((uint32_t)k < cn) dst[k] = acc[k];
        }
    }
}

// ---- k_feature_grad_quad ------------------------------------------------------------------------------------------------
enum : int { kGradF32 = 0, kSumsF32 = 1, kSumsLabelU8 = 2 };

// The same walk (replay_walk.hpp).  Per lane, once, in front of the walk: the pixel's CP values of the pass (0 outside
// a ragged frame and past cn):
//   kGradF32      v[k] = map[p, c0 + k], arbitrary
//   kSumsF32      v[k] = min(max(map[p, c0 + k], 0), 1): a NaN and every negative value are 0, everything above 1 is 1
//   kSumsLabelU8  v[k] = labels[p] == c0 + k ? 1 : 0   (a label >= C belongs to no class)
// Per walked (record, quadrant) with the entry added in any lane, with fac = alpha T where it was added, the row
// g = global_from_compact_gid[cgid] receives, from lane c < cn and when the sum is not zero,
//   kGradF32      dst_f[g, c0 + c] += wave sum of fac v[c]                     (one no-return float atomic)
//   otherwise     dst_q[g, c0 + c] += wave sum of (uint32) rint((fac v[c]) 2^24)   (one no-return 64-bit integer add;
//                 ties to even; at most 64 2^24 per record)
template <int CP, int MODE>
__global__ __launch_bounds__(kRasterThreads) void k_feature_grad_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, uint32_t cap, const float *__restrict__ projected,
    const uint32_t *__restrict__ global_from_compact, const uint32_t *__restrict__ num_visible, uint32_t n_splats,
    const void *__restrict__ map, uint32_t C, uint32_t c0, uint32_t cn, float *__restrict__ dst_f,
    unsigned long long *__restrict__ dst_q) {
    BRUSH_REPLAY_PROLOGUE(ReplayRec);
    float v[CP];
#pragma unroll
    for (int k = 0; k < CP; k++) v[k] = 0.0f;
    if (inside) {
        const size_t pix = (size_t)py * w + px;  // the maps' row pitch is w, not the tile-padded width
        if constexpr (MODE == kSumsLabelU8) {
            const uint32_t lab = static_cast<const uint8_t *>(map)[pix];
#pragma unroll
            for (int k = 0; k < CP; k++) v[k] = ((uint32_t)k < cn && lab == c0 + (uint32_t)k) ? 1.0f : 0.0f;
        } else {
            const float *src = static_cast<const float *>(map) + pix * C + c0;
            if ((C & 3u) == 0u && !misaligned(map, 16)) {  // wave-uniform
#pragma unroll
                for (int k = 0; k < CP / 4; k++)
                    if ((uint32_t)(4 * k) < cn) {
                        const float4 m = reinterpret_cast<const float4 *>(src)[k];
                        v[4 * k] = m.x, v[4 * k + 1] = m.y, v[4 * k + 2] = m.z, v[4 * k + 3] = m.w;
                    }
            } else {
#pragma unroll
                for (int k = 0; k < CP; k++)
                    if ((uint32_t)k < cn) v[k] = src[k];
            }
            if constexpr (MODE == kSumsF32) {
#pragma unroll
                for (int k = 0; k < CP; k++) v[k] = fminf(fmaxf(v[k], 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
            }
        }
    }

    BRUSH_REPLAY_WALK_STATE;
    BRUSH_REPLAY_WALK_BEGIN(true, 6, (void)0, __uint_as_float(gid), 0.f)
    const float fac = hit ? alpha * T : 0.0f;
    BRUSH_REPLAY_WALK_DIE(false)
    BRUSH_REPLAY_WALK_ADD()
    if (ballot64(hit) != 0ull) {
        const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(b.z));
        if constexpr (MODE == kGradF32) {
            float p[CP];
#pragma unroll
            for (int k = 0; k < CP; k++) p[k] = hit ? fac * v[k] : 0.0f;  // (0 inf = NaN stays out of other rows)
            const float s = transpose_sum<CP>(p, lane);
            if (lane < cn && g < n_splats && s != 0.0f) unsafeAtomicAdd(dst_f + (size_t)g * C + c0 + lane, s);
        } else {
            uint32_t p[CP];
            // fac v: one f32 rounding; the scale by 2^24 is exact (fac v <= 1)
#pragma unroll
            for (int k = 0; k < CP; k++) p[k] = (uint32_t)__builtin_rintf((fac * v[k]) * kQ24);
            const uint32_t s = transpose_sum<CP>(p, lane);
            if (lane < cn && g < n_splats && s != 0u) atomicAdd(dst_q + (size_t)g * C + c0 + lane, (unsigned long long)s);
        }
    }
    BRUSH_REPLAY_WALK_END
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
// The channel-count bound of the three entries, then the checks every replay entry makes.
bool feature_args(const BrushUniforms *h_uniforms, const BrushAux *h_aux, uint32_t C, uint32_t n, brush_stream_t stream,
                  WalkArgs &o) {
    return C >= 1u && C <= BRUSH_FEATURE_MAX_CHANNELS && walk_args(h_uniforms, h_aux, n, stream, o);
}

// Width of the pass that starts with `rem` channels left: 16 while more than 8 remain, then 8, then 4.
uint32_t pass_width(uint32_t rem) { return rem > 8u ? 16u : rem > 4u ? 8u : 4u; }

template <int CP>
void launch_forward(const WalkArgs &a, const float *features, uint32_t C, uint32_t c0, uint32_t cn, float *out) {
    const bool vec = (C & 3u) == 0u && !misaligned(features, 16) && !misaligned(out, 16);
    walk_launch(vec ? k_feature_quad<CP, true> : k_feature_quad<CP, false>, a, features, C, c0, cn, out);
}

template <int CP, int MODE>
void launch_grad(const WalkArgs &a, const void *map, uint32_t C, uint32_t c0, uint32_t cn, float *dst_f,
                 uint64_t *dst_q) {
    walk_launch(k_feature_grad_quad<CP, MODE>, a, map, C, c0, cn, dst_f, reinterpret_cast<unsigned long long *>(dst_q));
}

template <int MODE>
void grad_passes(const WalkArgs &a, const void *map, uint32_t C, float *dst_f, uint64_t *dst_q) {
    for (uint32_t c0 = 0; c0 < C;) {
        const uint32_t cp = pass_width(C - c0), cn = min(C - c0, cp);
        if (cp == 16u) launch_grad<16, MODE>(a, map, C, c0, cn, dst_f, dst_q);
        else if (cp == 8u) launch_grad<8, MODE>(a, map, C, c0, cn, dst_f, dst_q);
        else launch_grad<4, MODE>(a, map, C, c0, cn, dst_f, dst_q);
        c0 += cn;
    }
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_render_features(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *features,
                                     uint32_t C, float *out, uint32_t n, brush_stream_t stream) {
    WalkArgs a;
    if (!out || (!features && n != 0) || !feature_args(h_uniforms, h_aux, C, n, stream, a)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(features, 4) || misaligned(out, 4)) return BRUSH_ERR_INVALID_ARG;
    // n == 0 launches too: every pixel is written on every call (no list is read then)
    for (uint32_t c0 = 0; c0 < C;) {
        const uint32_t cp = pass_width(C - c0), cn = min(C - c0, cp);
        if (cp == 16u) launch_forward<16>(a, features, C, c0, cn, out);
        else if (cp == 8u) launch_forward<8>(a, features, C, c0, cn, out);
        else launch_forward<4>(a, features, C, c0, cn, out);
        c0 += cn;
    }
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_render_features_backward(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const float *v_out,
                                              uint32_t C, float *v_features, uint32_t n, brush_stream_t stream) {
    WalkArgs a;
    if (!v_out || !v_features || !feature_args(h_uniforms, h_aux, C, n, stream, a)) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(v_out, 4) || misaligned(v_features, 4)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    grad_passes<kGradF32>(a, v_out, C, v_features, nullptr);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_render_feature_sums(const BrushUniforms *h_uniforms, const BrushAux *h_aux, const void *maps,
                                         uint32_t map_kind, uint32_t C, uint64_t *sums, uint32_t n,
                                         brush_stream_t stream) {
    WalkArgs a;
    if (!maps || !sums || map_kind > BRUSH_FEATURE_MAP_LABEL_U8 || !feature_args(h_uniforms, h_aux, C, n, stream, a))
        return BRUSH_ERR_INVALID_ARG;
    if ((map_kind == BRUSH_FEATURE_MAP_F32 && misaligned(maps, 4)) || misaligned(sums, 8)) return BRUSH_ERR_INVALID_ARG;
    if (n == 0) return BRUSH_OK;  // no splat, no row
    if (map_kind == BRUSH_FEATURE_MAP_F32) grad_passes<kSumsF32>(a, maps, C, nullptr, sums);
    else grad_passes<kSumsLabelU8>(a, maps, C, nullptr, sums);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}
