// rasterize_bwd.hip — the backward pass of the per-tile compositing (forward: rasterize.hip; shared: raster_common.hpp).
//
// Replaces:
//   RasterizeBackwards  crates/brush-render/src/shaders/rasterize_backwards.wgsl:140-304
//
// Replaces the reference's LDS gradient queue + nine software CAS loops per queued gradient
// (rasterize_backwards.wgsl:47-135,276-301).  A wave owns NQ = 4, 2 or 1 of the 8x8 quadrants of a tile (one wave per
// tile, per half, per quadrant: backward_quadrants_per_wave), one pixel per lane PER QUADRANT: a lane sums the 9
// gradient components over its quadrants in registers; the 64:1 sums are TRANSPOSED THROUGH LDS (the wave stores its
// partials as rows of 64 words, two lanes per row add half a row each with plain v_add_f32, three records per pass: see
// kStageRecs) because a cross-lane VALU add costs 6 SIMD cycles beside this kernel's arithmetic and a plain one 2.7.  The
// reducing lanes apply the per-record factors and flush with hardware global_atomic_add_f32, consecutive lanes on
// consecutive components of one splat's 64-byte compact row: the L2 executes float atomics line by line.  Records that
// touch no pixel of the tile skip reduction and flush.  (Deterministic mode, NQ = 4 only, keeps the round-2 form: one
// transposing wave64 reduction per record with v_permlane32/16_swap + DPP row sums, rows stored per intersection.)
//
// Roofline: bound by fp32 VALU issue and by the L2's atomic rate, not by HBM; DESIGN.md states the ceilings and the
// measurements.
#include "raster_common.hpp"
#include "raster_zero_fill.hpp"
#include "trace.hpp"

namespace brush {
namespace {

constexpr float kHalfNegLog2e = -0.72134752044448170f;  // 2 sigma -> exp2 argument (backward)

constexpr uint32_t kGradComps = 9;  // v_xy(2) v_conic(3) v_rgb(3) v_opac(1)
constexpr uint32_t kGradCompsDepth = 10;  // ... + v_z (DEPTH), word 9 of the compact row
constexpr uint32_t kDepthRowWord = 10;    // DET + DEPTH: v_z's word of an intersection row (word 9 is the gid)

// Wave64 sum on the VALU with DPP (no LDS traffic, unlike __shfl_xor = ds_bpermute):
// inclusive scan inside each row of 16 (row_shr 1/2/4/8), then row_bcast:15 and row_bcast:31
// carry the row totals up.  The full sum is valid in LANE 63 only.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true);
    return v + __int_as_float(moved);
}
// Row-of-16 inclusive scan: the row total is valid in lane 15 of each row.
__device__ __forceinline__ float row_sum_lane15(float v) {
    v = dpp_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf>(v);  // row_shr:8
    return v;
}
// Transposing pair reductions with the gfx950 lane-swap instructions: one swap + one add fold two
// registers into one in which half of the lanes carry the pair sums of `a`, the other half of `b`.
//   swap32: lanes 0-31 <- a[l] + a[l+32],   lanes 32-63 <- b[l-32] + b[l]
//   swap16: even rows  <- a[row] + a[row+1], odd rows   <- b[row-1] + b[row]
__device__ __forceinline__ float fold_swap32(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float fold_swap16(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float wave_sum_lane63(float v) {
    v = row_sum_lane15(v);
    v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
    v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
    return v;
}

// development / test-only hooks (identity in the product build): dev_vva, dev_flush, dev_skip_reduce, BRUSH_DEV_BWD_TRACE
#define BRUSH_DEV_SECTION 1
#include "rasterize_dev.inc"

// ---- static LDS: one definition ---------------------------------------------------------------------------------------
// A wave's slice of every LDS array of the kernel, as types: the kernel declares arrays of them and bwd_static_lds() adds
// up their sizes for the launcher's occupancy padding, so the two cannot drift apart.

// Staged records of the backward, one array per field (the forward's QuadRec pads the opacity to 16 bytes).
struct BwdRecs {
    float4 a[kBatch];    // mean.x, mean.y, conic.x, conic.y
    float4 b[kBatch];    // conic.z, r, g, b
    float opac[kBatch];
};
typedef uint32_t LdsWords[kBatch];  // one word per staged record: its compact gid; DET: its row position as well
typedef float LdsZ[kBatch];         // DEPTH: z per staged record
// DET: the raw pixel sums of every record of the batch: 9 used (10 with DEPTH); 48-byte rows keep b128 stores aligned
constexpr uint32_t kAccRowWords = 12;
typedef float LdsAcc[kBatch][kAccRowWords];
// Default-mode reduction of the per-record lane partials.  Cross-lane VALU adds (DPP, lane swaps) cost 6 SIMD cycles
// each beside this kernel's arithmetic and a plain v_add_f32 2.7 (tools/ubench/valu_rate.hip), so the 64:1 sums are
// TRANSPOSED through LDS instead: the wave stores the 9 partials of every lane as 9 rows of 64 words (plain LDS stores,
// not VALU work), and once kStageRecs records wait, 2 lanes per row read half a row each (8 ds_read_b128) and add it up
// with plain adds: 31 adds + one lane swap per kStageRecs records instead of 26 cross-lane adds per record.  Rows start
// kRowWords apart so that the 8 lanes the LDS serves per cycle read 8 different groups of 4 banks.
constexpr uint32_t kStageRecs = 3;
constexpr uint32_t kRowWords = 68;
constexpr uint32_t grad_comps(bool depth) { return depth ? kGradCompsDepth : kGradComps; }
template <bool DEPTH>
using LdsStage = float[kStageRecs * grad_comps(DEPTH) * kRowWords];
static_assert(kStageRecs * kGradCompsDepth <= 32, "one row per lane pair");

// Static LDS of one workgroup of k_rasterize_backward_quad<NQ, DET, tpb, Depth...>.  The kernel declares the arrays of
// the other mode with one element and never touches them; the compiler drops those.
template <bool DET, bool DEPTH>
constexpr uint32_t bwd_static_lds(uint32_t tpb = kTilesPerBlock) {
    return tpb * (uint32_t)(sizeof(BwdRecs) + sizeof(LdsWords) +
                            (DET ? sizeof(LdsWords) + sizeof(LdsAcc) : sizeof(LdsStage<DEPTH>)) +
                            (DEPTH ? sizeof(LdsZ) : 0u));
}
// what the kernel descriptors of a build report (tests/test_host_cpu.py holds the build to the same four)
static_assert(sizeof(BwdRecs) == 2304, "two float4 and one float per staged record");
static_assert(bwd_static_lds<false, false>() == 39616 && bwd_static_lds<false, true>() == 43904, "default mode");
static_assert(bwd_static_lds<true, false>() == 23552 && bwd_static_lds<true, true>() == 24576, "deterministic mode");

// ---- phases of the kernel that stand on their own ---------------------------------------------------------------------
// (the others are written out in the kernel, under a comment that names them, or are lambdas that name their captures:
// as functions they changed the kernels' instruction schedule, see DESIGN.md "Where the compositing kernels' source
// lives").  The phases a wave goes through, as the comments in the kernel number them:
//   1  load the pixel state, per quadrant              written out
//   2  stage a batch, with its hit masks               written out
//   3  the per-pixel VJP of one (record, quadrant)     written out in one_record; zero_grads()
//   4  default mode: park and reduce                   park(); the reduce_stage lambda
//   5  deterministic mode: reduce one record           reduce_record_det()
//   6  deterministic mode: row flush (a), zero rows (b)   written out; the zero_rows lambda

// The lane partials of one record start as zeros the compiler cannot see through: every quadrant then accumulates in
// place under its exec mask, instead of each path materialising its own set of nine zero registers.
template <bool DEPTH, uint32_t NC>
__device__ __forceinline__ void zero_grads(float (&g)[NC]) {
    typedef float f2v __attribute__((ext_vector_type(2)));
    f2v z01, z23, z45, z67;
    asm volatile("v_mov_b64 %0, 0" : "=v"(z01));
    asm volatile("v_mov_b64 %0, 0" : "=v"(z23));
    asm volatile("v_mov_b64 %0, 0" : "=v"(z45));
    asm volatile("v_mov_b64 %0, 0" : "=v"(z67));
    g[0] = z01.x, g[1] = z01.y, g[2] = z23.x, g[3] = z23.y;
    g[4] = z45.x, g[5] = z45.y, g[6] = z67.x, g[7] = z67.y;
    asm volatile("v_mov_b32 %0, 0" : "=v"(g[8]));
    if constexpr (DEPTH) asm volatile("v_mov_b32 %0, 0" : "=v"(g[NC - 1]));
}
// Default mode: parks the lane partials of batch slot t as 9 (10) rows of stage slot `staged`: plain LDS stores, no
// cross-lane VALU work.  Slot s of the stage then holds batch slot (staged_t >> 6 s) & 63.
template <uint32_t NC>
__device__ __forceinline__ void park(const float (&g)[NC], uint32_t t, float *stage, uint32_t staged, uint64_t &staged_t,
                                     uint32_t lane) {
    float *dst = stage + staged * (NC * kRowWords) + lane;
#pragma unroll
    for (uint32_t k = 0; k < NC; k++) dst[k * kRowWords] = g[k];
    staged_t |= (uint64_t)t << (6u * staged);
}
// Deterministic mode: one transposing wave64 reduction of the lane partials into the record's row of raw pixel sums.
template <bool DEPTH, uint32_t NC>
__device__ __forceinline__ void reduce_record_det(const float (&g)[NC], float (&acc_row)[kAccRowWords], uint32_t lane) {
    const float u0 = fold_swap32(g[0], g[1]), u1 = fold_swap32(g[2], g[3]);
    const float u2 = fold_swap32(g[4], g[5]), u3 = fold_swap32(g[6], g[7]);
    const float w0 = row_sum_lane15(fold_swap16(u0, u1));
    const float w1 = row_sum_lane15(fold_swap16(u2, u3));
    const float s8 = wave_sum_lane63(g[8]);
    float s9 = 0.0f;
    if constexpr (DEPTH) s9 = wave_sum_lane63(g[NC - 1]);
    if ((lane & 15u) == 15u) {
        const uint32_t r = lane >> 4;
        const uint32_t i0 = ((r & 1u) << 1) | (r >> 1);
        acc_row[i0] = w0;
        acc_row[4 + i0] = w1;
        if (lane == 63) {
            acc_row[8] = s8;
            if constexpr (DEPTH) acc_row[9] = s9;
        }
    }
}

// Footprint-aware backward.  A wave owns NQ quadrants of one tile (NQ = 4: one wave per tile, NQ = 2:
// upper / lower half, NQ = 1: one quadrant), one pixel per lane PER QUADRANT, so a lane's gradient
// contributions of all its quadrants are summed in registers and the 9-component wave reduction runs
// once per (wave, record); quadrants the record cannot reach (quad_may_pass) are skipped by scalar branches.
//
// DET (deterministic mode, NQ = 4 only: one wave per tile, so every intersection has exactly one producer):
// instead of adding to the splat's compact row with float atomics, the wave STORES one 64-byte row per
// intersection, [9 sums | compact gid | 0 ...], at the position the intersection had before the tile sort
// (`unsorted_pos`, grouped by splat); intersections it does not walk get zero rows.  k_sum_isect_rows then adds a
// splat's rows in that fixed order.
//
// DEPTH (brush_render_backward_depth): the accumulated depth is a fourth colour channel whose per-splat value is z
// (compact_depth, staged with the record) and whose pixel gradient is v_depth: z v_D joins the colour term cv of
// v_alpha, KD keeps its start value (the depth behind a record comes in through cv record by record), and a tenth
// component g[9] = sum fac v_D = dL/dz is reduced beside the nine others: word 9 of the compact row (default mode),
// word 10 of the intersection row (DET: word 9 holds the gid).
// The depth instantiation takes one more argument, a DepthGrad.
struct DepthGrad {
    const float *compact_depth;  // [N] z, compact order
    const float *v_depth;        // [h][w]
};
template <uint32_t NQ, bool DET, uint32_t TPB, typename... Depth>
__global__ __launch_bounds__(TPB * kWave) void k_rasterize_backward_quad(
    uint32_t w, uint32_t h, uint32_t tbx, uint32_t num_tiles, const uint32_t *__restrict__ gid_from_isect,
    const uint32_t *__restrict__ tile_bins, const float *__restrict__ projected,
    const uint32_t *__restrict__ final_index, const float *__restrict__ out_img,
    const float *__restrict__ v_out, float *__restrict__ v_compact, const uint32_t *__restrict__ unsorted_pos,
    float *__restrict__ rows, const ZeroFill zf, const Depth... depth) {
    static_assert(!DET || NQ == 4, "deterministic mode: one wave per tile");
    constexpr bool DEPTH = sizeof...(Depth) != 0;
    static_assert(sizeof...(Depth) <= 1, "one DepthGrad");
    constexpr uint32_t NC = grad_comps(DEPTH);
    __shared__ LdsWords lds_pos_all[DET ? TPB : 1];
    __shared__ BwdRecs lds_all[TPB];
    __shared__ LdsWords lds_gid_all[TPB];
    __shared__ LdsAcc acc_all[DET ? TPB : 1];
    __shared__ LdsStage<DEPTH> stage_all[DET ? 1 : TPB];
    __shared__ LdsZ lds_z_all[DEPTH ? TPB : 1];
    // (bwd_static_lds<DET, DEPTH>(TPB) is the sum of those of the six that are used)
    constexpr uint32_t kWavesPerTile = 4u / NQ;
    BRUSH_KTRACE(kTrRasterizeBwd, 0);

    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    BwdRecs &lds = lds_all[wv];
    uint32_t *lds_gid = lds_gid_all[wv];
    uint32_t *lds_pos = lds_pos_all[DET ? wv : 0];
    float(*acc)[kAccRowWords] = acc_all[DET ? wv : 0];
    float *stage = stage_all[DET ? 0 : wv];
    const uint32_t unit = xcd_contiguous_block() * TPB + wv;
    const uint32_t tile_id = unit / kWavesPerTile, sub = unit % kWavesPerTile;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    // Zero-fill in passing (raster_zero_fill.hpp): every launched wave has a share of the block sequence, tile or not,
    // and leaves only once it is stored
    FillCursor fc;
    fill_begin(zf, fc, unit, gridDim.x * TPB);
    auto fill_rest = [&fc, &zf, lane]() {
        while (fc.quota != 0u) fill_step(zf, fc, lane);
    };
    if (tile_id >= num_tiles) return fill_rest();
    const uint32_t r0 = tile_bins[tile_id * 2], r1 = tile_bins[tile_id * 2 + 1];
    BRUSH_DEV_BWD_TRACE(blockIdx.x * TPB + wv, r1 > r0 ? r1 - r0 : 0u);
    if (r1 <= r0) return fill_rest();
    const uint32_t tx0 = (tile_id % tbx) * kTileWidth, ty0 = (tile_id / tbx) * kTileWidth;
    // Phase 6b, deterministic mode: zero rows (carrying their gid) for the intersections [lo, hi) this wave does not walk
    auto zero_rows = [&lane, &rows, &unsorted_pos, &gid_from_isect](uint32_t lo, uint32_t hi) {
        for (uint32_t i = lo + lane; i < hi; i += kWave) {
            float4 *r = reinterpret_cast<float4 *>(rows + (size_t)unsorted_pos[i] * kCompactStride);
            r[0] = r[1] = r[3] = make_float4(0.f, 0.f, 0.f, 0.f);  // the whole 64-byte row
            r[2] = make_float4(0.f, __uint_as_float(gid_from_isect[i]), 0.f, 0.f);
        }
    };

    // ---- phase 1: load the pixel state, per quadrant ----
    // T is the transmittance in front of the current record (the list is walked back to front).  The reference's running
    // colour `buffer` (rasterize_backwards.wgsl:253-257) only ever appears dotted with the pixel's constant v_out.rgb, so
    // the scalar D = sum_j fac_j (c_j . v_rgb) over the records walked so far carries the same information;
    // K = T_final v_out.a is constant.  v_alpha needs only their difference, so the state is KD = K - D: it starts at K
    // and loses fac (c . v_rgb) per record.  Pixels outside the image get fin = -1 and never contribute.
    float pcx[NQ], pcy[NQ], T[NQ], KD[NQ], vor[NQ], vog[NQ], vob[NQ];
    float vod[NQ];  // DEPTH: v_depth
    int32_t fin[NQ];
    int32_t max_fin = -1;
#pragma unroll
    for (uint32_t s = 0; s < NQ; s++) {
        const uint32_t qi = sub * NQ + s;
        const uint32_t px = tx0 + (qi & 1u) * 8u + (lane & 7u), py = ty0 + (qi >> 1) * 8u + (lane >> 3);
        pcx[s] = (float)px + 0.5f;
        pcy[s] = (float)py + 0.5f;
        float T_final = 1.0f;
        float4 vo = make_float4(0.f, 0.f, 0.f, 0.f);
        fin[s] = -1;
        if constexpr (DEPTH) vod[s] = 0.0f;
        if (px < w && py < h) {
            const size_t pix = (size_t)px + (size_t)py * w;
            T_final = 1.0f - out_img[pix * 4 + 3];  // rasterize_backwards.wgsl:163
            fin[s] = (int32_t)final_index[pix];
            vo = reinterpret_cast<const float4 *>(v_out)[pix];
            if constexpr (DEPTH) vod[s] = only(depth...).v_depth[pix];
        }
        T[s] = T_final, KD[s] = T_final * vo.w;
        vor[s] = vo.x, vog[s] = vo.y, vob[s] = vo.z;
        max_fin = max(max_fin, fin[s]);
    }
    // Entries behind the wave's largest final index fail `isect_id <= final_isect` for every pixel
    // (rasterize_backwards.wgsl:229): start the walk there.
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) max_fin = max(max_fin, __shfl_xor(max_fin, d, 64));
    // (wave-uniform by construction; said so, it stays on the scalar unit with everything derived from it)
    const uint32_t walk_end = __builtin_amdgcn_readfirstlane(min(r1, (uint32_t)(max_fin + 1)));
    if (DET) zero_rows(max(walk_end, r0), r1);
    if (walk_end <= r0) return fill_rest();
    // Zero-fill pacing, written out here and in one_record (as functions in raster_zero_fill.hpp it changed the kernels'
    // branch layout).  State: fill_num, fill_den (the walk), fill_budget, fill_rate, fill_acc (the batch).
    // The wave's blocks are spread evenly over the records it walks (`fill_num` blocks per `fill_den` records, an
    // error-diffusion counter on the scalar unit per batch).  Measured (profiles/r04_zero_fill_in_passing.json): the
    // placement inside a wave's life hardly matters at 8160 tiles (all blocks behind the walk: the same within 3 us),
    // a burst at every batch start costs 5 us, and on small frames whose waves all start together only the even
    // spread overlaps at all (1 M splats @512x512: step 0.332 -> 0.316 ms even, 0.328 behind the walk).
    const uint32_t fill_num = fc.quota, fill_den = walk_end - r0;
    uint32_t fill_acc = 0u, fill_budget = 0u, fill_rate = 0u;

    for (uint32_t batch_end = walk_end; batch_end > r0;) {
        const uint32_t remaining = min(kBatch, batch_end - r0);
        // ---- phase 2: stage a batch.  Lane l gathers record batch_end - 1 - l and bounds it against the wave's
        // quadrants: qm[s] = the records that may reach quadrant s, todo = those that may reach any ----
        bool hitq[NQ];
#pragma unroll
        for (uint32_t s = 0; s < NQ; s++) hitq[s] = false;
        float rec[9];
        float zrec = 0.0f;
        uint32_t cg_id = 0;
        if (lane < remaining) {
            cg_id = gid_from_isect[batch_end - 1u - lane];
            const float *p = projected + (size_t)cg_id * BRUSH_PROJECTED_FLOATS;
#pragma unroll
            for (int k = 0; k < 9; k++) rec[k] = p[k];
            if constexpr (DEPTH) zrec = only(depth...).compact_depth[cg_id];
#pragma unroll
            for (uint32_t s = 0; s < NQ; s++) {
                const uint32_t qi = sub * NQ + s;
                hitq[s] = quad_may_pass(rec[0], rec[1], rec[2], rec[3], rec[4], rec[8],
                                        (float)(tx0 + (qi & 1u) * 8u) + 0.5f, (float)(ty0 + (qi >> 1) * 8u) + 0.5f);
            }
        }
        uint64_t qm[NQ], todo = 0ull;
#pragma unroll
        for (uint32_t s = 0; s < NQ; s++) {
            qm[s] = ballot64(hitq[s]);
            todo |= qm[s];
        }
        if (fc.quota != 0u) {
            fill_budget = min(fc.quota, ceil_div(fill_num * remaining, fill_den));
            fill_rate = fill_budget, fill_acc = 0u;
        }
        if (todo == 0ull) {
            if (DET) zero_rows(batch_end - remaining, batch_end);
            fill_take(zf, fc, lane, fill_budget);
            batch_end -= remaining;
            continue;
        }
        wave_sync();  // previous batch fully flushed
        // the records that hit go to LDS; DET keeps every record's gid and row position for the row flush, and clears
        // the batch's sums
        if (DET && lane < remaining) {
            lds_gid[lane] = cg_id;
            lds_pos[lane] = unsorted_pos[batch_end - 1u - lane];
        }
        if ((todo >> lane) & 1ull) {
            lds_gid[lane] = cg_id;
            lds.a[lane] = make_float4(rec[0], rec[1], rec[2], rec[3]);
            lds.b[lane] = make_float4(rec[4], rec[5], rec[6], rec[7]);
            lds.opac[lane] = rec[8];
            if constexpr (DEPTH) lds_z_all[wv][lane] = zrec;
        }
        if (DET) {
            float4 *row = reinterpret_cast<float4 *>(&acc[lane][0]);
            row[0] = row[1] = row[2] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        wave_sync();
        const uint64_t flush_mask = todo;
        // ---- phase 4, default mode: park() and reduce_stage (phase 5, deterministic mode, is reduce_record_det()).  Reads lane, stage, staged_t, the staged opacities and gids;
        // adds to v_compact ----
        // Records whose partial sums wait in `stage` (slot s holds batch slot (staged_t >> 6 s) & 63)
        uint32_t staged = 0u;
        uint64_t staged_t = 0ull;
        // The transposed reduction of the staged records (see kStageRecs): lane (row, half) = (l & 31, l >> 5) adds half
        // of row `row` = (stage slot, component), the halves meet through one lane swap, and the lower lane applies the
        // per-record factor and issues the hardware float atomic: 9 consecutive lanes on the 9 consecutive words of one
        // splat's compact row, as the L2 executes float atomics line by line.
        auto reduce_stage = [&lane, &stage, &staged_t, &lds, &v_compact, &lds_gid](const uint32_t cnt) {
            const uint32_t row = lane & 31u, half = lane >> 5;
            float sum = 0.0f;
            if (row < cnt * NC) {
                const float4 *src = reinterpret_cast<const float4 *>(stage + row * kRowWords + half * 32u);
                float4 v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = src[k];
                float p[8];
#pragma unroll
                for (int k = 0; k < 8; k++) p[k] = (v[k].x + v[k].y) + (v[k].z + v[k].w);
                sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
            }
            sum = fold_swap32(sum, sum);  // every lane: lower + upper half of its row
            if (lane < cnt * NC) {
                const uint32_t slot = DEPTH ? row / NC : (row * 57u) >> 9;  // row / 9 for row < 32
                const uint32_t k = row - slot * NC;
                const uint32_t t = (uint32_t)(staged_t >> (6u * slot)) & 63u;
                // rasterize_backwards.wgsl:256-263: v_xy = -opac (sum vva gx, sum vva gy), v_conic = -opac (S2 / 2, S3,
                // S4 / 2), v_rgb, v_opac = S8
                const float nopac = -lds.opac[t];
                const float scale = k >= 5u ? 1.0f : ((k == 2u || k == 4u) ? 0.5f * nopac : nopac);
                dev_flush(&v_compact[(size_t)lds_gid[t] * kCompactStride + k], sum * scale);  // != 0: one float atomic
            }
        };
        // ---- phases 3 and 4 / 5 for batch slot t (a, b, opac: its staged record).  Reads qm, fin, pcx, pcy, the v_out state;
        // moves T and KD one record forward; takes the zero-fill steps that are due (fc and the pacing state) ----
        auto one_record = [&](const uint32_t t, const float4 a, const float4 b, const float opac) {
            const int32_t isect_id = (int32_t)(batch_end - 1u - t);
            if (fill_budget != 0u) {
                fill_acc += fill_rate;
                while (fill_acc >= remaining && fill_budget != 0u) {
                    fill_step(zf, fc, lane);
                    fill_acc -= remaining, fill_budget--;
                }
            }
            float g[NC];
            zero_grads<DEPTH>(g);
            bool contributed = false;
            // phase 3: the VJP at the lane's pixel of every quadrant the record may reach.  Under the per-pixel `if` the
            // updates are plain (exec-masked) moves, no selects.  sigma is evaluated as 0.5 (dx gx + dy gy) with
            // gx = a dx + b dy, gy = b dx + c dy, which are the v_xy factors of rasterize_backwards.wgsl:260-263 as well.
            // The two modes differ in g[0] / g[1] only.
#pragma unroll
            for (uint32_t s = 0; s < NQ; s++) {
                if (((qm[s] >> t) & 1ull) == 0ull) continue;  // scalar: the record cannot reach quadrant s
                const float dx = a.x - pcx[s], dy = a.y - pcy[s];
                const float gx = fmaf(a.z, dx, a.w * dy);
                const float gy = fmaf(a.w, dx, b.x * dy);
                const float sig2 = fmaf(dx, gx, dy * gy);  // 2 sigma
                const float vis = __builtin_amdgcn_exp2f(sig2 * kHalfNegLog2e);
                const float alpha_u = opac * vis;
                if (isect_id <= fin[s] && sig2 >= 0.0f && alpha_u >= 1.0f / 255.0f) {
                    // rasterize_backwards.wgsl:239-271
                    const float alpha = vmin(0.99f, alpha_u);  // 0.99 here, 0.999 in the forward (:239)
                    const float om = 1.0f - alpha;
                    // v_rcp_f32 is good to 1 ulp and 1 - alpha >= 0.01 (always finite); WGSL's own division is
                    // specified to 2.5 ulp, so no refinement step
                    const float ra = __builtin_amdgcn_rcpf(om);
                    const float Tn = T[s] * ra;
                    const float fac = alpha * Tn;
                    float cv = fmaf(b.w, vob[s], fmaf(b.z, vog[s], b.y * vor[s]));
                    if constexpr (DEPTH) cv = fmaf(lds_z_all[wv][t], vod[s], cv);  // the fourth channel
                    // v_alpha = (c*T - buffer*ra) . v_rgb + T_final*ra*v_a = T (c . v_rgb) + ra (K - D)
                    const float v_alpha = fmaf(Tn, cv, ra * KD[s]);
                    T[s] = Tn;
                    KD[s] = fmaf(-fac, cv, KD[s]);
                    // v_sigma = -opac vis v_alpha; the factors that are the same for every pixel (-opac, the conic
                    // in gx / gy, the 1/2 of the conic terms) are applied once per record at the flush:
                    //   g0 = sum vva dx, g1 = sum vva dy (default mode: vva gx, vva gy), g2..4 = sum vva (dx dx, dx dy,
                    //   dy dy), g8 = sum vva
                    const float vva = dev_vva(vis, v_alpha);  // vis * v_alpha
                    const float wx = vva * dx, wy = vva * dy;
                    if (DET) {
                        g[0] += wx;
                        g[1] += wy;
                    } else {  // the conic factors of v_xy applied per pixel: the flush scales single sums only
                        g[0] = fmaf(vva, gx, g[0]);
                        g[1] = fmaf(vva, gy, g[1]);
                    }
                    g[2] = fmaf(wx, dx, g[2]);
                    g[3] = fmaf(wx, dy, g[3]);
                    g[4] = fmaf(wy, dy, g[4]);
                    g[5] = fmaf(fac, vor[s], g[5]);
                    g[6] = fmaf(fac, vog[s], g[6]);
                    g[7] = fmaf(fac, vob[s], g[7]);
                    g[8] += vva;
                    if constexpr (DEPTH) g[NC - 1] = fmaf(fac, vod[s], g[NC - 1]);
                    contributed = true;
                }
            }
            if (ballot64(contributed) != 0ull) {  // wave-uniform: all 64 lanes take part in the reduction
                if (dev_skip_reduce<DET>(g, v_compact, lane)) return;  // never in the product build
                if constexpr (!DET) {
                    park(g, t, stage, staged, staged_t, lane);
                    if (++staged == kStageRecs) {
                        reduce_stage(kStageRecs);
                        staged = 0u, staged_t = 0ull;
                    }
                    return;
                }
                reduce_record_det<DEPTH>(g, acc[t], lane);
            }
        };
        // The walk over `todo`: a record's LDS row is read one record AHEAD (software pipeline, two register sets in
        // turn), so the broadcast's latency is covered by the previous record's arithmetic instead of stalling the wave.
        {
            uint32_t tA = (uint32_t)__builtin_ctzll(todo), tB = tA;
            float4 aA = lds.a[tA], bA = lds.b[tA], aB, bB;
            float oA = lds.opac[tA], oB;
            for (;;) {
                todo &= todo - 1ull;
                tB = todo != 0ull ? (uint32_t)__builtin_ctzll(todo) : tA;
                aB = lds.a[tB], bB = lds.b[tB], oB = lds.opac[tB];
                one_record(tA, aA, bA, oA);
                if (todo == 0ull) break;
                todo &= todo - 1ull;
                tA = todo != 0ull ? (uint32_t)__builtin_ctzll(todo) : tB;
                aA = lds.a[tA], bA = lds.b[tA], oA = lds.opac[tA];
                one_record(tB, aB, bB, oB);
                if (todo == 0ull) break;
            }
        }
        fill_take(zf, fc, lane, fill_budget);  // (a batch with few hits)
        if constexpr (!DET) {
            if (staged != 0u) reduce_stage(staged);
        } else {
            wave_sync();
            // ---- phase 6a, deterministic mode: flush the batch's rows.  Reads acc, the staged records, gids and positions;
            // stores to rows ----
            // acc holds the raw pixel sums; the per-record factors (rasterize_backwards.wgsl:256-263):
            //   v_xy = -opac (a S0 + b S1, b S0 + c S1), v_conic = -opac (S2 / 2, S3, S4 / 2), v_rgb, v_opac = S8
            auto finish = [&acc, &lds](uint32_t t, uint32_t k) -> float {
                const float v = acc[t][k];
                if (k >= 5u) return v;
                const float4 a = lds.a[t];
                const float nopac = -lds.opac[t];
                if (k >= 2u) return (k == 3u ? nopac : 0.5f * nopac) * v;
                const float other = acc[t][k ^ 1u];
                return nopac * (k == 0u ? fmaf(a.z, v, a.w * other) : fmaf(lds.b[t].x, v, a.w * other));
            };
            // one row per intersection of the batch (zeros where nothing contributed), 16 consecutive lanes per row
            for (uint32_t f = lane; f < remaining * kCompactStride; f += kWave) {
                const uint32_t t = f / kCompactStride, k = f - t * kCompactStride;
                float v = 0.0f;
                if (k < kGradComps) {
                    if ((flush_mask >> t) & 1ull) v = finish(t, k);
                } else if (k == kGradComps) {
                    v = __uint_as_float(lds_gid[t]);
                } else if (DEPTH && k == kDepthRowWord) {
                    if ((flush_mask >> t) & 1ull) v = acc[t][9];
                }
                rows[(size_t)lds_pos[t] * kCompactStride + k] = v;
            }
        }
        batch_end -= remaining;
    }
    fill_rest();
}

}  // namespace

// Lays the given arrays end to end as a sequence of KiB blocks (64 lanes x 16 bytes).
bool make_zero_fill(ZeroFill *zf, float *const *arrays, const size_t *floats, uint32_t count) {
    *zf = ZeroFill{};
    const auto fail = [zf]() { return *zf = ZeroFill{}, false; };  // an inactive fill
    if (count > kFillSegs) return false;
    uint64_t blocks = 0;
    for (uint32_t i = 0; i < kFillSegs; i++) {
        zf->first_block[i] = (uint32_t)blocks;
        if (i >= count || !arrays[i] || floats[i] == 0) continue;
        const uint64_t chunks = floats[i] / 4u;
        if (misaligned(arrays[i], 16) || chunks >= (1ull << 32) - 64u)
            return fail();
        zf->base[i] = arrays[i];
        zf->full[i] = (uint32_t)chunks;
        zf->tail[i] = (uint32_t)(floats[i] & 3u);
        blocks += (chunks + (zf->tail[i] ? 1u : 0u) + kWave - 1u) / kWave;
    }
    if (blocks >= (1ull << 31)) return fail();
    zf->first_block[kFillSegs] = (uint32_t)blocks;
    return true;
}

// Quadrants per wave of the backward: fewer waves per tile mean less repeated per-record work (staging, set-up and
// reduction run once per wave and record), more waves per tile fill the chip when the frame has few tiles.  Thresholds
// from a sweep of frame sizes with the LDS-transposed reduction (backward kernel, us, 1 / 2 / 4 quadrants per wave;
// profiles/r03_bwd_occupancy_schedule_experiment.json): 972 tiles 42 / 48 / 73, 1200: 56 / 46 / 66, 1728: 56 / 47 / 58,
// 2040: 60 / 45 / 48, 2500: 70 / 68 / 66 (dense scene 283 / 177 / 129), 3072: 78 / 59 / 52, 3600: 97 / 61 / 47,
// 4096: 141 / 121 / 112.  (With round 2's reduction the switch to one wave per tile paid only from 6144 tiles.)
static uint32_t backward_quadrants_per_wave(uint32_t tiles) {
    return tiles >= 2304u ? 4u : (tiles >= 1100u ? 2u : 1u);
}

template <uint32_t NQ> using NqC = std::integral_constant<uint32_t, NQ>;

// SIMDs of the current device (queried once per device).
static uint32_t device_simds() {
    static std::atomic<uint32_t> simds_of[kMaxDevices];  // per device (0 = not queried yet)
    const int slot = current_device_slot();
    uint32_t simds = simds_of[slot].load(std::memory_order_relaxed);
    if (simds == 0u || slot == kMaxDevices - 1) {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        simds = (uint32_t)cus * 4u;
        simds_of[slot].store(simds, std::memory_order_relaxed);
    }
    return simds;
}

// Waves per SIMD.  The kernel is bound by VALU issue once a SIMD holds 3+ waves, every wave lives for its whole
// tile and the tiles' lists are about equally long, so the launch proceeds in rounds of (SIMDs x k) waves and a
// partly filled last round costs as much as a full one: k in {3, 4, 5} is chosen to waste the least of the last
// round (1080p: 8160 waves on 1024 SIMDs, k = 4 -> 2 rounds, 152 us; k = 5 -> 1.6 rounds, 164 us; k = 3: 177 us).
// Registers and static LDS allow 4; fewer are enforced with unused dynamic LDS per workgroup.  Workgroups of 4 waves
// (4 tiles in a row): 1, 2 and 8 measured slower (154 / 157 / 172 vs 142 us).
// Returns the dynamic LDS per workgroup that admits exactly k workgroups (of 4 waves) per CU beside `static_lds` bytes
// of static LDS, for `units` waves on `simds` SIMDs.
static uint32_t lds_pad_for(uint32_t units, uint32_t simds, uint32_t static_lds, uint32_t max_k_regs) {
    constexpr uint32_t kLdsPerCu = 160u * 1024u;
    const uint32_t max_k = min(max_k_regs, kLdsPerCu / static_lds);
    uint32_t best_k = max_k, best_cost = 0xFFFFFFFFu;
    for (uint32_t k = max_k; k >= 3u; k--) {
        const uint32_t cost = ceil_div(units, simds * k) * k;  // in wave-rounds per SIMD
        if (cost < best_cost) best_cost = cost, best_k = k;
    }
    if (best_k >= max_k_regs) return 0u;  // the registers stop the (k+1)-th workgroup
    // halfway between "k + 1 fit" and "k fit": sized to the last KB (160 KB / k) the CU admitted one workgroup fewer
    // than intended (per-wave timeline: 2 resident waves per SIMD instead of 3)
    const uint32_t per_wg = ((kLdsPerCu / (best_k + 1u) + kLdsPerCu / best_k) / 2u) & ~1023u;
    return per_wg > static_lds ? per_wg - static_lds : 0u;
}

hipError_t launch_rasterize_backward(const RasterFrame &f, const RasterGrads &g, const ZeroFill &fill, hipStream_t s) {
    const uint32_t tiles = f.tbx * f.tby;
    if (tiles == 0) return hipSuccess;
    if (g.v_depth && !g.compact_depth) return hipErrorInvalidValue;
    float *const rows = g.rows;  // deterministic mode, else nullptr
    // The one launch of k_rasterize_backward_quad<nq, det, kTilesPerBlock, Depth...>: tiles * 4 / nq waves, four to a
    // workgroup, the grid a multiple of 8 workgroups (xcd_contiguous_block).  Registers (kernel_diff.py --resources:
    // 96 / 98 VGPRs at NQ = 1, 104 / 108 at NQ = 2, 124 / 130 at NQ = 4, deterministic 124 / 128; without / with depth)
    // are taken to allow 4 waves per SIMD in every instantiation.
    auto launch = [&](auto nq, auto det, const auto... depth) {
        const uint32_t units = tiles * (4u / nq());
        const uint32_t lds_pad = lds_pad_for(units, device_simds(), bwd_static_lds<det(), sizeof...(depth) != 0>(), 4u);
        hipLaunchKernelGGL((k_rasterize_backward_quad<nq(), det(), kTilesPerBlock, std::decay_t<decltype(depth)>...>),
                           dim3(ceil_div(ceil_div(units, kTilesPerBlock), 8u) * 8u), dim3(kRasterThreads), lds_pad, s, f.w,
                           f.h, f.tbx, tiles, f.compact_gid_from_isect, f.tile_bins, f.projected, f.final_index,
                           g.out_img, g.v_out, g.v_compact, det() ? g.unsorted_pos : nullptr, det() ? rows : nullptr,
                           fill, depth...);
    };
    // deterministic mode (rows): one wave per tile, one stored row per intersection
    auto pick = [&](const auto... depth) {
        const uint32_t nq = rows ? 0u : backward_quadrants_per_wave(tiles);
        if (rows) launch(NqC<4>{}, std::true_type{}, depth...);
        else if (nq == 4) launch(NqC<4>{}, std::false_type{}, depth...);
        else if (nq == 2) launch(NqC<2>{}, std::false_type{}, depth...);
        else launch(NqC<1>{}, std::false_type{}, depth...);
    };
    // depth as a fourth channel: one more staged float per record, 10-component stage rows
    g.v_depth ? pick(DepthGrad{g.compact_depth, g.v_depth}) : pick();
    return hipGetLastError();
}

}  // namespace brush

#define BRUSH_DEV_SECTION 2
#include "rasterize_dev.inc"
