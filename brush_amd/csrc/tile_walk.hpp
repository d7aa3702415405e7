// tile_walk.hpp — what the two tile passes share: the walk policy, the device work queue, the two-phase tile test and
// the rebuild of a splat's walk rectangle.  Included by tile_count.hip (which tiles does a splat touch, and how many)
// and tile_emit.hip (write them out); both are compiled with -ffp-contract=off, see project.hip.
//
// The contract between the passes.  The count pass (k_project_visible, k_walk_count) runs the exact tile test once per
// candidate tile and records WHICH tiles passed; the emit pass (k_map_intersects) replays that record and never
// repeats the test.  Per visible splat c the count pass leaves slot_of[c]: kInlineFlag for a splat walked inside
// k_project_visible, whose hit mask (bit i = tile i of its rectangle, row-major) is inline_mask[c]; the first queue
// slot (< 2^31) for a splat cut into chunks of kChunkTiles tiles, one queue item (c, k) per chunk in consecutive
// slots; kInlineRetest for a splat that did not fit into the queue, which both passes walk serially.  Per queue item
// it leaves chunk_mask (the chunk's hit mask) and chunk_count, the inclusive running hit count inside the item's group
// of walk_group(n) items.  The emit pass reads slot_of, inline_mask, items, chunk_mask and chunk_count back, together
// with the scan of tiles_hit: a splat's entries go to [cum[c-1], cum[c]) in row-major order of its rectangle, and a
// chunk's offset inside that range is a difference of chunk_counts.  Both passes take walk_group from the same item
// count, and both derive the rectangle from the same record bits through walk_rect (splat_math.hpp), so bit i names
// the same tile on both sides.
//
// No dispatch buffer (crates/brush-kernel/src/shaders/wg.wgsl:15-40 in the reference): the kernels read the
// device-side counts themselves and grid-stride.
#pragma once
#include "internal.hpp"
#include "splat_math.hpp"

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
// Tile walks.  A splat's bbox holds 1 .. tiles_x*tiles_y candidate tiles and the exact
// can_be_visible test costs ~300 VALU instructions, so the walk is split by size:
//   * bboxes of <= kSmallArea (16) tiles are walked inside project_visible, but not lane by lane:
//     the candidate tiles of the wave's 64 splats are flattened into one list (wave prefix sum of
//     the bbox areas), every lane tests one candidate per step after finding its owner splat with
//     a 6-step shuffle binary search, and each owner harvests its hit bits from the step's ballot
//     (count + 64-bit hit mask).  All lanes do useful tests regardless of how uneven the areas are;
//   * larger ones are cut into chunks of kChunkTiles (64) tiles and queued as (splat, chunk) work items
//     (one atomicAdd per workgroup reserves consecutive slots).  A second launch consumes the queue
//     walk_group(n) = 4, 16 or 64 items per wave (the lanes fetch the items' geometry in one memory phase,
//     then one 64-tile step per item), so a whole-screen splat is spread over many waves.
// If the queue is full the lane falls back to walking its bbox inline (slow, still correct).
// The hit masks are kept so that the emission pass never repeats the exact test.
constexpr uint32_t kSmallArea = 16;      // few visible splats (latency-bound launch): short inline walks
constexpr uint32_t kSmallAreaMany = 64;  // many visible splats (throughput-bound): everything one hit mask can hold
// Visible-splat count above which kSmallAreaMany applies (S3, 2 M visible: 470 -> 259 us; at 100 k visible the short
// inline walks win: 28.5 vs 50.4 us).  launch_project_visible passes it as a kernel argument.
constexpr uint32_t kSmallAreaSwitch = 1u << 19;
constexpr uint32_t kHalfWaveSplats = 1u << 18;  // up to this many visible splats a ProjectVisible wave takes 32 of them
constexpr uint32_t kChunkTiles = 64;   // one 64-bit hit mask per queue item
constexpr uint32_t kWalkGroupMax = 64;  // queue items a consumer wave takes at a time when the queue is very long
constexpr uint32_t kFlatEmitMin = 1u << 19;  // visible splats from which the inline emission is flattened (tile_emit.hip)
// Few items: small groups (more waves, shorter serial chains); many items: amortise the memory phase and the per-item
// set-up (record gather, log / sqrt / divisions of the tile test and the walk rectangle: ~300 instructions that only
// the group's lanes execute, so a group of 16 runs them at a quarter of the wave).
__device__ __forceinline__ uint32_t walk_group(uint32_t n_items) {
    return n_items <= 16384u ? 4u : (n_items <= (1u << 18) ? 16u : kWalkGroupMax);
}

// Device view of WalkWs (internal.hpp).  The struct's name is part of four kernels' mangled names.
struct WalkQueue {
    uint32_t *counter;      // [1] items reserved so far (zeroed by the cull kernel)
    uint2 *items;           // [capacity] (compact gid, chunk index)
    uint32_t *chunk_count;  // [capacity] tiles hit inside the chunks up to and including this one, counted from the
                            //     start of the item's group of walk_group(n) items (group-local inclusive prefix)
    uint64_t *chunk_mask;   // [capacity] hit bitmask of the chunk's 64 tiles (count pass -> emit pass)
    uint32_t *slot_of;      // [N] queued splat: first item slot (< 2^31); inline splat: kInlineFlag
                            //     (hit mask in inline_mask) or kInlineRetest
    uint64_t *inline_mask;  // [N] hit mask of an inline splat's <= 64 bbox tiles (row-major)
    uint32_t capacity;
};
constexpr uint32_t kInlineFlag = 0x80000000u;
constexpr uint32_t kInlineRetest = 0xFFFFFFFFu;  // walked inline because the queue was full
inline WalkQueue make_queue(const WalkWs &w) {
    WalkQueue q;
    q.counter = w.counter;
    q.items = reinterpret_cast<uint2 *>(w.items);
    q.chunk_count = w.chunk_count;
    q.chunk_mask = reinterpret_cast<uint64_t *>(w.chunk_mask);
    q.slot_of = w.slot_of;
    q.inline_mask = reinterpret_cast<uint64_t *>(w.inline_mask);
    q.capacity = w.capacity;
    return q;
}
inline uint32_t stride_grid(uint32_t work_items) { return max(1u, min(ceil_div(work_items, kThreads), 2048u)); }

// A lane without a splat: no tile passes.
__device__ __forceinline__ TileTest idle_tile_test() {
    TileTest t;
    t.q[0] = t.q[1] = t.q[2] = 0.f;
    t.any = false;
    return t;
}

// Serial walk of one bbox by its own lane (queue-full fallback only).
__device__ __forceinline__ uint32_t walk_inline_count(const uint32_t bb[4], const TileTest &tt, const float xy[2]) {
    uint32_t cnt = 0;
    for (uint32_t ty = bb[1]; ty < bb[3]; ty++)
        for (uint32_t tx = bb[0]; tx < bb[2]; tx++)
            if (can_be_visible(tt, tx, ty, xy)) cnt++;
    return cnt;
}
__device__ __forceinline__ void walk_inline_emit(const uint32_t bb[4], const TileTest &tt, const float xy[2],
                                                 uint32_t c, uint32_t isect, uint32_t tbx, uint32_t cap,
                                                 uint32_t *__restrict__ tile_ids, uint32_t *__restrict__ gids) {
    for (uint32_t ty = bb[1]; ty < bb[3]; ty++)
        for (uint32_t tx = bb[0]; tx < bb[2]; tx++)
            if (can_be_visible(tt, tx, ty, xy) && isect < cap) {
                tile_ids[isect] = tx + ty * tbx;
                gids[isect] = c;
                isect++;
            }
}

// Row / column of row-major index i in a rectangle `bw` tiles wide: i = row * bw + col.  The u32 division the compiler
// emits is ~25 instructions; here one v_rcp_f32 estimate (i < 2^24 is exact in f32, so the estimate is off by at most
// one) and an integer fix-up make it exact for every input the walks can produce.
__device__ __forceinline__ void row_col(uint32_t i, uint32_t bw, uint32_t &row, uint32_t &col) {
    int32_t q = (int32_t)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)bw));
    int32_t r = (int32_t)i - q * (int32_t)bw;
    if (r < 0) q -= 1, r += (int32_t)bw;
    else if (r >= (int32_t)bw) q += 1, r -= (int32_t)bw;
    row = (uint32_t)q, col = (uint32_t)r;
}
// Id of tile i (row-major) of the rectangle at (b0, b1), `bw` tiles wide, on a screen `tbx` tiles wide.
__device__ __forceinline__ uint32_t tile_id_at(uint32_t b0, uint32_t b1, uint32_t bw, uint32_t i, uint32_t tbx) {
    uint32_t row, col;
    row_col(i, bw, row, col);
    return (b0 + col) + (b1 + row) * tbx;
}

// Owner of entry j of a wave-flattened list: the number of lanes whose inclusive prefix `incl` is <= j (the prefixes
// are non-decreasing), by a 6-step shuffle binary search.
__device__ __forceinline__ uint32_t wave_owner(uint32_t incl, uint32_t j) {
    uint32_t own = 0;
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1)
        if (__shfl(incl, own + step - 1, 64) <= j) own += step;
    return min(own, kWave - 1);
}

// ---- two-phase tile test (splat_math.hpp: tile_test_head / tile_test_tail) --------------------------------------------
// Every candidate tile gets the cheap head at once; the ~18 % whose head returns kTileEdge wait in a per-wave LDS ring
// with their geometry until 64 of them are there, then the expensive tail runs on a full wave and its hits are OR-ed
// into the owner's late-hit words.  The owner adds them to its hit mask when the walk is over.
constexpr uint32_t kLateRing = 128;  // < 64 waiting + <= 64 pushed per step
struct LateRing {
    float4 a[kLateRing];  // q0 q1 q2 centre.x
    float4 b[kLateRing];  // centre.y | tx + (ty << 16) | owner lane + (bit << 8) | -
    uint32_t lo[kWave], hi[kWave];  // late hits of the mask owned by lane l
};
// One ring per wave: 4 x 4608 = 18 432 bytes of static LDS in k_walk_count, and 20 more (wave_chunks, block_base_s) in
// k_project_visible.
static_assert(sizeof(LateRing) == 4608, "the two walk kernels' static LDS follows from this");
struct LateState {
    uint32_t head, count;  // wave-uniform
};
__device__ __forceinline__ void late_reset(LateRing &R, LateState &st) {
    R.lo[lane_id()] = 0u;
    R.hi[lane_id()] = 0u;
    st.head = st.count = 0u;
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void late_run(LateRing &R, uint32_t first, uint32_t n) {
    const uint32_t lane = lane_id();
    if (lane < n) {
        const uint32_t e = (first + lane) & (kLateRing - 1u);
        const float4 a = R.a[e], b = R.b[e];
        const float q[3] = {a.x, a.y, a.z};
        const float c[2] = {a.w, b.x};
        const uint32_t t = __float_as_uint(b.y), dst = __float_as_uint(b.z);
        if (tile_test_tail(q, t & 0xFFFFu, t >> 16, c)) {
            const uint32_t owner = dst & 0xFFu, bit = dst >> 8;
            atomicOr(bit < 32u ? &R.lo[owner] : &R.hi[owner], 1u << (bit & 31u));
        }
    }
    __builtin_amdgcn_wave_barrier();
}
// Must be called by all 64 lanes.  `edge`: this lane's candidate needs the tail.
__device__ __forceinline__ void late_push(LateRing &R, LateState &st, bool edge, const float q[3], const float c[2],
                                          uint32_t tx, uint32_t ty, uint32_t owner, uint32_t bit) {
    const uint64_t m = __ballot(edge);
    if (m == 0ull) return;  // wave-uniform
    if (edge) {
        const uint32_t e = (st.head + st.count + __popcll(m & lanemask_lt())) & (kLateRing - 1u);
        R.a[e] = make_float4(q[0], q[1], q[2], c[0]);
        R.b[e] = make_float4(c[1], __uint_as_float(tx | (ty << 16)), __uint_as_float(owner | (bit << 8)), 0.0f);
    }
    st.count += (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
    if (st.count >= kWave) {
        late_run(R, st.head, kWave);
        st.head = (st.head + kWave) & (kLateRing - 1u);
        st.count -= kWave;
    }
}
// Runs what is left and returns this lane's late hits.
__device__ __forceinline__ uint64_t late_flush(LateRing &R, LateState &st) {
    if (st.count) late_run(R, st.head, st.count);
    st.head = (st.head + st.count) & (kLateRing - 1u);
    st.count = 0u;
    __builtin_amdgcn_wave_barrier();
    const uint64_t late = ((uint64_t)R.hi[lane_id()] << 32) | R.lo[lane_id()];
    __builtin_amdgcn_wave_barrier();
    return late;
}

// Wave-flattened walk of the wave's small bboxes.  `area` = this lane's bbox tile count (0 if the
// lane has no small bbox).  Must be called by all 64 lanes.  Returns this lane's hit count and
// its row-major hit mask.
// `first` = row-major index (inside the lane's bbox) of the lane's first candidate: 0 for a whole
// small bbox, k * kChunkTiles for chunk k of a queued one.
__device__ __forceinline__ void walk_flat(uint32_t area, const uint32_t bb[4], const TileTest &tt, const float xy[2],
                                          uint32_t first, uint32_t &cnt, uint64_t &mask, LateRing &ring) {
    const uint32_t lane = lane_id();
    const uint32_t bw = bb[2] - bb[0];
    cnt = 0;
    mask = 0;
    const TileReach reach = make_tile_reach(tt);
    LateState st;
    late_reset(ring, st);
    const uint32_t incl = wave_inclusive_scan(area);
    const uint32_t excl = incl - area;
    const uint32_t total = wave_bcast(incl, 63u);
    for (uint32_t base = 0; base < total; base += kWave) {  // wave-uniform
        const uint32_t j = base + lane;
        // wave_owner(incl, j), written out: through the helper k_project_visible comes out rescheduled
        uint32_t own = 0;
#pragma unroll
        for (uint32_t step = 32; step > 0; step >>= 1)
            if (__shfl(incl, own + step - 1, 64) <= j) own += step;
        own = min(own, kWave - 1);
        TileTest ot;
        ot.q[0] = __shfl(tt.q[0], own, 64);
        ot.q[1] = __shfl(tt.q[1], own, 64);
        ot.q[2] = __shfl(tt.q[2], own, 64);
        ot.any = __shfl((int)tt.any, own, 64) != 0;
        const float oxy[2] = {__shfl(xy[0], own, 64), __shfl(xy[1], own, 64)};
        const uint32_t ob0 = __shfl(bb[0], own, 64), ob1 = __shfl(bb[1], own, 64);
        const uint32_t obw = __shfl(bw, own, 64), oexcl = __shfl(excl, own, 64), ofirst = __shfl(first, own, 64);
        TileReach orr;
        orr.rx = __shfl(reach.rx, own, 64);
        orr.ry = __shfl(reach.ry, own, 64);
        uint32_t cls = kTileMiss, tx = 0, ty = 0;
        if (j < total) {
            const uint32_t li = ofirst + (j - oexcl);
            uint32_t row, col;
            row_col(li, obw, row, col);
            tx = ob0 + col, ty = ob1 + row;
            cls = tile_test_head(ot, orr, tx, ty, oxy);
        }
        const uint64_t bal = __ballot(cls == kTileHit);
        late_push(ring, st, cls == kTileEdge, ot.q, oxy, tx, ty, own, j - oexcl);
        // harvest: this lane's candidates occupy [excl, incl) of the flattened list
        const uint32_t lo = max(excl, base), hi = min(incl, base + kWave);
        if (lo < hi) {
            const uint32_t len = hi - lo;
            const uint64_t seg = (bal >> (lo - base)) & (len == 64 ? ~0ull : ((1ull << len) - 1ull));
            mask |= seg << (lo - excl);
        }
    }
    mask |= late_flush(ring, st);
    cnt = (uint32_t)__popcll(mask);
}

// Geometry of one queued splat, rebuilt from its ProjectedSplat record (words 0-4 and 8: xy, conic, opacity).
struct SplatWalk {
    float xy[2];
    TileTest tt;
    TileReach reach;
    uint32_t b0, b1, bw, area;  // the walk rectangle (splat_math.hpp: walk_rect)
};
__device__ __forceinline__ SplatWalk load_walk(const ViewParams &vp, const float *__restrict__ projected, uint32_t c) {
    const float *p = projected + (size_t)c * BRUSH_PROJECTED_FLOATS;
    SplatWalk s;
    s.xy[0] = p[0];
    s.xy[1] = p[1];
    const float conic[3] = {p[2], p[3], p[4]};
    uint32_t bb[4];
    s.tt = make_tile_test(conic, p[8]);
    s.reach = make_tile_reach(s.tt);
    walk_rect(s.xy, conic, s.tt, s.reach, vp.tile_bounds, bb);
    s.b0 = bb[0];
    s.b1 = bb[1];
    s.bw = bb[2] - bb[0];
    s.area = s.bw * (bb[3] - bb[1]);
    return s;
}

}  // namespace
}  // namespace brush
