// tile_emit.hip — the emit pass of the tile walks: the (tile id, compact gid) list of every visible splat, replayed
// from the hit masks of the count pass (tile_count.hip; the contract is in tile_walk.hpp), and the tile bin edges.
//
// Replaces (paths relative to the reference checkout):
//   MapGaussiansToIntersect  crates/brush-render/src/shaders/map_gaussian_to_intersects.wgsl:10-48
//   GetTileBinEdges          .../get_tile_bin_edges.wgsl:15-42
//
// Compiled with -ffp-contract=off like project.hip: the tile lists are reproducible bit-for-bit.
#include "tile_walk.hpp"
#include "trace.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

// ---- MapGaussiansToIntersect ---------------------------------------------------------------
// map_gaussian_to_intersects.wgsl:10-48: splats walked inline by project_visible emit here inline;
// queued splats are emitted by the queue role of the same launch.
// Index of the k-th set bit (k = 0 is the lowest) of a 64-bit mask that has more than k bits set.
__device__ __forceinline__ uint32_t kth_set_bit(uint64_t m, uint32_t k) {
    uint32_t w = (uint32_t)m, base = 0;
    const uint32_t c0 = __popc(w);
    if (k >= c0) k -= c0, w = (uint32_t)(m >> 32), base = 32;
#pragma unroll
    for (uint32_t s = 16; s >= 1; s >>= 1) {
        const uint32_t c = __popc(w & ((1u << s) - 1u));
        if (k >= c) k -= c, w >>= s, base += s;
    }
    return base;
}

// Inline splats, two forms chosen from the visible count (block-uniform):
//  * up to kFlatEmitMin visible splats: one lane per splat replays its recorded hit mask into its own output run (the
//    launch is bound by its dependent-load chain, the short serial loops are free);
//  * beyond: the wave's 64 consecutive inline splats own ONE contiguous output range (their offsets are consecutive
//    values of the scan), so the emission is flattened like the count walk: lane l of step s writes entry 64 s + l of
//    that range, finding its splat by a shuffle binary search over the running hit counts and its tile as the k-th set
//    bit of that splat's hit mask.  Consecutive lanes, consecutive addresses: at 2 M visible splats / 18 M
//    intersections 139 -> 79 us for the launch (lane-private runs: a stride of ~9 entries between neighbouring lanes);
//    at 100 k visible splats the flat form is 2 us SLOWER (same-box A/B), hence the switch.
__device__ __forceinline__ void map_inline_role(uint32_t bid, uint32_t nblocks, const ViewParams &vp,
                                                const float *__restrict__ projected,
                                                const uint32_t *__restrict__ cum_tiles_hit,
                                                const uint32_t *__restrict__ num_visible, uint32_t cap,
                                                uint32_t *__restrict__ tile_ids, uint32_t *__restrict__ gids,
                                                const WalkQueue &q) {
    const uint32_t V = *num_visible;
    const uint32_t lane = lane_id();
    const bool flat = V >= kFlatEmitMin;
    const uint32_t wave_stride = nblocks * kThreads;
    for (uint32_t cbase = bid * kThreads + (threadIdx.x / kWave) * kWave; cbase < V; cbase += wave_stride) {  // wave-uniform
        const uint32_t c = cbase + lane;
        const uint32_t code = c < V ? q.slot_of[c] : 0u;
        const bool replay = (code & kInlineFlag) && code != kInlineRetest;
        uint32_t bb[4] = {0, 0, 0, 0};
        uint32_t start = 0;
        uint64_t mask = 0;
        float xy[2] = {0.f, 0.f};
        TileTest tt = idle_tile_test();
        if (code & kInlineFlag) {  // inline splat (replayed or re-tested): its rectangle and its first output slot
            // load_walk's rebuild, written out: the retest below needs the whole bb, and one helper under both changes
            // this kernel's and k_walk_count's control flow
            const float *p = projected + (size_t)c * BRUSH_PROJECTED_FLOATS;
            xy[0] = p[0], xy[1] = p[1];
            const float conic[3] = {p[2], p[3], p[4]};
            tt = make_tile_test(conic, p[8]);
            walk_rect(xy, conic, tt, make_tile_reach(tt), vp.tile_bounds, bb);
            start = c > 0 ? cum_tiles_hit[c - 1] : 0u;
            if (replay) mask = q.inline_mask[c];
        }
        const uint32_t bw = bb[2] - bb[0];
        if (!flat) {
            uint32_t isect = start;
            while (mask) {  // row-major over the walk rectangle
                const uint32_t i = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                if (isect < cap) {
                    tile_ids[isect] = tile_id_at(bb[0], bb[1], bw, i, vp.tile_bounds[0]);
                    gids[isect] = c;
                    isect++;
                }
            }
        } else {
            const uint32_t cnt = (uint32_t)__popcll(mask);
            const uint32_t incl = wave_inclusive_scan(cnt), excl = incl - cnt;
            const uint32_t total = wave_bcast(incl, 63u);
            const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
            for (uint32_t base = 0; base < total; base += kWave) {  // wave-uniform
                const uint32_t j = base + lane;
                const uint32_t own = wave_owner(incl, j);
                const uint64_t omask = ((uint64_t)__shfl(mhi, own, 64) << 32) | __shfl(mlo, own, 64);
                const uint32_t ob0 = __shfl(bb[0], own, 64), ob1 = __shfl(bb[1], own, 64), obw = __shfl(bw, own, 64);
                const uint32_t k = j - __shfl(excl, own, 64);
                const uint32_t pos = __shfl(start, own, 64) + k;
                if (j < total && pos < cap) {
                    tile_ids[pos] = tile_id_at(ob0, ob1, obw, kth_set_bit(omask, k), vp.tile_bounds[0]);
                    gids[pos] = cbase + own;
                }
            }
        }
        // queue-full fallback: the splat was counted by an inline walk and is walked again here (rare)
        if (code == kInlineRetest) walk_inline_emit(bb, tt, xy, c, start, vp.tile_bounds[0], cap, tile_ids, gids);
    }
}

// Emission for the queued splats, walk_group(n) items per wave like the count pass.  Item (c, k) writes
// after the k earlier chunks of its splat, which are the k items before it in the queue: their hit
// total is a difference of the group-local running counts (at most 128 / G + 2 loads), so
// the entries of a splat land in [cum[c-1], cum[c]) in row-major bbox order, as an inline walk
// writes them.
__device__ __forceinline__ void map_queue_role(uint32_t bid, uint32_t nblocks, const ViewParams &vp,
                                               const float *__restrict__ projected,
                                               const uint32_t *__restrict__ cum_tiles_hit, uint32_t cap,
                                               uint32_t *__restrict__ tile_ids, uint32_t *__restrict__ gids,
                                               const WalkQueue &q) {
    const uint32_t n_items = min(*q.counter, q.capacity);
    const uint32_t G = walk_group(n_items);
    const uint32_t n_groups = (n_items + G - 1) / G;
    const uint32_t lane = lane_id();
    const uint64_t lt = lanemask_lt();
    const uint32_t waves = nblocks * (kThreads / kWave);
    for (uint32_t grp = bid * (kThreads / kWave) + threadIdx.x / kWave; grp < n_groups; grp += waves) {
        const uint32_t g_first = grp * G;
        const uint32_t it = g_first + lane;
        const bool mine = lane < G && it < n_items;
        uint2 item = make_uint2(kInvalid, 0u);
        if (mine) item = q.items[it];
        const bool valid = mine && item.x != kInvalid;
        uint32_t b0 = 0, b1 = 0, bw = 1, base = 0, first = 0;
        uint64_t mask = 0;
        if (valid) {
            const uint32_t c = item.x, k = item.y;
            mask = q.chunk_mask[it];
            // hits of the k preceding items = [it - k, it): whole groups by their last running count,
            // the two partial groups by differences
            uint32_t before = 0;
            const uint32_t lo = it - k;  // first item of this splat
            if (lo >= g_first) {         // all in this group
                before = (lane > 0 ? q.chunk_count[it - 1] : 0u) - (lo > g_first ? q.chunk_count[lo - 1] : 0u);
            } else {
                before = lane > 0 ? q.chunk_count[it - 1] : 0u;                       // this group's part
                const uint32_t lo_grp = lo / G;
                for (uint32_t g2 = lo_grp + 1; g2 < grp; g2++) before += q.chunk_count[g2 * G + G - 1];
                const uint32_t lg_last = lo_grp * G + G - 1;                             // the splat's first group
                before += q.chunk_count[lg_last] - (lo > lo_grp * G ? q.chunk_count[lo - 1] : 0u);
            }
            const SplatWalk s = load_walk(vp, projected, c);
            b0 = s.b0, b1 = s.b1, bw = s.bw;
            first = k * kChunkTiles;
            base = (c > 0 ? cum_tiles_hit[c - 1] : 0u) + before;
        }
        const uint32_t mlo = (uint32_t)mask, mhi = (uint32_t)(mask >> 32);
        const uint32_t in_group = min(G, n_items - g_first);
        for (uint32_t qi = 0; qi < in_group; qi++) {  // wave-uniform
            const uint64_t bal = ((uint64_t)wave_bcast(mhi, qi) << 32) | wave_bcast(mlo, qi);
            if (bal == 0ull) continue;
            const uint32_t qb0 = wave_bcast(b0, qi), qb1 = wave_bcast(b1, qi), qbw = wave_bcast(bw, qi);
            const uint32_t i = wave_bcast(first, qi) + lane;
            const uint32_t pos = wave_bcast(base, qi) + __popcll(bal & lt);
            const uint32_t qc = wave_bcast(item.x, qi);
            if (((bal >> lane) & 1ull) && pos < cap) {
                tile_ids[pos] = tile_id_at(qb0, qb1, qbw, i, vp.tile_bounds[0]);
                gids[pos] = qc;
            }
        }
    }
}

// One launch, two roles: the first `inline_blocks` workgroups emit the inline splats, the rest consume
// the queue (they write disjoint ranges of the same arrays, so neither waits for the other).
__global__ __launch_bounds__(kThreads) void k_map_intersects(ViewParams vp, const float *__restrict__ projected,
                                                             const uint32_t *__restrict__ cum_tiles_hit,
                                                             const uint32_t *__restrict__ num_visible, uint32_t cap,
                                                             uint32_t *__restrict__ tile_ids,
                                                             uint32_t *__restrict__ gids, WalkQueue q,
                                                             uint32_t inline_blocks) {
    BRUSH_KTRACE(kTrMap, blockIdx.x < inline_blocks ? 0u : (1u << 24) | 1u);
    if (blockIdx.x < inline_blocks)
        map_inline_role(blockIdx.x, inline_blocks, vp, projected, cum_tiles_hit, num_visible, cap, tile_ids, gids, q);
    else
        map_queue_role(blockIdx.x - inline_blocks, gridDim.x - inline_blocks, vp, projected, cum_tiles_hit, cap,
                       tile_ids, gids, q);
}

// ---- GetTileBinEdges -----------------------------------------------------------------------
// get_tile_bin_edges.wgsl:15-42
// perm != nullptr (deterministic mode): the tile sort carried the PRE-SORT positions as values; the compact gid
// of sorted intersection i is then gathered from the unsorted list here.
__global__ __launch_bounds__(kThreads) void k_tile_bin_edges(const uint32_t *__restrict__ sorted_tile_ids,
                                                             const uint32_t *__restrict__ num_intersections,
                                                             uint32_t *__restrict__ tile_bins,
                                                             const uint32_t *__restrict__ perm,
                                                             const uint32_t *__restrict__ gid_unsorted,
                                                             uint32_t *__restrict__ gid_sorted) {
    const uint32_t I = *num_intersections;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < I; i += gridDim.x * kThreads) {
        const uint32_t cur = sorted_tile_ids[i];
        if (perm) gid_sorted[i] = gid_unsorted[perm[i]];
        if (i == I - 1) tile_bins[cur * 2 + 1] = I;
        if (i == 0) {
            tile_bins[cur * 2 + 0] = 0;
        } else {
            const uint32_t prev = sorted_tile_ids[i - 1];
            if (prev != cur) {
                tile_bins[prev * 2 + 1] = i;
                tile_bins[cur * 2 + 0] = i;
            }
        }
    }
}

}  // namespace

hipError_t launch_map_intersects(const ViewParams &vp, const float *projected, const uint32_t *cum_tiles_hit,
                                 const uint32_t *num_visible, uint32_t cap, uint32_t *tile_ids, uint32_t *gids,
                                 const WalkWs &walk, hipStream_t s) {
    const WalkQueue q = make_queue(walk);
    const uint32_t inline_blocks = stride_grid(vp.total_splats);
    hipLaunchKernelGGL(k_map_intersects, dim3(inline_blocks + 1024u), dim3(kThreads), 0, s, vp, projected,
                       cum_tiles_hit, num_visible, cap, tile_ids, gids, q, inline_blocks);
    return hipGetLastError();
}

hipError_t launch_tile_bin_edges(const uint32_t *sorted_tile_ids, const uint32_t *num_intersections,
                                 uint32_t cap, uint32_t *tile_bins, const uint32_t *perm,
                                 const uint32_t *gid_unsorted, uint32_t *gid_sorted, hipStream_t s) {
    hipLaunchKernelGGL(k_tile_bin_edges, dim3(stride_grid(cap)), dim3(kThreads), 0, s, sorted_tile_ids,
                       num_intersections, tile_bins, perm, gid_unsorted, gid_sorted);
    return hipGetLastError();
}

}  // namespace brush
