// tile_sort.hip — the tile sort of a frame of 257 to 65 536 tiles in the default mode and the fused launch shape: three
// launches instead of four.
//
// A tile id of 9 to 16 significant bits: bucket = its top 8 bits, a shift of the key, so ONE plain count + scatter pair
// (sort_partition_launch, radix_sort.hip) partitions the pairs with (shift, mask) = (sig - 8, 0xFF), and one workgroup
// per bucket (k_tile_bucket_finish, here) finishes its bucket with ONE stable counting pass over the `shift` <= 8 bits
// below, streaming the bucket through registers in 8192-pair chunks.  Every tile's run lies inside one bucket, so that
// workgroup also knows the run's start and end: the bin edges are plain stores (no per-key atomicMax proposals).  Tile
// sort 27.7 -> 20.5 us in situ at the headline scene (profiles/tile_sort_buckets.json).  sort_common.hpp states what
// the scatter leaves for the finish kernel.  Anything else runs sort_launch.
#include "internal.hpp"
#include "sort_common.hpp"

namespace brush {
namespace {

constexpr uint32_t kTileFinishItems = 8;                                // pairs per lane and chunk, in registers
constexpr uint32_t kTileFinishChunk = kSortThreads * kTileFinishItems;  // 8192: pairs a finish workgroup ranks at a time
struct TileFinishLds {
    uint32_t wave_hist[kSortWaves][kRadix];
    uint32_t wave_tot2[4][2];
};

// Workgroup b: bucket b = pairs [off[b], off[b + 1]) of the scatter's output (tmp), all with key >> shift == b, in
// ascending compact gid order inside every tile (the scatter is stable).  Values -> the same range of vals_out ordered
// by (key, position); no keys are written.  Tile t = (b << shift) | d with a non-zero count: edges[2 t] = ~start,
// edges[2 t + 1] = end (the caller zeroed the array, absent tiles stay (0, 0)).
// The bucket is streamed in chunks of kTileFinishChunk pairs held in registers: the waves own contiguous pieces of a
// chunk and rank 64 keys at a time with match-any ballots (index order = stable), thread d carries digit d's running
// output position from chunk to chunk.  A bucket of one chunk (every evenly spread scene up to 2 M pairs) takes its
// digit totals from the ranking itself: one trip to memory.  A longer one counts its digits in a coalesced pass first.
// Any size is the same path; no workgroup waits for another one and every loop is bounded by a count read once.
__global__ __launch_bounds__(kSortThreads) void k_tile_bucket_finish(
    const uint32_t *__restrict__ tmp_keys, const uint32_t *__restrict__ tmp_vals, uint32_t *__restrict__ vals_out,
    uint32_t *__restrict__ edges, uint32_t edge_keys, const uint32_t *__restrict__ d_n, uint32_t max_n, uint32_t shift,
    const uint32_t *__restrict__ bucket_off) {
    __shared__ TileFinishLds L;
    // the finish preamble of sort_common.hpp's contract, as in k_sort_bucket_finish: kernel_diff refused a shared helper
    const uint32_t off0 = bucket_off[blockIdx.x], off1 = bucket_off[blockIdx.x + 1];  // requested beside the count
    const uint32_t n = min(*d_n, max_n);
    if (n == 0) return;  // no scatter workgroup ran: the offsets are leftovers, nothing has looked at them
    const uint32_t start = min(off0, n), stop = min(off1, n);
    if (stop <= start) return;
    const uint32_t cnt = stop - start;
    const uint32_t sub_mask = (1u << shift) - 1u;  // shift <= 8
    const uint32_t wid = threadIdx.x / kWave, lane = lane_id();
    const uint64_t lt = lanemask_lt();
    tmp_keys += start, tmp_vals += start;
    const bool one_chunk = cnt <= kTileFinishChunk;  // block-uniform

    // thread d < 256: pairs of digit d in the whole bucket -> position of the next pair of digit d in vals_out, and
    // the edges of tile (b << shift) | d.  Every thread calls (two barriers).
    uint32_t next_pos = 0;
    auto publish = [&](uint32_t tot) {
        uint32_t smaller = tot, unused = 0;
        block_excl_scan256_pair(smaller, unused, L.wave_tot2);
        next_pos = start + smaller;
        const uint32_t t = (blockIdx.x << shift) | threadIdx.x;
        if (threadIdx.x <= sub_mask && tot != 0u && t < edge_keys) {
            edges[2 * t] = ~next_pos;
            edges[2 * t + 1] = next_pos + tot;
        }
    };
    if (!one_chunk) {
        zero_wave_hist<kSortWaves, kSortThreads>(L.wave_hist);
        __syncthreads();
        constexpr uint32_t kCountLoads = 8;
        for (uint32_t i0 = 0; i0 < cnt; i0 += kSortThreads * kCountLoads) {
            uint32_t k[kCountLoads];
#pragma unroll
            for (uint32_t j = 0; j < kCountLoads; j++) {
                const uint32_t i = i0 + j * kSortThreads + threadIdx.x;
                k[j] = i < cnt ? tmp_keys[i] : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < kCountLoads; j++)
                if (i0 + j * kSortThreads + threadIdx.x < cnt) atomicAdd(&L.wave_hist[wid][k[j] & sub_mask], 1u);
        }
        __syncthreads();
        uint32_t tot = 0;
        // the 16-wave total, written out here and below: kernel_diff refused a shared helper (the adds swap operands)
        if (threadIdx.x < kRadix) {
#pragma unroll
            for (uint32_t w = 0; w < kSortWaves; w++) tot += L.wave_hist[w][threadIdx.x];
        }
        publish(tot);  // its barriers also order the reads above before the zeroing below
    }
    for (uint32_t c0 = 0; c0 < cnt; c0 += kTileFinishChunk) {  // block-uniform
        const uint32_t m = min(kTileFinishChunk, cnt - c0);
        const uint32_t per_wave = ceil_div(m, kSortThreads) * kWave;
        const uint32_t beg = min(m, wid * per_wave), end = min(m, beg + per_wave);
        uint32_t key[kTileFinishItems], val[kTileFinishItems], rank[kTileFinishItems];
#pragma unroll
        for (uint32_t i = 0; i < kTileFinishItems; i++) {
            const uint32_t idx = beg + i * kWave + lane;
            key[i] = idx < end ? tmp_keys[c0 + idx] : 0u;
            val[i] = idx < end ? tmp_vals[c0 + idx] : 0u;
        }
        zero_wave_hist<kSortWaves, kSortThreads>(L.wave_hist);
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kTileFinishItems; i++) {
            if (beg + i * kWave >= end) break;  // wave-uniform
            const bool valid = beg + i * kWave + lane < end;
            const uint32_t digit = key[i] & sub_mask;
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (uint32_t b = 0; b < 8; b++) {
                if (b >= shift) break;  // uniform
                const bool bit = (digit >> b) & 1u;
                const uint64_t vote = __ballot(valid && bit);
                peers &= bit ? vote : ~vote;
            }
            rank[i] = claim_rank(peers, valid, lane, lt, &L.wave_hist[wid][digit]);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        // thread d: the waves' counts of digit d -> output positions of their first pair of digit d
        uint32_t chunk_tot = 0;
        if (threadIdx.x < kRadix) {
#pragma unroll
            for (uint32_t w = 0; w < kSortWaves; w++) chunk_tot += L.wave_hist[w][threadIdx.x];
        }
        if (one_chunk) publish(chunk_tot);
        if (threadIdx.x < kRadix) wave_hist_to_starts<kSortWaves>(L.wave_hist, threadIdx.x, next_pos);
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kTileFinishItems; i++) {
            if (beg + i * kWave + lane < end) vals_out[L.wave_hist[wid][key[i] & sub_mask] + rank[i]] = val[i];
        }
        if (!one_chunk) __syncthreads();  // the next chunk zeroes the counters
    }
}

// sig: the significant bits of the largest tile id.
bool tile_sort_uses_buckets(uint32_t max_n, uint32_t sig) { return sort_is_fused(max_n) && sig > 8u && sig <= 16u; }

}  // namespace

hipError_t tile_sort_launch(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                            const uint32_t *d_n, uint32_t max_n, uint32_t bits, void *ws, hipStream_t s, uint32_t *edges,
                            uint32_t num_tiles) {
    const uint32_t sig = significant_bits(num_tiles ? num_tiles - 1u : 0u);
    if (!vals_in || keys_out || !edges || !tile_sort_uses_buckets(max_n, sig))
        return sort_launch(keys_in, vals_in, keys_out, vals_out, d_n, max_n, bits, ws, s, edges, num_tiles);
    if (max_n == 0) return hipSuccess;
    const SortWs w = carve_sort(ws, max_n);
    const uint32_t shift = sig - 8u;
    const hipError_t e = sort_partition_launch(keys_in, vals_in, d_n, max_n, w, s, false, shift);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tile_bucket_finish, dim3(kRadix), dim3(kSortThreads), 0, s, (const uint32_t *)w.tmp_keys,
                       (const uint32_t *)w.tmp_vals, vals_out, edges, num_tiles, d_n, max_n, shift,
                       (const uint32_t *)w.bucket_off);
    return hipGetLastError();
}

}  // namespace brush
