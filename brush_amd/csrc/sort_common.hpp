// sort_common.hpp — what the three sorters share: the LSD passes (radix_sort.hip), the depth sort by key-range buckets
// (depth_sort.hip) and the tile sort by tile-range buckets (tile_sort.hip).
//
// All of them run 1024-thread workgroups (16 waves) over 256 digits, keep one LDS counter row per wave
// (wave_hist[wave][digit]) and rank the keys of a wave with match-any ballots; the helpers below are the pieces of that
// scheme that more than one kernel uses.  The element count stays on the device (*d_n): grids are sized for max_n and
// surplus workgroups exit at once.
//
// The contract between the partition launcher and the two bucket finish kernels.  sort_partition_launch (radix_sort.hip)
// runs ONE count + scatter pair of the fused launch shape over the n = min(*d_n, max_n) pairs and leaves them in
// w.tmp_keys / w.tmp_vals, grouped by bucket: the bucket of a key is bucket_of over sampled splitters (the depth sort)
// or (key >> shift) & 0xFF (the tile sort), so buckets are ordered like the keys.  The scatter is stable: inside a
// bucket the pairs keep their input order.  Tile 0 of the scatter stores the run starts: bucket_off[b] = position of the
// first pair of bucket b, bucket_off[256] = n, ascending.  Tile 0 exists whenever n > 0; when n == 0 no workgroup of
// the scatter runs and bucket_off holds leftovers, so a finish workgroup reads n itself and looks at nothing else when
// it is zero.  Workgroup b of a finish kernel owns pairs [bucket_off[b], bucket_off[b + 1]) and
// that range of the outputs, and waits for no other workgroup.  The fused shape leaves two pieces of its workspace
// unused and the bucket sorts live in them (SortWs): `splitters` is `totals`, `bucket_off` is the upper half of the
// count table, whose rows are 16-bit in that shape.  Both sorts of a frame run in one workspace, in turn.
#pragma once
#include <initializer_list>
#include <utility>

#include "common.hpp"

namespace brush {

constexpr uint32_t kSortThreads = 1024;
constexpr uint32_t kSortWaves = kSortThreads / kWave;  // 16
constexpr uint32_t kSortMaxItems = 16;
// Measured at the headline scene (sweep of the keys per lane): the 103 k-key depth sort is fastest with 1 key per
// lane (101 tiles), the 419 k-key tile sort with 4 (103 tiles): ~100 workgroups either way.
constexpr uint32_t kSortTargetTiles = 128;
constexpr uint32_t kRadix = 256;
constexpr uint32_t kMaxTileKeys = kSortThreads * kSortMaxItems;  // 16384
constexpr uint32_t kFusedMaxTiles = 512;
// Sorts larger than that (3-launch shape): fixed 8192-key tiles.
constexpr uint32_t kBigTileKeys = 8192;
// The depth sort partitions clouds of up to this many splats into key-range buckets (depth_sort.hip).
constexpr uint32_t kBucketMaxN = 1u << 20;

// Keys per lane for a sort of n keys: smallest power of two K in [1,16] with n / (1024 K) <= 128.
__host__ __device__ __forceinline__ uint32_t sort_items(uint32_t n) {
    uint32_t k = 1;
    while (k < kSortMaxItems && (uint64_t)kSortThreads * k * kSortTargetTiles < n) k <<= 1;
    return k;
}
// Upper bound of the tile count over every n <= max_n.
inline uint32_t sort_max_tiles(uint32_t max_n) {
    const uint32_t big = (uint32_t)(((uint64_t)max_n + kMaxTileKeys - 1) / kMaxTileKeys);
    if (big > kFusedMaxTiles) return (uint32_t)(((uint64_t)max_n + kBigTileKeys - 1) / kBigTileKeys);
    return big > kSortTargetTiles ? big : kSortTargetTiles;  // n <= 128 * 1024 * K selects K: never more than 128 tiles
}
inline bool sort_is_fused(uint32_t max_n) {
    return (uint32_t)(((uint64_t)max_n + kMaxTileKeys - 1) / kMaxTileKeys) <= kFusedMaxTiles;
}
// Number of bits up to and including the highest set one (0 for 0).
inline uint32_t significant_bits(uint32_t x) { return x ? 32u - (uint32_t)__builtin_clz(x) : 0u; }

struct SortWs {
    uint32_t *tmp_keys, *tmp_vals, *counts, *totals;
    uint32_t *splitters, *bucket_off;  // fused shape only: aliases of unused pieces, see carve_sort
    uint32_t max_tiles;
    size_t bytes;
};
inline SortWs carve_sort(void *ws, uint32_t max_n) {
    SortWs w;
    Carver c(ws);
    w.max_tiles = sort_max_tiles(max_n ? max_n : 1);
    w.tmp_keys = c.take<uint32_t>(max_n ? max_n : 1);
    w.tmp_vals = c.take<uint32_t>(max_n ? max_n : 1);
    w.counts = c.take<uint32_t>((size_t)kRadix * w.max_tiles);
    w.totals = c.take<uint32_t>(kRadix);
    w.bytes = c.bytes();
    // The fused shape never reads `totals` (here: the 256 splitters) nor the upper half of the count table, whose
    // rows are 16-bit (here: the kRadix + 1 bucket offsets).  The 3-launch shape uses both pieces itself.
    static_assert(kRadix + 1 <= (kRadix / 2) * kSortTargetTiles, "the offsets fit in the unused half");
    w.splitters = w.totals;
    w.bucket_off = ws ? w.counts + (size_t)(kRadix / 2) * w.max_tiles : nullptr;
    return w;
}

// radix_sort.hip.  The single count + scatter pair of a bucket sort (max_n > 0, fused shape): by sampled splitters
// (by_splitters, the depth sort; `shift` unused) or by (key >> shift) & 0xFF (the tile sort).  Leaves the pairs in
// w.tmp_keys / w.tmp_vals and the 257 run starts in w.bucket_off, w.splitters too in the first form (contract above).
hipError_t sort_partition_launch(const uint32_t *keys_in, const uint32_t *vals_in, const uint32_t *d_n, uint32_t max_n,
                                 const SortWs &w, hipStream_t s, bool by_splitters, uint32_t shift);

// Kernels that need more dynamic LDS than the 64 KiB a kernel gets by default opt in once per DEVICE (the attribute
// belongs to the function's instance on the current device; an embedder may drive several devices from one process).
// `done`: one flag array per group of kernels; `kernels`: (kernel, bytes of dynamic LDS) of every kernel of the group.
inline hipError_t enable_big_lds(std::atomic<int> (&done)[kMaxDevices],
                                 std::initializer_list<std::pair<const void *, size_t>> kernels) {
    const int dev = current_device_slot();
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    for (const auto &k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.second);
        if (e != hipSuccess) return e;
    }
    done[dev].store(1, std::memory_order_release);
    return hipSuccess;
}

// ---- device helpers ----
// Every thread of a THREADS-wide workgroup: clears the per-wave digit counters.  No barrier.
template <uint32_t WAVES, uint32_t THREADS>
__device__ __forceinline__ void zero_wave_hist(uint32_t (*wave_hist)[kRadix]) {
    for (uint32_t i = threadIdx.x; i < WAVES * kRadix; i += THREADS) (&wave_hist[0][0])[i] = 0;
}
// Thread d of the first 256: wave_hist[w][d] <- `run` + the counts of digit d in the waves before w; run += all of them.
template <uint32_t WAVES>
__device__ __forceinline__ void wave_hist_to_starts(uint32_t (*wave_hist)[kRadix], uint32_t d, uint32_t &run) {
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
        const uint32_t t = wave_hist[w][d];
        wave_hist[w][d] = run;
        run += t;
    }
}

// Exclusive scans of two 256-entry arrays held by threads 0..255 (one value of each per thread) behind the same
// two barriers; all 1024 threads must call.
__device__ __forceinline__ void block_excl_scan256_pair(uint32_t &a, uint32_t &b, uint32_t (*wave_tot)[2]) {
    const uint32_t ia = wave_inclusive_scan(a), ib = wave_inclusive_scan(b);
    if (threadIdx.x < kRadix && lane_id() == 63) {
        wave_tot[threadIdx.x / kWave][0] = ia;
        wave_tot[threadIdx.x / kWave][1] = ib;
    }
    __syncthreads();
    uint32_t oa = ia - a, ob = ib - b;
    for (uint32_t w = 0; w < threadIdx.x / kWave && w < 4; w++) {
        oa += wave_tot[w][0];
        ob += wave_tot[w][1];
    }
    __syncthreads();
    a = oa, b = ob;
}

// The claim of the match-any ranking step.  `peers`: the valid lanes of the wave whose key has this lane's digit (the
// ballots over the digit bits, which every caller words for its own bit count).  The lowest of them bumps the wave's
// counter of the digit (`counter`, in LDS) by their number; returns the counter's old value + the peers below this
// lane: the lane's rank among the keys of its digit that the wave has seen so far.
__device__ __forceinline__ uint32_t claim_rank(uint64_t peers, bool valid, uint32_t lane, uint64_t lt,
                                               uint32_t *counter) {
    const uint32_t below = __popcll(peers & lt);
    const int leader = valid ? (__ffsll((long long)peers) - 1) : 0;
    uint32_t old = 0;
    if (valid && (int)lane == leader) {
        old = *counter;
        *counter = old + __popcll(peers);
    }
    return __shfl(old, leader, 64) + below;
}

}  // namespace brush
