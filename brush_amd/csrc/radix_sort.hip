// radix_sort.hip — stable LSD radix argsort of u32 key/value pairs (replaces crates/brush-sort), and the count +
// scatter pair that partitions the keys for the two bucket sorts (sort_partition_launch; depth_sort.hip, tile_sort.hip).
//
// Reference: radix_argsort() crates/brush-sort/src/lib.rs:32-147 — FidelityFX-style, 4 bits per
// pass, 5 launches per pass (count / reduce / scan / scan_add / scatter), element count read
// from a GPU buffer, only the low `sorting_bits` sorted.  32-bit keys = 40 launches.
//
// gfx950 design: 8-bit digits (half the passes), 1024-thread workgroups (16 waves), tiles of
// 1024 x {1,2,4,8,16} keys chosen ON THE DEVICE from *d_n: at most 128 tiles while that fits (a 103 k-key
// sort: 101 tiles of 1024 keys, a 419 k-key sort: 103 of 4096), 16384-key tiles when the sort is large.
//   k_sort_upsweep   : per-wave LDS histograms -> counts of the tile's 256 digits
//   k_sort_scan      : (large sorts only) one block per digit scans counts[digit][*] over the tiles
//   k_sort_downsweep : every wave ranks its contiguous chunk with ballot match-any masks (8 x v_cmp per
//                 key on 64-bit masks, the lowest peer lane bumps the wave's private LDS counter),
//                 16-wave combine, then the pairs are REORDERED BY DIGIT IN LDS and written out so
//                 that consecutive lanes write consecutive addresses of a digit run.
// Two launch shapes, chosen on the host from max_n:
//   * FUSED (max_n <= 512 tiles of 16384 keys, i.e. the reference's 8.39 M intersection cap and below):
//     2 launches per pass.  counts are laid out [tile][digit]; every downsweep block sums the rows of the
//     tiles before it and of all tiles itself (T coalesced 1-KiB row reads, T = the ACTUAL tile count of
//     *d_n, ~26-64 at the headline scene) instead of waiting for a scan launch: at 100 k - 400 k keys a
//     pass is bound by kernel boundaries (~4 us each), not by bytes.
//   * otherwise 3 launches per pass with counts laid out [digit][tile] and the scan kernel, fixed 8192-key tiles and
//     512-thread scatter workgroups whose 76 KiB of LDS let two of them share a CU (one's loads and stores overlap the
//     other's ranking): the 18 M-key tile sort of the 4K / 20 M-splat frame 326 -> 246 us (37 % of the HBM peak);
//     256-thread / 4096-key workgroups (four per CU) measured slower (278 us: shorter digit runs, twice the tiles).
// The BUCKET instantiations of the two pass kernels take "bucket of key" over sampled splitters as the digit; they and
// the plain pair with the run starts published are what sort_partition_launch runs (contract: sort_common.hpp).
// Stability: tiles, wave chunks, rounds and lanes are all ranked in index order.
// Traffic per pass: 4 B/key (upsweep) + 16 B/pair (downsweep).  Roofline: HBM at large n, kernel
// boundaries at n ~ 100 k.  The pass structure sorts exactly the reference's 4*ceil(bits/4) low bits.
#include "sort_common.hpp"
#include "trace.hpp"

namespace brush {
namespace {

// 3-launch shape: the 8192-key tiles are scattered by 512-thread workgroups of 16 keys per lane whose LDS image
// (74 KiB) lets TWO of them share a CU, so one's loads and stores overlap the other's ranking.
constexpr uint32_t kBigThreads = 512;
// FUSED scatter: count-table rows every thread requests before the element count has arrived (4 quarters x 32 rows =
// the first kSortTargetTiles rows)
// Thread (group g8 = tid / 128, digit pair dp = tid % 128) owns rows g8 + 8 j of the 16-bit table: 16 dword loads
// cover digits 2 dp and 2 dp + 1 of the first 128 rows (32 registers of 32-bit counts spilled the 16-key variant).
constexpr uint32_t kSpecRows = 16;
constexpr uint32_t kTableGroups = 8;
static_assert(kTableGroups * kSpecRows == kSortTargetTiles, "the table always has the speculatively loaded rows");

// ---- the bucket of a key by sampled splitters (the BUCKET instantiations of the two pass kernels) ----
constexpr uint32_t kSampleKeys = kSortThreads;  // one sampled key per thread of a count workgroup
static_assert(kBucketMaxN <= kSortThreads * 8 * kSortTargetTiles, "bucket scatter: at most 8 keys per lane");

// Trace tag of a count or scatter launch of the 1024-thread kernels: the pass's shift, the pass number and the sort.
__device__ __forceinline__ uint32_t sort_pass_tag(uint32_t shift, uint32_t max_n) {
    return shift | (((shift >> 3) + (max_n > (1u << 21) ? 4u : 0u)) << 24);
}

// Every thread of a 1024-thread workgroup: sorts a fixed-stride sample of the keys (all of them below kSampleKeys,
// padded with the largest key) with a bitonic network, steps inside a wave by lane exchange and the rest through `xch`,
// and leaves every (kSampleKeys / kRadix)-th of it in spl[1 .. 255] (spl[0] is never read).  Ends with a barrier.
__device__ __forceinline__ void select_splitters(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *spl,
                                                 uint32_t (*xch)[kSampleKeys]) {
    const uint32_t t = threadIdx.x;
    uint32_t k = 0xFFFFFFFFu;
    if (n >= kSampleKeys) k = keys[(uint32_t)(((uint64_t)t * n) / kSampleKeys)];
    else if (t < n) k = keys[t];
    uint32_t buf = 0;
#pragma unroll
    for (uint32_t size = 2; size <= kSampleKeys; size <<= 1) {
#pragma unroll
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
            uint32_t other;
            if (j < kWave) {
                other = (uint32_t)__shfl_xor((int)k, (int)j, (int)kWave);
            } else {
                // two buffers in turn: a slot is rewritten two exchanges later, behind the barrier of the one between
                xch[buf][t] = k;
                __syncthreads();
                other = xch[buf][t ^ j];
                buf ^= 1u;
            }
            const bool ascending = (t & size) == 0, lower = (t & j) == 0;
            k = lower == ascending ? min(k, other) : max(k, other);
        }
    }
    constexpr uint32_t kPer = kSampleKeys / kRadix;
    if (t % kPer == 0) spl[t / kPer] = k;
    __syncthreads();
}

// Bucket of a key = number of splitters spl[1 .. 255] (ascending) that are <= key: equal keys share a bucket and the
// buckets are ordered like the keys.
__device__ __forceinline__ uint32_t bucket_of(const uint32_t *spl, uint32_t k) {
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = kRadix / 2; step; step >>= 1) b += spl[b + step] <= k ? step : 0u;
    return b;
}

// BUCKET: the digit is the key's bucket; every workgroup selects the same splitters from the same sample (cheaper than
// a launch of its own and its boundary) and tile 0 publishes them for the scatter kernel.
template <bool FUSED, bool BUCKET = false>
__global__ __launch_bounds__(kSortThreads) void k_sort_upsweep(const uint32_t *__restrict__ keys,
                                                              const uint32_t *__restrict__ d_n, uint32_t max_n,
                                                              uint32_t shift, uint32_t mask,
                                                              uint32_t *__restrict__ counts, uint32_t max_tiles,
                                                              uint32_t *__restrict__ splitters) {
    BRUSH_KTRACE(kTrSortUp, sort_pass_tag(shift, max_n));
    const uint32_t n = min(*d_n, max_n);
    BRUSH_KTRACE_MARK(1, n);
    const uint32_t items = FUSED ? sort_items(n) : kBigTileKeys / kSortThreads;
    const uint32_t tile_keys = kSortThreads * items;
    const uint32_t tile = blockIdx.x;
    if ((uint64_t)tile * tile_keys >= n) return;
    __shared__ uint32_t hist[kSortWaves][kRadix];
    zero_wave_hist<kSortWaves, kSortThreads>(hist);
    const uint32_t *spl = nullptr;
    if constexpr (BUCKET) {
        __shared__ uint32_t spl_s[kRadix], xch[2][kSampleKeys];
        select_splitters(keys, n, spl_s, xch);
        if (tile == 0 && threadIdx.x < kRadix) splitters[threadIdx.x] = spl_s[threadIdx.x];  // [0]: unused
        spl = spl_s;
    }
    __syncthreads();
    const uint32_t wid = threadIdx.x / kWave;
    const uint32_t base = tile * tile_keys;
    for (uint32_t i = 0; i < items; i++) {
        const uint32_t idx = base + i * kSortThreads + threadIdx.x;
        if (idx < n) {
            const uint32_t k = keys[idx];
            if (i == 0) BRUSH_KTRACE_MARK(2, k);
            atomicAdd(&hist[wid][BUCKET ? bucket_of(spl, k) : (k >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    BRUSH_KTRACE_MARK(3, n);
    if (threadIdx.x < kRadix) {
        const uint32_t d = threadIdx.x;
        uint32_t c = 0;
        // the 16-wave total, written out: kernel_diff refused a shared helper (the adds swap their operands)
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; w++) c += hist[w][d];
        // FUSED: 16-bit counts (a tile holds at most 16384 keys), row = 128 dwords of digit pairs
        if (FUSED) reinterpret_cast<uint16_t *>(counts)[(size_t)tile * kRadix + d] = (uint16_t)c;
        else counts[(size_t)d * max_tiles + tile] = c;
    }
}

// Large sorts: block d = exclusive scan over tiles of counts[d][*]; totals[d] = number of keys with digit d.
__global__ __launch_bounds__(256) void k_sort_scan(uint32_t *__restrict__ counts,
                                                   const uint32_t *__restrict__ d_n, uint32_t max_n,
                                                   uint32_t max_tiles, uint32_t *__restrict__ totals) {
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t carry_s;
    const uint32_t n = min(*d_n, max_n);
    const uint32_t num_tiles = (n + kBigTileKeys - 1) / kBigTileKeys;
    uint32_t *row = counts + (size_t)blockIdx.x * max_tiles;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < num_tiles; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < num_tiles ? row[i] : 0u;
        const uint32_t incl = wave_inclusive_scan(v);
        if (lane_id() == 63) wave_tot[threadIdx.x / kWave] = incl;
        __syncthreads();
        uint32_t off = carry_s;
        for (uint32_t w = 0; w < threadIdx.x / kWave; w++) off += wave_tot[w];
        if (i < num_tiles) row[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) carry_s = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry_s;
}

// LDS of the downsweep: the tile's pairs reordered by digit (128 KiB at 16 keys per lane) + the per-wave
// digit counters.  One 1024-thread workgroup per CU.
template <uint32_t TILE_KEYS, uint32_t WAVES, uint32_t PARTS>
struct DownLdsT {
    uint32_t keys[TILE_KEYS];
    uint32_t vals[TILE_KEYS];
    uint32_t wave_hist[WAVES][kRadix];
    uint32_t digit_base[kRadix];  // global position of the tile's first key of each digit
    uint32_t tile_start[kRadix];  // position inside the tile (after the reorder) of each digit's run
    uint32_t wave_tot2[4][2];
    // FUSED: partial column sums of the count table per row group (keys of earlier tiles / of all tiles).  They live
    // from before barrier A to barrier C, the reordered pairs from barrier C on: same storage.
    static_assert(2 * PARTS * kRadix <= TILE_KEYS, "part / part_all alias keys[]");
    __device__ __forceinline__ uint32_t (*part())[kRadix] { return reinterpret_cast<uint32_t(*)[kRadix]>(keys); }
    __device__ __forceinline__ uint32_t (*part_all())[kRadix] {
        return reinterpret_cast<uint32_t(*)[kRadix]>(keys + PARTS * kRadix);
    }
};
using DownLds = DownLdsT<kMaxTileKeys, kSortWaves, kTableGroups>;
using DownLdsBig = DownLdsT<kBigTileKeys, kBigThreads / kWave, 1>;
static_assert(2 * sizeof(DownLdsBig) <= 160 * 1024, "two large-sort workgroups per CU");

// Sums of the speculatively loaded count-table rows (thread = (group g8, digit pair dp), rows g8 + 8 j): keys of the
// pair's digits in the tiles before `tile` / in all `num_tiles` tiles, as packed 16-bit-pair sums of at most 16 rows
// each (16 * 16384 overflows 16 bits, so the halves are split before they are added up).
struct PairSums {
    uint32_t below[2], all[2];
};
// FUSED: the partial column sums of the [tile][digit] count table -> L.part() / L.part_all().  Rows 0 .. 127 were
// requested by the kernel before it knew n (`spec`, masked here); the rest of a large table (more than 128 tiles: sorts
// above 2 M keys) is read with kTableLoads independent row loads in flight per thread (latency-, not bandwidth-bound).
template <typename LDS>
__device__ __forceinline__ void table_sums_to_lds(const uint32_t (&spec)[kSpecRows], const uint32_t *__restrict__ counts,
                                                  uint32_t tile, uint32_t num_tiles, LDS &L, KTraceRef trace) {
    const uint32_t dp = threadIdx.x & (kRadix / 2 - 1), g8 = threadIdx.x / (kRadix / 2);
    PairSums ps{};
#pragma unroll
    for (uint32_t j = 0; j < kSpecRows; j++) {
        const uint32_t t = g8 + kTableGroups * j;
        const uint32_t a = t < num_tiles ? spec[j] : 0u;
        const uint32_t b = t < tile ? spec[j] : 0u;  // tile < num_tiles
        ps.all[0] += a & 0xFFFFu, ps.all[1] += a >> 16;
        ps.below[0] += b & 0xFFFFu, ps.below[1] += b >> 16;
    }
    constexpr uint32_t kTableLoads = 16;
    for (uint32_t t0 = kTableGroups * kSpecRows + g8; t0 < num_tiles; t0 += kTableGroups * kTableLoads) {
        uint32_t c[kTableLoads];
#pragma unroll
        for (uint32_t j = 0; j < kTableLoads; j++) {
            const uint32_t t = t0 + kTableGroups * j;
            c[j] = t < num_tiles ? counts[(size_t)t * (kRadix / 2) + dp] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < kTableLoads; j++) {
            const uint32_t b = (t0 + kTableGroups * j) < tile ? c[j] : 0u;
            ps.all[0] += c[j] & 0xFFFFu, ps.all[1] += c[j] >> 16;
            ps.below[0] += b & 0xFFFFu, ps.below[1] += b >> 16;
        }
    }
    BRUSH_KTRACE_MARK_VIA(trace, 2, ps.below[0] + ps.all[1]);
    L.part()[g8][2 * dp] = ps.below[0], L.part()[g8][2 * dp + 1] = ps.below[1];
    L.part_all()[g8][2 * dp] = ps.all[0], L.part_all()[g8][2 * dp + 1] = ps.all[1];
}

// BUCKET (sort_partition_launch by splitters): the digit of a key is its bucket (bucket_of over `spl`, 256 splitters in
// LDS that are visible from barrier A on), kept packed four to a register; tile 0 also publishes the 257 bucket offsets.
template <bool FUSED, uint32_t ITEMS, uint32_t THREADS, typename LDS, bool BUCKET = false>
__device__ __forceinline__ void downsweep_body(const uint32_t *__restrict__ keys_in,
                                               const uint32_t *__restrict__ vals_in,
                                               uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                               uint32_t n, uint32_t shift, uint32_t mask,
                                               const uint32_t *__restrict__ counts,
                                               const uint32_t *__restrict__ totals, uint32_t max_tiles,
                                               uint32_t *__restrict__ edges, uint32_t edge_keys, LDS &L,
                                               const uint32_t (&spec)[kSpecRows], KTraceRef trace = KTraceRef{},
                                               const uint32_t *spl = nullptr, uint32_t *__restrict__ bucket_off = nullptr) {
    static_assert(!FUSED || THREADS == kSortThreads, "the fused table sums assume 8 groups of 128 threads");
    static_assert(!BUCKET || (FUSED && ITEMS <= 8), "bucket scatter: the fused shape below kBucketMaxN");
    constexpr uint32_t kTileKeys = THREADS * ITEMS;
    constexpr uint32_t kWaves = THREADS / kWave;
    // small sorts: the scatter is a few hundred KB, not worth two barriers — unless the pass also finds the run
    // edges (below), which needs every key's neighbours in output order
    const bool reorder = ITEMS > 2 || edges != nullptr;
    const uint32_t tile = blockIdx.x;
    const uint32_t wid = threadIdx.x / kWave;
    const uint32_t lane = lane_id();
    zero_wave_hist<kWaves, THREADS>(L.wave_hist);

    // Each wave owns a contiguous chunk of 64*ITEMS keys; round i covers keys chunk + i*64 + lane.
    // The loads are issued first so that they are in flight during the table sums below.
    const uint32_t tile_base = tile * kTileKeys;
    const uint32_t chunk = tile_base + wid * (kWave * ITEMS);
    // Large tiles are register-bound (16 keys, 16 ranks and the ballot temporaries per lane): their values are loaded
    // late, just before they are placed, instead of being held across the ranking.
    constexpr bool kLateVals = ITEMS >= 8;
    uint32_t key[ITEMS], val[kLateVals ? 1 : ITEMS];
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; i++) {
        const uint32_t idx = chunk + i * kWave + lane;
        key[i] = idx < n ? keys_in[idx] : 0u;
        if constexpr (!kLateVals)
            val[i] = idx < n ? (vals_in ? vals_in[idx] : idx) : 0u;  // vals_in == nullptr: the positions themselves
    }
    // FUSED: counts[t][d] (16-bit); the small-tile variants sum their share of the table now, behind the key loads
    // issued above; for the large-tile variants (ITEMS >= 8, register-bound) the kernel did it before the switch.
    uint32_t glob_base = 0, glob_tot = 0;
    if (FUSED) {
        if constexpr (ITEMS < 8) table_sums_to_lds(spec, counts, tile, (n + kTileKeys - 1) / kTileKeys, L, trace);
    } else if (threadIdx.x < kRadix) {
        glob_tot = totals[threadIdx.x];
        glob_base = counts[(size_t)threadIdx.x * max_tiles + tile];
    }
    __syncthreads();  // A: wave_hist zeroed, partial column sums published
    BRUSH_KTRACE_MARK_VIA(trace, 3, key[0]);
    uint32_t bucket4[BUCKET ? (ITEMS + 3) / 4 : 1] = {};
    if constexpr (BUCKET) {
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; i++) bucket4[i / 4] |= bucket_of(spl, key[i]) << ((i & 3u) * 8u);
    }
    auto digit_of = [&](uint32_t i) -> uint32_t {
        if constexpr (BUCKET) return (bucket4[i / 4] >> ((i & 3u) * 8u)) & 0xFFu;
        else return (key[i] >> shift) & mask;
    };

    // rank of a key among the keys of its digit inside its wave's chunk: < 64 * ITEMS <= 1024.  The large-tile variants
    // are register-bound and keep two ranks per register.
    constexpr bool kPackRanks = ITEMS >= 8;
    uint32_t rank[kPackRanks ? ITEMS / 2 : ITEMS];
    auto rank_of = [&](uint32_t i) -> uint32_t {
        if constexpr (kPackRanks) return (rank[i / 2] >> ((i & 1u) * 16u)) & 0xFFFFu;
        else return rank[i];
    };
    const uint64_t lt = lanemask_lt();
    // digit bits this pass looks at (a 13-bit tile id is sorted as 7 + 6 bits: one and two ballots fewer per key).  Only
    // in the 1024-thread kernel: measured same box, tile sort 30.4 -> 29.6 us at S1 and 74.3 -> 70.9 on the dense scene,
    // but the 512-thread large-sort kernel lost 4 us per sort to the extra scalar branches (c3 386 -> 391).
    const uint32_t nbits = THREADS == kSortThreads ? (uint32_t)__builtin_amdgcn_readfirstlane((int)__popc(mask)) : 8u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; i++) {
        const uint32_t idx = chunk + i * kWave + lane;
        const bool valid = idx < n;
        const uint32_t digit = digit_of(i);
        // the match-any ranking step, claim included, written out: kernel_diff refused claim_rank here (all three
        // scatter kernels are scheduled differently)
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            if (b >= nbits) break;  // wave-uniform
            const bool bit = (digit >> b) & 1u;
            const uint64_t vote = __ballot(valid && bit);
            peers &= bit ? vote : ~vote;
        }
        const uint32_t below = __popcll(peers & lt);
        const uint32_t cnt = __popcll(peers);
        const int leader = valid ? (__ffsll((long long)peers) - 1) : 0;
        uint32_t old = 0;
        if (valid && (int)lane == leader) {
            old = L.wave_hist[wid][digit];
            L.wave_hist[wid][digit] = old + cnt;
        }
        old = __shfl(old, leader, 64);
        if constexpr (kPackRanks) rank[i / 2] = (i & 1u) ? (rank[i / 2] | ((old + below) << 16)) : (old + below);
        else rank[i] = old + below;
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();  // B: every wave's digit counts are final
    // Threads 0..255 (digit d): 16-wave combine (wave_hist[w][d] <- keys of digit d in earlier waves of the tile),
    // the tile's count of d, and the global sums; then both exclusive scans over the digits behind one pair of
    // barriers: (#keys with a smaller digit anywhere) and (start of the digit's run inside the tile).
    uint32_t tile_cnt = 0;
    if (threadIdx.x < kRadix) {
        const uint32_t d = threadIdx.x;
        // wave_hist_to_starts, written out: kernel_diff refused the helper here (other branches in the 1024-thread kernels)
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t t = L.wave_hist[w][d];
            L.wave_hist[w][d] = tile_cnt;
            tile_cnt += t;
        }
        if (FUSED) {
#pragma unroll
            for (uint32_t g = 0; g < kTableGroups; g++) glob_tot += L.part_all()[g][d], glob_base += L.part()[g][d];
        }
    }
    uint32_t smaller = glob_tot, run_start = tile_cnt;
    block_excl_scan256_pair(smaller, run_start, L.wave_tot2);
    if (threadIdx.x < kRadix) {
        L.digit_base[threadIdx.x] = smaller + glob_base;
        L.tile_start[threadIdx.x] = run_start;
        // BUCKET, or a plain pass whose runs are finished per digit (sort_partition_launch by shift): the run starts are published
        if ((BUCKET || bucket_off != nullptr) && tile == 0) {  // tile 0 exists whenever n > 0
            bucket_off[threadIdx.x] = smaller;
            if (threadIdx.x == kRadix - 1) bucket_off[kRadix] = n;
        }
    }
    __syncthreads();  // C
    BRUSH_KTRACE_MARK_VIA(trace, 4, smaller);
    if (!reorder) {
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; i++) {
            const uint32_t idx = chunk + i * kWave + lane;
            if (idx < n) {
                const uint32_t digit = digit_of(i);
                const uint32_t pos = L.digit_base[digit] + L.wave_hist[wid][digit] + rank_of(i);
                if (keys_out) keys_out[pos] = key[i];
                vals_out[pos] = kLateVals ? (vals_in ? vals_in[idx] : idx) : val[kLateVals ? 0 : i];
            }
        }
        return;
    }
    // reorder by digit in LDS (stable: wave order, then rank inside the wave) ...
    if constexpr (kLateVals) {
        // The late values are requested kValBatch at a time: one at a time (each load followed by its LDS write) the 16
        // loads of a lane were 16 dependent round trips — 12.7 of the 24 us a 8192-key tile's workgroup lives at 27 M
        // keys (in-kernel timeline, profiles/r04b_big_sort_timeline.json).  The ballot temporaries are dead by now.
        constexpr uint32_t kValBatch = THREADS == kSortThreads ? 4 : 16;
#pragma unroll
        for (uint32_t i0 = 0; i0 < ITEMS; i0 += kValBatch) {
            uint32_t v[kValBatch];
#pragma unroll
            for (uint32_t u = 0; u < kValBatch; u++) {
                const uint32_t idx = chunk + (i0 + u) * kWave + lane;
                v[u] = idx < n ? (vals_in ? vals_in[idx] : idx) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kValBatch; u++) {
                const uint32_t i = i0 + u, idx = chunk + i * kWave + lane;
                if (idx < n) {
                    const uint32_t digit = digit_of(i);
                    const uint32_t lp = L.tile_start[digit] + L.wave_hist[wid][digit] + rank_of(i);
                    L.keys[lp] = key[i];
                    L.vals[lp] = v[u];
                }
            }
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; i++) {
            const uint32_t idx = chunk + i * kWave + lane;
            if (idx < n) {
                const uint32_t digit = digit_of(i);
                const uint32_t lp = L.tile_start[digit] + L.wave_hist[wid][digit] + rank_of(i);
                L.keys[lp] = key[i];
                L.vals[lp] = val[i];
            }
        }
    }
    __syncthreads();
    BRUSH_KTRACE_MARK_VIA(trace, 2, L.keys[threadIdx.x]);  // (big tiles: mark 2 is free; reordered in LDS, values loaded)
    // ... and write out: position lp of the reordered tile belongs to the run of its digit, so consecutive lanes
    // write consecutive global addresses
    const uint32_t tile_n = min(kTileKeys, n - tile_base);
    // 16 keys per lane at 1024 threads (128 registers): fully unrolled it spills
    constexpr uint32_t kOutUnroll = (ITEMS > 8 && THREADS == kSortThreads) ? 4 : ITEMS;
#pragma unroll kOutUnroll
    for (uint32_t i = 0; i < ITEMS; i++) {
        const uint32_t lp = i * THREADS + threadIdx.x;
        if (lp < tile_n) {
            const uint32_t k = L.keys[lp];
            const uint32_t digit = BUCKET ? bucket_of(spl, k) : (k >> shift) & mask;
            const uint32_t ts = L.tile_start[digit];
            const uint32_t pos = L.digit_base[digit] + (lp - ts);
            if (keys_out) keys_out[pos] = k;  // nullptr: nobody reads the sorted keys (the run edges are found right here)
            vals_out[pos] = L.vals[lp];
            // LAST pass only (edges != nullptr): the keys are in their final order, so the run of equal keys around
            // `pos` is a bin of the caller (GetTileBinEdges, get_tile_bin_edges.wgsl:15-42, without its launch).  A key
            // that differs from its predecessor / successor inside this workgroup's run of the digit proposes
            // [pos, pos + 1) as (start, end); so do the first and the last key of the run, whose outer neighbours belong
            // to other workgroups.  edges[2k] = max ~start, edges[2k+1] = max end over all proposals (zero-initialised
            // by the caller): proposals from the inside of a bin lose against the true edges.
            if (!BUCKET && edges && k < edge_keys) {
                const bool first = lp == ts;
                const bool last = lp + 1 == tile_n || ((L.keys[lp + 1] >> shift) & mask) != digit;
                if (first || L.keys[lp - 1] != k) atomicMax(&edges[2 * k], ~pos);
                if (last || L.keys[lp + 1] != k) atomicMax(&edges[2 * k + 1], pos + 1u);
            }
        }
    }
}

template <bool FUSED, bool BUCKET = false>
__global__ __launch_bounds__(kSortThreads) void k_sort_downsweep(
    const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ vals_in,
    uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ d_n,
    uint32_t max_n, uint32_t shift, uint32_t mask, const uint32_t *__restrict__ counts,
    const uint32_t *__restrict__ totals, uint32_t max_tiles, uint32_t *__restrict__ edges, uint32_t edge_keys,
    const uint32_t *__restrict__ splitters, uint32_t *__restrict__ bucket_off) {
    BRUSH_KTRACE(kTrSortDown, sort_pass_tag(shift, max_n));
    // The first 128 rows of the [tile][digit] count table (every row a sort of up to 2 M keys has) are requested before
    // the element count is known: the table sum used to start only when *d_n had arrived and took two dependent batches
    // of loads (2.2 us of the kernel's 6.5 at 100 k keys, profiles/r04_small_kernel_timeline.json).  The table has at least
    // kSortTargetTiles = 128 rows (sort_max_tiles); rows of tiles that do not exist hold leftovers and are masked in the body.
    uint32_t spec[kSpecRows];
    {
        const uint32_t dp = threadIdx.x & (kRadix / 2 - 1), g8 = threadIdx.x / (kRadix / 2);
#pragma unroll
        for (uint32_t j = 0; j < kSpecRows; j++)
            spec[j] = FUSED ? counts[(size_t)(g8 + kTableGroups * j) * (kRadix / 2) + dp] : 0u;
    }
    const uint32_t *spl = nullptr;
    if constexpr (BUCKET) {
        __shared__ uint32_t spl_s[kRadix];  // read behind the body's barrier A
        if (threadIdx.x < kRadix) spl_s[threadIdx.x] = splitters[threadIdx.x];
        spl = spl_s;
    }
    const uint32_t n = min(*d_n, max_n);
    BRUSH_KTRACE_MARK(1, n);
    const uint32_t items = sort_items(n);
    if ((uint64_t)blockIdx.x * kSortThreads * items >= n) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    DownLds &L = *reinterpret_cast<DownLds *>(lds_raw);
#define BRUSH_DOWN(K, SPEC)                                                                                       \
    downsweep_body<FUSED, K, kSortThreads, DownLds, BUCKET>(keys_in, vals_in, keys_out, vals_out, n, shift, mask,  \
                                                            counts, totals, max_tiles, edges, edge_keys, L, SPEC, \
                                                            BRUSH_KTRACE_REF, spl, bucket_off)
    if (items >= 8) {  // block-uniform
        // large tiles are register-bound: the table sums are formed here, before their 8 / 16 keys per lane are live
        table_sums_to_lds(spec, counts, blockIdx.x, (n + kSortThreads * items - 1) / (kSortThreads * items), L,
                          BRUSH_KTRACE_REF);
        const uint32_t none[kSpecRows] = {};
        if (BUCKET || items == 8) BRUSH_DOWN(8, none);  // BUCKET: n <= kBucketMaxN never selects 16
        else if constexpr (!BUCKET) BRUSH_DOWN(16, none);
        return;
    }
    switch (items) {
        case 1: BRUSH_DOWN(1, spec); break;
        case 2: BRUSH_DOWN(2, spec); break;
        default: BRUSH_DOWN(4, spec); break;
    }
#undef BRUSH_DOWN
}

// Large sorts: one 8192-key tile per 512-thread workgroup, two workgroups per CU.
__global__ __launch_bounds__(kBigThreads) void k_sort_downsweep_big(
    const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ vals_in,
    uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ d_n,
    uint32_t max_n, uint32_t shift, uint32_t mask, const uint32_t *__restrict__ counts,
    const uint32_t *__restrict__ totals, uint32_t max_tiles, uint32_t *__restrict__ edges, uint32_t edge_keys) {
    BRUSH_KTRACE(kTrSortDownBig, shift | ((shift ? 1u : 0u) << 24));
    const uint32_t n = min(*d_n, max_n);
    BRUSH_KTRACE_MARK(1, n);
    if ((uint64_t)blockIdx.x * kBigTileKeys >= n) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    DownLdsBig &L = *reinterpret_cast<DownLdsBig *>(lds_raw);
    const uint32_t no_spec[kSpecRows] = {};
    downsweep_body<false, kBigTileKeys / kBigThreads, kBigThreads>(keys_in, vals_in, keys_out, vals_out, n, shift,
                                                                   mask, counts, totals, max_tiles, edges, edge_keys, L,
                                                                   no_spec, BRUSH_KTRACE_REF);
}

__global__ void k_sort_copy(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ vals_in,
                            uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                            const uint32_t *__restrict__ d_n, uint32_t max_n) {
    const uint32_t n = min(*d_n, max_n);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        keys_out[i] = keys_in[i];
        vals_out[i] = vals_in ? vals_in[i] : i;
    }
}

// The 1024- and 512-thread scatter kernels hold a whole tile in dynamic LDS.
hipError_t enable_downsweep_lds() {
    static std::atomic<int> done[kMaxDevices];
    return enable_big_lds(done, {{reinterpret_cast<const void *>(&k_sort_downsweep<true>), sizeof(DownLds)},
                                 {reinterpret_cast<const void *>(&k_sort_downsweep_big), sizeof(DownLdsBig)},
                                 {reinterpret_cast<const void *>(&k_sort_downsweep<true, true>), sizeof(DownLds)}});
}

}  // namespace

size_t sort_workspace_bytes(uint32_t max_n) { return carve_sort(nullptr, max_n).bytes; }

hipError_t sort_launch(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                       uint32_t *vals_out, const uint32_t *d_n, uint32_t max_n, uint32_t bits, void *ws,
                       hipStream_t s, uint32_t *edges, uint32_t edge_keys) {
    if (max_n == 0) return hipSuccess;
    if (edges && bits == 0) return hipErrorInvalidValue;  // the edges come out of the last pass
    if (!keys_out && (bits == 0 || bits > 16)) return hipErrorInvalidValue;  // only the LAST of <= 2 passes may drop its keys
    const SortWs w = carve_sort(ws, max_n);
    const uint32_t total_bits = 4u * ((bits + 3u) / 4u);  // brush-sort/src/lib.rs:58
    const uint32_t passes = (total_bits + 7u) / 8u;
    if (passes == 0) {
        hipLaunchKernelGGL(k_sort_copy, dim3(min(w.max_tiles * 4u, 2048u)), dim3(256), 0, s, keys_in, vals_in,
                           keys_out, vals_out, d_n, max_n);
        return hipGetLastError();
    }
    const hipError_t lds = enable_downsweep_lds();
    if (lds != hipSuccess) return lds;
    const bool fused = sort_is_fused(max_n);
    const uint32_t *src_k = keys_in, *src_v = vals_in;
    // Internal callers that bound the key values (edge_keys: every key < edge_keys, the tile sort) get the significant
    // bits split evenly over the passes instead of 8 + the rest: a 13-bit tile id is sorted as 7 + 6 bits, so the first
    // pass scatters into 128 runs per tile instead of 256 (runs twice as long: fewer partial lines written).  Same
    // result: the bits above the bound are zero in every key.
    uint32_t even_width = 0;
    if (edge_keys > 1u) {
        const uint32_t sig = significant_bits(edge_keys - 1u);
        if (sig <= total_bits) even_width = (sig + passes - 1u) / passes;
    }
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = even_width ? p * even_width : p * 8u;
        const uint32_t width = even_width ? even_width : min(8u, total_bits - shift);
        const uint32_t mask = (1u << width) - 1u;
        const bool to_out = ((passes - 1 - p) % 2u) == 0;
        uint32_t *dst_k = to_out ? keys_out : w.tmp_keys;  // keys_out may be nullptr: the last pass then writes no keys
        uint32_t *dst_v = to_out ? vals_out : w.tmp_vals;
        uint32_t *pass_edges = p + 1 == passes ? edges : nullptr;
        hipLaunchKernelGGL((fused ? k_sort_upsweep<true, false> : k_sort_upsweep<false, false>), dim3(w.max_tiles),
                           dim3(kSortThreads), 0, s, src_k, d_n, max_n, shift, mask, w.counts, w.max_tiles, nullptr);
        if (fused) {
            hipLaunchKernelGGL(k_sort_downsweep<true>, dim3(w.max_tiles), dim3(kSortThreads), sizeof(DownLds), s, src_k,
                               src_v, dst_k, dst_v, d_n, max_n, shift, mask, w.counts, w.totals, w.max_tiles, pass_edges,
                               edge_keys, nullptr, nullptr);
        } else {
            hipLaunchKernelGGL(k_sort_scan, dim3(kRadix), dim3(256), 0, s, w.counts, d_n, max_n, w.max_tiles, w.totals);
            hipLaunchKernelGGL(k_sort_downsweep_big, dim3(w.max_tiles), dim3(kBigThreads), sizeof(DownLdsBig), s,
                               src_k, src_v, dst_k, dst_v, d_n, max_n, shift, mask, w.counts, w.totals, w.max_tiles,
                               pass_edges, edge_keys);
        }
        src_k = dst_k;
        src_v = dst_v;
    }
    return hipGetLastError();
}

hipError_t sort_partition_launch(const uint32_t *keys_in, const uint32_t *vals_in, const uint32_t *d_n, uint32_t max_n,
                                 const SortWs &w, hipStream_t s, bool by_splitters, uint32_t shift) {
    const hipError_t lds = enable_downsweep_lds();
    if (lds != hipSuccess) return lds;
    // the BUCKET instantiations take the plain ones' arguments: one argument list, the kernels chosen here
    const auto count = by_splitters ? k_sort_upsweep<true, true> : k_sort_upsweep<true, false>;
    const auto scatter = by_splitters ? k_sort_downsweep<true, true> : k_sort_downsweep<true, false>;
    uint32_t *const spl = by_splitters ? w.splitters : nullptr, *const no_edges = nullptr;
    hipLaunchKernelGGL(count, dim3(w.max_tiles), dim3(kSortThreads), 0, s, keys_in, d_n, max_n, shift, kRadix - 1u,
                       w.counts, w.max_tiles, spl);
    hipLaunchKernelGGL(scatter, dim3(w.max_tiles), dim3(kSortThreads), sizeof(DownLds), s, keys_in, vals_in, w.tmp_keys,
                       w.tmp_vals, d_n, max_n, shift, kRadix - 1u, w.counts, w.totals, w.max_tiles, no_edges, 0u,
                       (const uint32_t *)spl, w.bucket_off);
    return hipGetLastError();
}

}  // namespace brush

using namespace brush;

extern "C" int brush_radix_argsort_workspace_size(uint32_t max_n, size_t *bytes) {
    if (!bytes) return BRUSH_ERR_INVALID_ARG;
    *bytes = sort_workspace_bytes(max_n);
    return BRUSH_OK;
}

extern "C" int brush_radix_argsort_u32(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                                       uint32_t *vals_out, const uint32_t *d_n, uint32_t max_n,
                                       uint32_t sorting_bits, void *workspace, size_t workspace_bytes,
                                       brush_stream_t stream) {
    if (sorting_bits > 32) return BRUSH_ERR_INVALID_ARG;  // brush-sort/src/lib.rs:38-39
    if (max_n == 0) return BRUSH_OK;
    if (!keys_in || !vals_in || !keys_out || !vals_out || !d_n || !workspace) return BRUSH_ERR_INVALID_ARG;
    if (keys_in == keys_out || vals_in == vals_out) return BRUSH_ERR_INVALID_ARG;
    if (workspace_bytes < sort_workspace_bytes(max_n)) return BRUSH_ERR_WORKSPACE_SMALL;
    BRUSH_HIP_CHECK(sort_launch(keys_in, vals_in, keys_out, vals_out, d_n, max_n, sorting_bits, workspace,
                                static_cast<hipStream_t>(stream)));
    return BRUSH_OK;
}
