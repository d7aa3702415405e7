// depth_sort.hip — the depth sort of clouds up to kBucketMaxN = 2^20 splats: three launches instead of the eight of
// four LSD passes.
//
// ONE count + scatter pair (sort_partition_launch, radix_sort.hip) partitions the keys into kRadix key-range buckets:
// the digit of that pass is "bucket of key", a binary search over 255 splitters picked from a sorted fixed-stride
// sample.  Then one workgroup per bucket (k_sort_bucket_finish, here) finishes its bucket in LDS, where a pass costs a
// barrier and not a kernel boundary (~4 us each at 100 k keys).  A bucket's keys agree in their high bits, so the
// workgroup sorts only the bits in which they differ.  Buckets that do not fit in LDS (long runs of equal keys, a spike
// the sample missed) run the same passes between their own ranges of two global buffers.  sort_common.hpp states what
// the scatter leaves for the finish kernel.  Larger clouds run sort_launch.
#include "sort_common.hpp"

namespace brush {
namespace {

constexpr uint32_t kBucketLdsKeys = 8192;  // pairs a finish workgroup sorts in LDS; larger buckets: global passes
static_assert(kBucketMaxN / kRadix <= kBucketLdsKeys / 2, "evenly spread keys fill a bucket's LDS at most half");

struct FinishLds {
    uint32_t keys[2][kBucketLdsKeys];
    uint32_t vals[2][kBucketLdsKeys];
    uint32_t wave_hist[kSortWaves][kRadix];
    uint32_t wave_tot2[4][2];
    uint32_t or_and[kSortWaves][2];
};
static_assert(sizeof(FinishLds) <= 160 * 1024, "one finish workgroup per CU");

// One stable counting pass of the whole workgroup over `cnt` pairs, src -> dst (LDS or this bucket's own range of a
// global buffer) by the digit (key >> shift) & mask.  Every wave owns a contiguous chunk: it counts its digits, the
// counts are scanned in (digit, wave) order, then it walks the chunk again in index order and ranks 64 keys at a time
// with match-any ballots, so nothing per key stays in registers and every loop is bounded by cnt.  Ends with a barrier
// (workgroup-scope release / acquire: the next pass reads what this one wrote, also in global memory).
__device__ __forceinline__ void bucket_pass(const uint32_t *sk, const uint32_t *sv, uint32_t *dk, uint32_t *dv,
                                            uint32_t cnt, uint32_t shift, uint32_t mask, FinishLds &L) {
    const uint32_t wid = threadIdx.x / kWave, lane = lane_id();
    zero_wave_hist<kSortWaves, kSortThreads>(L.wave_hist);
    __syncthreads();
    const uint32_t per_wave = ceil_div(cnt, kSortThreads) * kWave;  // cnt <= kBucketMaxN
    const uint32_t beg = min(cnt, wid * per_wave), end = min(cnt, beg + per_wave);
    for (uint32_t i = beg + lane; i < end; i += kWave) atomicAdd(&L.wave_hist[wid][(sk[i] >> shift) & mask], 1u);
    __syncthreads();
    uint32_t tot = 0, unused = 0;
    if (threadIdx.x < kRadix) wave_hist_to_starts<kSortWaves>(L.wave_hist, threadIdx.x, tot);
    block_excl_scan256_pair(tot, unused, L.wave_tot2);  // tot: pairs of a smaller digit
    if (threadIdx.x < kRadix) {
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; w++) L.wave_hist[w][threadIdx.x] += tot;
    }
    __syncthreads();
    const uint64_t lt = lanemask_lt();
    for (uint32_t i0 = beg; i0 < end; i0 += kWave) {  // wave-uniform
        const uint32_t i = i0 + lane;
        const bool valid = i < end;
        const uint32_t k = valid ? sk[i] : 0u, v = valid ? sv[i] : 0u;
        const uint32_t digit = (k >> shift) & mask;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t vote = __ballot(valid && bit);
            peers &= bit ? vote : ~vote;
        }
        const uint32_t pos = claim_rank(peers, valid, lane, lt, &L.wave_hist[wid][digit]);
        if (valid) {
            dk[pos] = k;
            dv[pos] = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
}

// Workgroup b sorts bucket b = pairs [off[b], off[b + 1]) of the scatter's output (tmp) by key, stable, into the same
// range of the final buffers.  The bucket's keys agree in every bit above the highest one in which any two of them
// differ (OR ^ AND over the bucket), so only the bits below it are sorted, split evenly over ceil(bits / 8) passes.
//   * up to kBucketLdsKeys pairs: loaded once, passes between two LDS images, the last one writes the result;
//   * more (long runs of equal keys, a spike the sample missed): the same passes between the bucket's range of tmp
//     and of out, an odd number of them so that the last one lands in out.  Slow, and alone in its own range.
// No workgroup waits for another one.
__global__ __launch_bounds__(kSortThreads) void k_sort_bucket_finish(uint32_t *tmp_keys, uint32_t *tmp_vals,
                                                                    uint32_t *keys_out, uint32_t *vals_out,
                                                                    const uint32_t *__restrict__ d_n, uint32_t max_n,
                                                                    const uint32_t *__restrict__ bucket_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    FinishLds &L = *reinterpret_cast<FinishLds *>(lds_raw);
    // the finish preamble of sort_common.hpp's contract, as in k_tile_bucket_finish: kernel_diff refused a shared helper
    const uint32_t off0 = bucket_off[blockIdx.x], off1 = bucket_off[blockIdx.x + 1];
    const uint32_t n = min(*d_n, max_n);
    if (n == 0) return;  // no scatter workgroup ran: the offsets are leftovers
    const uint32_t start = min(off0, n), stop = min(off1, n);
    if (stop <= start) return;
    const uint32_t cnt = stop - start;
    const bool in_lds = cnt <= kBucketLdsKeys;  // block-uniform
    tmp_keys += start, tmp_vals += start, keys_out += start, vals_out += start;
    uint32_t k_or = 0, k_and = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < cnt; i += kSortThreads) {
        const uint32_t k = tmp_keys[i];
        k_or |= k, k_and &= k;
        if (in_lds) L.keys[0][i] = k, L.vals[0][i] = tmp_vals[i];
    }
#pragma unroll
    for (uint32_t m = kWave / 2; m; m >>= 1) {
        k_or |= (uint32_t)__shfl_xor((int)k_or, (int)m, (int)kWave);
        k_and &= (uint32_t)__shfl_xor((int)k_and, (int)m, (int)kWave);
    }
    if (lane_id() == 0) L.or_and[threadIdx.x / kWave][0] = k_or, L.or_and[threadIdx.x / kWave][1] = k_and;
    __syncthreads();
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; w++) k_or |= L.or_and[w][0], k_and &= L.or_and[w][1];
    const uint32_t differ = k_or ^ k_and;
    const uint32_t bits = differ ? 32u - (uint32_t)__clz((int)differ) : 0u;
    uint32_t passes = (bits + 7u) / 8u;
    if (in_lds) {
        if (passes == 0) {  // one key value: the scatter's order is the result
            for (uint32_t i = threadIdx.x; i < cnt; i += kSortThreads) keys_out[i] = L.keys[0][i], vals_out[i] = L.vals[0][i];
            return;
        }
        const uint32_t width = (bits + passes - 1u) / passes, mask = (1u << width) - 1u;
        uint32_t p = 0;
        for (; p + 1 < passes; p++)
            bucket_pass(L.keys[p & 1u], L.vals[p & 1u], L.keys[(p + 1u) & 1u], L.vals[(p + 1u) & 1u], cnt, p * width,
                        mask, L);
        bucket_pass(L.keys[p & 1u], L.vals[p & 1u], keys_out, vals_out, cnt, p * width, mask, L);
        return;
    }
    passes |= 1u;  // 1, 3 or 5: tmp -> out -> tmp ... -> out (a pass over bits that agree is a stable copy)
    const uint32_t width = (bits + passes - 1u) / passes, mask = (1u << width) - 1u;  // <= 8; 5 passes: 7 bits, shifts <= 28
    for (uint32_t p = 0; p < passes; p++) {
        const bool to_out = (p & 1u) == 0;
        bucket_pass(to_out ? tmp_keys : keys_out, to_out ? tmp_vals : vals_out, to_out ? keys_out : tmp_keys,
                    to_out ? vals_out : tmp_vals, cnt, p * width, mask, L);
    }
}

}  // namespace

bool depth_sort_uses_buckets(uint32_t max_n) { return max_n <= kBucketMaxN; }

hipError_t depth_sort_launch(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                             const uint32_t *d_n, uint32_t max_n, void *ws, hipStream_t s) {
    if (!depth_sort_uses_buckets(max_n)) return sort_launch(keys_in, vals_in, keys_out, vals_out, d_n, max_n, 32, ws, s);
    if (max_n == 0) return hipSuccess;
    if (!keys_out) return hipErrorInvalidValue;
    static std::atomic<int> done[kMaxDevices];
    hipError_t e = enable_big_lds(done, {{reinterpret_cast<const void *>(&k_sort_bucket_finish), sizeof(FinishLds)}});
    const SortWs w = carve_sort(ws, max_n);
    if (e == hipSuccess) e = sort_partition_launch(keys_in, vals_in, d_n, max_n, w, s, true, 0u);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sort_bucket_finish, dim3(kRadix), dim3(kSortThreads), sizeof(FinishLds), s, w.tmp_keys,
                       w.tmp_vals, keys_out, vals_out, d_n, max_n, (const uint32_t *)w.bucket_off);
    return hipGetLastError();
}

}  // namespace brush
