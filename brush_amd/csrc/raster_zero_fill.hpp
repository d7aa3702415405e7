// raster_zero_fill.hpp — device side of the zero-fill the compositing backward carries in passing (ZeroFill,
// internal.hpp; the host side is make_zero_fill, rasterize_bwd.hip).  Provides the cursor of a wave's share of the
// block sequence (FillCursor), fill_begin (a wave's share), fill_seek, fill_step (one block) and fill_take (n blocks).
// The pacing of the steps over the records a wave walks (fill_num, fill_den, fill_budget, fill_rate, fill_acc) and the
// draining loop (fill_rest) are written out in k_rasterize_backward_quad, rasterize_bwd.hip.
#pragma once
#include "raster_common.hpp"

namespace brush {
namespace {

// A wave owes `quota` consecutive KiB blocks of the launch-wide block sequence (the dense gradient arrays laid end to
// end); the cursor lives in SGPRs, one block is one fire-and-forget 16-byte store per lane.  Only the last block of an
// array looks at chunk counts (partial block, up to three trailing floats).
struct FillCursor {
    float4 *ptr;              // the next block of the current array
    uint32_t block;           // its index in the block sequence
    uint32_t seg, seg_left;   // current array; blocks left in it, this one included
    uint32_t quota;           // blocks this wave still owes
};
__device__ __forceinline__ void fill_seek(const ZeroFill &zf, FillCursor &c) {
    uint32_t seg = 0;
#pragma unroll
    for (uint32_t i = 1; i < kFillSegs; i++) seg = c.block >= zf.first_block[i] ? i : seg;  // empty arrays are passed over
    c.seg = seg;
    c.seg_left = zf.first_block[seg + 1] - c.block;
    c.ptr = reinterpret_cast<float4 *>(zf.base[seg]) + (size_t)(c.block - zf.first_block[seg]) * kWave;
}
__device__ __forceinline__ void fill_step(const ZeroFill &zf, FillCursor &c, uint32_t lane) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.seg_left > 1u) {
        // streaming store: written once, far larger than the L2s (measured against ordinary stores at 1 M splats:
        // compositing backward 126 vs 133 us, the VJP kernel behind it 25 vs 34 us)
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f nz = {0.f, 0.f, 0.f, 0.f};
        __builtin_nontemporal_store(nz, reinterpret_cast<v4f *>(c.ptr + lane));
    } else {
        const uint32_t chunk = (zf.first_block[c.seg + 1] - zf.first_block[c.seg] - 1u) * kWave + lane;
        const uint32_t full = zf.full[c.seg];
        if (chunk < full) {
            c.ptr[lane] = z4;
        } else if (chunk == full) {
            float *t = reinterpret_cast<float *>(c.ptr + lane);
            for (uint32_t d = 0; d < zf.tail[c.seg]; d++) t[d] = 0.0f;
        }
    }
    c.ptr += kWave;
    c.block++;
    c.quota--;
    if (--c.seg_left == 0u && c.quota != 0u) fill_seek(zf, c);
}

// This wave's share of the block sequence (every launched wave has one, tile or not): unit `unit` of `units`.
__device__ __forceinline__ void fill_begin(const ZeroFill &zf, FillCursor &c, uint32_t unit, uint32_t units) {
    c.quota = 0u;
    if (zf.active()) {
        const uint32_t total = zf.first_block[kFillSegs], per = ceil_div(total, units);
        c.block = min(unit * per, total);
        c.quota = min(per, total - c.block);
        if (c.quota != 0u) fill_seek(zf, c);
    }
}
// Takes n steps (n <= c.quota) and leaves n at 0.
__device__ __forceinline__ void fill_take(const ZeroFill &zf, FillCursor &c, uint32_t lane, uint32_t &n) {
    for (; n != 0u; n--) fill_step(zf, c, lane);
}

}  // namespace
}  // namespace brush
