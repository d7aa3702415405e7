// ssim_dev.hpp — the pieces of the separable SSIM blur shared by the training loss (train_step.hip) and the
// metrics-only evaluation pass (eval.hip): the window and its geometry, the wave-uniform-row loads (ground truth as f32
// or u8), the window dispatch.  The wave reduction is tree_sum of fixed_sum.hpp.
#pragma once
#include "fixed_sum.hpp"
#include "internal.hpp"

namespace brush {
namespace {

// The SSIM window: TrainConfig::ssim_window_size (train.rs:63, default 11); odd sizes 3..15 are compiled.  For an odd
// window 2m+1 the zero padding is div_ceil(window, 2) = m+1 (ssim.rs:49), so the SSIM map is (h+2) x (w+2) whatever
// the size.
constexpr int kMaxWin = 15;
template <int WIN>
struct Geo {
    static constexpr int kPad = (WIN + 1) / 2;      // div_ceil(WIN, 2)
    static constexpr int kOutCols = 64 - (WIN - 1);  // columns a wave produces: 64 lanes minus the halo
    static constexpr int kSegRows = 3 * WIN + 1;     // rows a block produces: + (WIN - 1) halo = 4 * WIN marched rows
    static constexpr int kOff = WIN - 1 - kPad;
};
constexpr int kRowBuf = 80;     // floats per LDS row buffer (lane + kMaxWin - 1 taps < 80)
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct Window {
    float g[kMaxWin];
};

// Element at a wave-uniform base plus a per-lane BYTE offset below 4 GiB: global_load/store with an SGPR base and a
// 32-bit VGPR offset, no 64-bit vector address arithmetic.
__device__ __forceinline__ float ld_off(const float *base, uint32_t byte_off) {
    return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + byte_off);
}

// One ground-truth sample at a wave-uniform row plus a per-lane BYTE offset (element index * sizeof(GT)).  u8 is
// (float)b / 255.0f, a correctly rounded division as image_to_tensor / to_rgb32f compute it (a reciprocal multiply
// gives different bits), so a u8 target reaches the arithmetic with the bits of an f32 target holding u8 / 255.
__device__ __forceinline__ float ld_gt_off(const float *row, uint32_t byte_off) { return ld_off(row, byte_off); }
__device__ __forceinline__ float ld_gt_off(const uint8_t *row, uint32_t byte_off) { return (float)row[byte_off] / 255.0f; }
// The same at a per-lane element index.
template <typename GT>
__device__ __forceinline__ float ld_gt(const GT *row, uint32_t idx) { return ld_gt_off(row, idx * (uint32_t)sizeof(GT)); }

// LDS traffic inside one wave is in order; this only stops the compiler from moving accesses.
// A fence would also wait for the prefetched global loads, so this is a pure compiler barrier.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// The normalised 1-D Gaussian of ssim.rs:7-14 (sigma 1.5); the 2-D window is outer(g, g).
Window make_window(int n) {
    Window win;
    float sum = 0.0f;
    for (int i = 0; i < kMaxWin; i++) win.g[i] = 0.0f;
    for (int i = 0; i < n; i++) {
        const float d = (float)i - (float)(n / 2);
        win.g[i] = expf(-(d * d) / (2.0f * 1.5f * 1.5f));  // ssim.rs:7-14
        sum += win.g[i];
    }
    for (int i = 0; i < n; i++) win.g[i] /= sum;
    return win;
}

inline bool window_ok(uint32_t n) { return n >= 3 && n <= (uint32_t)kMaxWin && (n & 1u); }
// Runtime window (window_ok) -> the WIN template argument of a kernel launch: f receives an IntC<WIN>, as
// dispatch_degree (internal.hpp).
template <typename F>
void dispatch_window(uint32_t n, F &&f) {
    switch (n) {
        case 3: return f(IntC<3>{});
        case 5: return f(IntC<5>{});
        case 7: return f(IntC<7>{});
        case 9: return f(IntC<9>{});
        case 11: return f(IntC<11>{});
        case 13: return f(IntC<13>{});
        default: return f(IntC<15>{});
    }
}

}  // namespace
}  // namespace brush
