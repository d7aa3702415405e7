// rasterize_dev.inc — every development / test-only hook of the compositing backward, so that rasterize_bwd.hip reads as
// the product kernel.  Included twice by rasterize_bwd.hip (BRUSH_DEV_SECTION 1: device helpers inside namespace brush::{};
// 2: the host-side reader at file scope).  In the product build every hook below is the identity:
//   dev_vva()          vis * v_alpha                 BRUSH_INJECT_VVA_ULPS=<n> (build/libbrush_hip_inject.so, tests/
//                                                    test_gpu_gate.py): a one-signed error of n eps32 per gradient term
//   dev_flush()        one hardware float atomic     BRUSH_ELIM_NO_ATOMICS: elimination timing, everything but the atomic
//   dev_skip_reduce()  false                         BRUSH_ELIM_NO_REDUCE: elimination timing, no staging / reduction / flush
//   BRUSH_DEV_BWD_TRACE  nothing                     BRUSH_BWD_TRACE (make trace): per-wave timeline, tools/debug/bwd_timeline.py
#if BRUSH_DEV_SECTION == 1

__device__ __forceinline__ float dev_vva(float vis, float v_alpha) {
#ifdef BRUSH_INJECT_VVA_ULPS
    return fmaf(fabsf(vis * v_alpha), BRUSH_INJECT_VVA_ULPS * 5.9604645e-8f, vis * v_alpha);
#else
    return vis * v_alpha;
#endif
}

__device__ __forceinline__ void dev_flush(float *dst, float val) {
#ifdef BRUSH_ELIM_NO_ATOMICS
    if (val == 12345.678f) *dst = val;
#else
    if (val != 0.0f) unsafeAtomicAdd(dst, val);
#endif
}

template <bool DET, uint32_t N>
__device__ __forceinline__ bool dev_skip_reduce(const float (&g)[N], float *v_compact, uint32_t lane) {
#ifdef BRUSH_ELIM_NO_REDUCE
    if (!DET) {
        if (g[0] + g[1] + g[2] + g[3] + g[4] + g[5] + g[6] + g[7] + g[8] == 12345.678f) v_compact[lane] = g[0];
        return true;
    }
#endif
    (void)g, (void)v_compact, (void)lane;
    return false;
}

#ifdef BRUSH_BWD_TRACE
__device__ uint64_t g_bwd_trace[16384 * 4];
struct BwdTrace {
    uint64_t t0;
    uint32_t wid, recs;
    __device__ ~BwdTrace() {
        if (lane_id() == 0 && wid < 16384u) {
            uint32_t hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_bwd_trace[wid * 4 + 0] = t0;
            g_bwd_trace[wid * 4 + 1] = (uint64_t)wall_clock64();
            g_bwd_trace[wid * 4 + 2] = ((uint64_t)xcc << 32) | hwid;
            g_bwd_trace[wid * 4 + 3] = ((uint64_t)1 << 48) | ((uint64_t)recs << 24);
        }
    }
};
#define BRUSH_DEV_BWD_TRACE(wave_id, recs) const BwdTrace brush_bwd_trace_{(uint64_t)wall_clock64(), (wave_id), (recs)}
#else
#define BRUSH_DEV_BWD_TRACE(wave_id, recs) ((void)0)
#endif

#elif BRUSH_DEV_SECTION == 2

#ifdef BRUSH_BWD_TRACE
extern "C" int brush_debug_read_bwd_trace(uint64_t *out, size_t words) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(brush::g_bwd_trace), words * 8);
}
#endif

#endif
#undef BRUSH_DEV_SECTION
