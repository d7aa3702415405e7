// profiler.hip — opt-in stage timing of the render passes (brush_profiler_*, brush_stage_name) and, in the development
// build only (make trace), the host side of the in-kernel timeline ring of trace.hpp.  No kernel.
#include "render_host.hpp"
#include "trace.hpp"

// One pass as its profiler records it: events[0] = the pass starts, events[1 + i] = end of its stage i.
struct PassRecord {
    int stages;
    hipEvent_t events[BRUSH_STAGE_RASTERIZE + 2];  // (the forward is the longer pass)
    uint32_t mask;   // events recorded by the last pass (a stage without a launch records none)
    bool recorded;   // a whole pass has been recorded
};

struct BrushProfiler {
    static constexpr int kFwdStages = BRUSH_STAGE_RASTERIZE + 1;
    PassRecord pass[2] = {{kFwdStages}, {BRUSH_NUM_STAGES - kFwdStages}};  // indexed by brush::StagePass
    int stop_after = -1;  // brush_profiler_stop_after: the pass ends behind this stage, no events
};

namespace brush {

static thread_local BrushProfiler *g_prof = nullptr;

bool stop_behind(int stage) { return g_prof && g_prof->stop_after == stage; }

void mark_stage(StagePass pass, hipStream_t s, int idx) {
    if (g_prof && g_prof->stop_after < 0) {
        PassRecord &r = g_prof->pass[pass];
        if (idx == 0) r.mask = 0;
        (void)hipEventRecord(r.events[idx], s);
        r.mask |= 1u << idx;
        if (idx == r.stages) r.recorded = true;
    }
}

}  // namespace brush

using namespace brush;

extern "C" int brush_profiler_create(BrushProfiler **out) {
    if (!out) return BRUSH_ERR_INVALID_ARG;
    BrushProfiler *p = new BrushProfiler();
    for (auto &r : p->pass)
        for (int i = 0; i <= r.stages; i++) BRUSH_HIP_CHECK(hipEventCreate(&r.events[i]));
    *out = p;
    return BRUSH_OK;
}

extern "C" void brush_profiler_destroy(BrushProfiler *p) {
    if (!p) return;
    if (g_prof == p) g_prof = nullptr;
    for (auto &r : p->pass)
        for (int i = 0; i <= r.stages; i++) (void)hipEventDestroy(r.events[i]);
    delete p;
}

extern "C" void brush_profiler_attach(BrushProfiler *p) { g_prof = p; }

extern "C" int brush_profiler_read(BrushProfiler *p, float *h_ms) {
    if (!p || !h_ms) return BRUSH_ERR_INVALID_ARG;
    for (int i = 0; i < BRUSH_NUM_STAGES; i++) h_ms[i] = 0.0f;
    // a stage that launched nothing recorded no event: it reads 0 and the next stage is measured from the last event
    for (const auto &r : p->pass) {
        if (r.recorded) {
            BRUSH_HIP_CHECK(hipEventSynchronize(r.events[r.stages]));
            int last = 0;
            for (int i = 0; i < r.stages; i++) {
                if (!((r.mask >> (i + 1)) & 1u)) continue;
                BRUSH_HIP_CHECK(hipEventElapsedTime(&h_ms[i], r.events[last], r.events[i + 1]));
                last = i + 1;
            }
        }
        h_ms += r.stages;  // the backward's stages follow the forward's
    }
    return BRUSH_OK;
}

extern "C" int brush_profiler_stop_after(BrushProfiler *p, int stage) {
    if (!p || stage < -1 || stage >= BRUSH_NUM_STAGES) return BRUSH_ERR_INVALID_ARG;
    p->stop_after = stage;
    return BRUSH_OK;
}

extern "C" const char *brush_stage_name(int stage) {
    static const char *names[BRUSH_NUM_STAGES] = {"project_cull", "depth_sort", "project_visible", "prefix_sum",
                                                  "map_intersects", "tile_sort", "tile_bins", "rasterize",
                                                  "bwd_zero", "rasterize_bwd", "project_bwd"};
    return (stage >= 0 && stage < BRUSH_NUM_STAGES) ? names[stage] : "?";
}

#ifdef BRUSH_TRACE
// ---- development build only (make trace): the in-kernel timeline ring of trace.hpp --------------------------
#include <vector>
namespace brush {
static std::vector<void (*)(TraceRec *, uint32_t *)> &trace_attachers() {
    static std::vector<void (*)(TraceRec *, uint32_t *)> v;
    return v;
}
void trace_register(void (*attach)(TraceRec *, uint32_t *)) { trace_attachers().push_back(attach); }
static TraceRec *g_trace_ring = nullptr;
static uint32_t *g_trace_cursor = nullptr;
}  // namespace brush
// Allocates the ring on first use, points every translation unit at it and resets the cursor.
extern "C" int brush_debug_trace_begin(void) {
    if (!g_trace_ring) {
        BRUSH_HIP_CHECK(hipMalloc(&g_trace_ring, sizeof(TraceRec) * kTraceCap));
        BRUSH_HIP_CHECK(hipMalloc(&g_trace_cursor, 256));
        for (auto f : trace_attachers()) f(g_trace_ring, g_trace_cursor);
    }
    BRUSH_HIP_CHECK(hipMemset(g_trace_ring, 0, sizeof(TraceRec) * kTraceCap));
    BRUSH_HIP_CHECK(hipDeviceSynchronize());
    return BRUSH_OK;
}
// Copies up to max_records 64-byte records to the host; returns how many were written (< 0: error).
extern "C" long brush_debug_trace_read(void *out, size_t max_records) {
    if (!g_trace_ring || !out) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    uint32_t n = kTraceCap;  // slots nobody wrote stay zero (t[0] == 0)
    if (n > max_records) n = (uint32_t)max_records;
    if (n && hipMemcpy(out, g_trace_ring, sizeof(TraceRec) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return (long)n;
}
#endif
