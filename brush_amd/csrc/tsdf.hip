// tsdf.hip — mesh export: brush_tsdf_integrate fuses rendered depth maps into a dense truncated signed distance volume,
// brush_tsdf_mesh_count / brush_tsdf_mesh_emit cut an indexed triangle mesh out of it by marching tetrahedra on the
// Kuhn decomposition (include/brush_hip.h states the arithmetic and the orders).  A load-time tool, not a training
// stage.  One lane per voxel / lattice point / cell, x fastest, so a wave's lanes project to nearby pixels and read
// and write whole lines of one plane; every sum is an integer one lane owns: no atomics, no workspace for the fusion.
// Built WITHOUT FMA contraction: every skip decision must be the one the header's f32 formulas give.
// Roofline: the fusion streams the volume (24 B read per voxel, up to 24 B written) and gathers 20 B per voxel and view
// that passes the frustum test from images the L2 mostly holds; the extraction kernels stream 1-9 B per lattice point
// and gather neighbour words through the L2.
#include "internal.hpp"

#pragma clang fp contract(off)

namespace brush {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxViews = BRUSH_TSDF_MAX_VIEWS;
constexpr uint32_t kViewWords = sizeof(BrushFilterView) / 4;
static_assert(sizeof(BrushFilterView) == 96, "the record is 24 words");
static_assert(sizeof(BrushTsdfGrid) == 32, "the grid is 8 words");

struct ViewPointers {
    BrushTsdfViewData v[kMaxViews];
};

// ---------------------------------------------------------------------------------------------- the case table
// One tetrahedron and one pattern of inside vertices: the triangles, each corner of which is an edge of the cell given
// as (lower cell corner << 3 | slot): the vertex sits on the edge that the lattice point at `lower corner` owns in
// `slot` (offset code slot + 1).  In a Kuhn tetrahedron 0 c 1 c 2 c 3 the corner codes are nested bit sets, so the
// lower corner of an edge is the numerically smaller one.
struct TetCase {
    uint8_t ntri;
    uint8_t edge[6];
    uint8_t pad;
};
struct TetTable {
    TetCase c[6][16];
};

constexpr TetTable make_tet_table() {
    TetTable tab{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; t++) {
        const int tv[4] = {0, 1 << perm[t][0], (1 << perm[t][0]) | (1 << perm[t][1]), 7};
        for (int m = 0; m < 16; m++) {
            int ins[4] = {}, outs[4] = {}, ni = 0, no = 0;
            for (int p = 0; p < 4; p++) {
                if (m >> p & 1) ins[ni++] = p;
                else outs[no++] = p;
            }
            int tri[2][3][2] = {};  // [triangle][corner] = (inside position, outside position)
            int ntri = 0;
            if (ni == 1) {
                ntri = 1;
                for (int k = 0; k < 3; k++) tri[0][k][0] = ins[0], tri[0][k][1] = outs[k];
            } else if (ni == 3) {
                ntri = 1;
                for (int k = 0; k < 3; k++) tri[0][k][0] = ins[k], tri[0][k][1] = outs[0];
            } else if (ni == 2) {
                ntri = 2;
                const int quad[4][2] = {{ins[0], outs[0]}, {ins[0], outs[1]}, {ins[1], outs[1]}, {ins[1], outs[0]}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                for (int f = 0; f < 2; f++)
                    for (int k = 0; k < 3; k++) tri[f][k][0] = quad[pick[f][k]][0], tri[f][k][1] = quad[pick[f][k]][1];
            }
            // from the inside vertices' centroid to the outside ones', times ni * no
            int dir[3] = {};
            for (int a = 0; a < 3; a++) {
                int si = 0, so = 0;
                for (int k = 0; k < ni; k++) si += tv[ins[k]] >> a & 1;
                for (int k = 0; k < no; k++) so += tv[outs[k]] >> a & 1;
                dir[a] = so * ni - si * no;
            }
            TetCase &tc = tab.c[t][m];
            tc.ntri = (uint8_t)ntri;
            for (int f = 0; f < ntri; f++) {
                int P[3][3] = {};  // twice the edge midpoints
                for (int k = 0; k < 3; k++)
                    for (int a = 0; a < 3; a++) P[k][a] = (tv[tri[f][k][0]] >> a & 1) + (tv[tri[f][k][1]] >> a & 1);
                int e1[3] = {}, e2[3] = {};
                for (int a = 0; a < 3; a++) e1[a] = P[1][a] - P[0][a], e2[a] = P[2][a] - P[0][a];
                const int n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                  e1[0] * e2[1] - e1[1] * e2[0]};
                const int dot = n[0] * dir[0] + n[1] * dir[1] + n[2] * dir[2];
                const int order[3] = {0, dot < 0 ? 2 : 1, dot < 0 ? 1 : 2};
                for (int k = 0; k < 3; k++) {
                    const int ca = tv[tri[f][order[k]][0]], cb = tv[tri[f][order[k]][1]];
                    const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
                    tc.edge[f * 3 + k] = (uint8_t)(lo << 3 | ((lo ^ hi) - 1));
                }
            }
        }
    }
    return tab;
}

constexpr TetTable kHostTable = make_tet_table();
static_assert(kHostTable.c[0][0].ntri == 0 && kHostTable.c[5][15].ntri == 0, "no surface without a sign change");
static_assert(kHostTable.c[0][1].ntri == 1 && kHostTable.c[0][3].ntri == 2 && kHostTable.c[0][7].ntri == 1, "");
// corner 0 alone inside: its three edges in the first tetrahedron (0, 1, 3, 7) are the slots 0, 2 and 6 of corner 0
static_assert((kHostTable.c[0][1].edge[0] == 0) && (kHostTable.c[0][1].edge[1] | kHostTable.c[0][1].edge[2]) == (2 | 6),
              "");
__constant__ TetTable c_tet_table = make_tet_table();

// ---------------------------------------------------------------------------------------------- integration
__device__ __forceinline__ float centre(float origin, uint32_t idx, float voxel) {
    return origin + ((float)idx + 0.5f) * voxel;
}

// METRIC: d.depth is already a distance (a median depth map), not the accumulated depth D = sum T alpha z.
template <bool METRIC>
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(BrushTsdfGrid g, uint32_t nvox, uint32_t *__restrict__ vol,
                                                             const BrushFilterView *__restrict__ views,
                                                             ViewPointers data, uint32_t num_views, float alpha_min,
                                                             float max_depth, float near_z) {
    __shared__ BrushFilterView s_views[kMaxViews];
    __shared__ BrushTsdfViewData s_data[kMaxViews];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(views);
        uint32_t *dst = reinterpret_cast<uint32_t *>(s_views);
        for (uint32_t i = threadIdx.x; i < num_views * kViewWords; i += kThreads) dst[i] = src[i];
#pragma unroll
        for (uint32_t k = 0; k < kMaxViews; k++)  // (constant indices: the launch arguments stay scalar loads)
            if (threadIdx.x == k) s_data[k] = data.v[k];
    }
    __syncthreads();
    const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= nvox) return;
    const uint32_t i = idx % g.nx, row = idx / g.nx, j = row % g.ny, k = row / g.ny;
    const float x = centre(g.origin[0], i, g.voxel), y = centre(g.origin[1], j, g.voxel),
                z = centre(g.origin[2], k, g.voxel);
    uint32_t *plane[BRUSH_TSDF_PLANES];
#pragma unroll
    for (uint32_t q = 0; q < BRUSH_TSDF_PLANES; q++) plane[q] = vol + (size_t)q * nvox + idx;
    const uint32_t count0 = *plane[0], rgb_count0 = *plane[5];
    uint32_t count = count0, rgb_count = rgb_count0;
    int32_t sdf_sum = (int32_t)*plane[1];
    uint32_t rgb_sum[3] = {*plane[2], *plane[3], *plane[4]};
    for (uint32_t v = 0; v < num_views; v++) {
        const BrushFilterView &r = s_views[v];
        const float *m = r.viewmat;  // column-major: element (row, col) at [col * 4 + row]
        const float pz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
        if (!(pz > near_z)) continue;
        const float px = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
        const float py = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
        const float fu = floorf((r.fx * px) / pz + r.cx), fv = floorf((r.fy * py) / pz + r.cy);
        if (!(fu >= 0.0f && fu < (float)r.width && fv >= 0.0f && fv < (float)r.height)) continue;  // (a NaN fails)
        const size_t pix = (size_t)(uint32_t)fv * r.width + (uint32_t)fu;
        const BrushTsdfViewData d = s_data[v];
        if (d.mask && d.mask[pix] == 0) continue;
        const float4 c = reinterpret_cast<const float4 *>(d.img)[pix];
        const float a = c.w;
        if (!(a >= alpha_min)) continue;
        const float depth = METRIC ? d.depth[pix] : d.depth[pix] / a;
        if (!(depth > 0.0f && depth <= max_depth)) continue;
        const float s = depth - pz;
        if (!(s >= -g.trunc)) continue;
        count += 1u;
        sdf_sum += (int32_t)rintf(fminf(1.0f, s / g.trunc) * 32767.0f);
        if (fabsf(s) <= g.trunc) {
            rgb_sum[0] += (uint32_t)rintf(255.0f * fminf(fmaxf(c.x / a, 0.0f), 1.0f));
            rgb_sum[1] += (uint32_t)rintf(255.0f * fminf(fmaxf(c.y / a, 0.0f), 1.0f));
            rgb_sum[2] += (uint32_t)rintf(255.0f * fminf(fmaxf(c.z / a, 0.0f), 1.0f));
            rgb_count += 1u;
        }
    }
    if (count != count0) {
        *plane[0] = count;
        *plane[1] = (uint32_t)sdf_sum;
    }
    if (rgb_count != rgb_count0) {
        *plane[2] = rgb_sum[0];
        *plane[3] = rgb_sum[1];
        *plane[4] = rgb_sum[2];
        *plane[5] = rgb_count;
    }
}

// ---------------------------------------------------------------------------------------------- extraction
struct Lattice {
    uint32_t nx, ny, nz, n;
};

__device__ __forceinline__ uint32_t corner_offset(const Lattice &l, uint32_t code) {
    return (code & 1u) + ((code >> 1) & 1u) * l.nx + ((code >> 2) & 1u) * l.nx * l.ny;
}

// 0: not valid, 1: valid and outside, 2: valid and inside
__device__ __forceinline__ uint32_t point_state(const uint32_t *__restrict__ vol, const Lattice &l, uint32_t p,
                                                uint32_t min_views) {
    if (vol[p] < min_views) return 0u;
    return (int32_t)vol[(size_t)l.n + p] < 0 ? 2u : 1u;
}

// (a) the 7-bit mask of the active edges every lattice point owns, and their number
__global__ __launch_bounds__(kThreads) void k_tsdf_edge_mask(Lattice l, const uint32_t *__restrict__ vol,
                                                             uint32_t min_views, uint8_t *__restrict__ mask,
                                                             uint32_t *__restrict__ counts) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= l.n) return;
    const uint32_t i = p % l.nx, row = p / l.nx, j = row % l.ny, k = row / l.ny;
    const uint32_t s0 = point_state(vol, l, p, min_views);
    uint32_t bits = 0u;
    if (s0 != 0u) {
        // bit a: the point has a neighbour in +a
        const uint32_t room = (i + 1 < l.nx ? 1u : 0u) | (j + 1 < l.ny ? 2u : 0u) | (k + 1 < l.nz ? 4u : 0u);
#pragma unroll
        for (uint32_t e = 0; e < 7; e++) {
            const uint32_t code = e + 1;
            if ((code & room) != code) continue;
            const uint32_t s1 = point_state(vol, l, p + corner_offset(l, code), min_views);
            if (s1 != 0u && s1 != s0) bits |= 1u << e;
        }
    }
    mask[p] = (uint8_t)bits;
    counts[p] = __popc(bits);
}

struct EndPoint {
    float m, rgb[3];
    bool has_rgb;
};

__device__ __forceinline__ EndPoint load_end(const uint32_t *__restrict__ vol, const Lattice &l, uint32_t p) {
    EndPoint e;
    const float count = (float)vol[p];
    e.m = (float)(int32_t)vol[(size_t)l.n + p] / count;
    const uint32_t rc = vol[(size_t)5 * l.n + p];
    e.has_rgb = rc != 0u;
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) e.rgb[c] = e.has_rgb ? (float)vol[(size_t)(2 + c) * l.n + p] / (float)rc : 128.0f;
    return e;
}

// (c) one vertex per active edge, in lattice order, then slot
__global__ __launch_bounds__(kThreads) void k_tsdf_vertices(BrushTsdfGrid g, Lattice l,
                                                            const uint32_t *__restrict__ vol,
                                                            const uint8_t *__restrict__ mask,
                                                            const uint32_t *__restrict__ incl, uint32_t num_vertices,
                                                            float *__restrict__ vertices, uint8_t *__restrict__ colors) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= l.n) return;
    const uint32_t bits = mask[p];
    if (bits == 0u) return;
    const uint32_t i = p % l.nx, row = p / l.nx, j = row % l.ny, k = row / l.ny;
    const EndPoint e0 = load_end(vol, l, p);
    uint32_t out = incl[p] - __popc(bits);
    for (uint32_t e = 0; e < 7; e++) {
        if (!(bits >> e & 1u)) continue;
        const uint32_t code = e + 1;
        const EndPoint e1 = load_end(vol, l, p + corner_offset(l, code));
        const float w = e0.m / (e0.m - e1.m);
        if (out < num_vertices) {  // (always, with the totals of the count call)
            const uint32_t lat[3] = {i, j, k};
#pragma unroll
            for (uint32_t a = 0; a < 3; a++) {
                const float step = (float)((code >> a) & 1u);
                vertices[(size_t)out * 3 + a] = fmaf(((float)lat[a] + 0.5f) + w * step, g.voxel, g.origin[a]);
                const float c0 = e0.has_rgb ? e0.rgb[a] : e1.rgb[a], c1 = e1.has_rgb ? e1.rgb[a] : e0.rgb[a];
                colors[(size_t)out * 3 + a] = (uint8_t)rintf(fminf(fmaxf(c0 + w * (c1 - c0), 0.0f), 255.0f));
            }
        }
        out++;
    }
}

// The inside bits of a cell's 8 corners, or false when the cell does not take part (no room, or a corner not valid).
__device__ __forceinline__ bool cell_inside_bits(const uint32_t *__restrict__ vol, const Lattice &l, uint32_t p,
                                                 uint32_t min_views, uint32_t *inside) {
    const uint32_t i = p % l.nx, row = p / l.nx, j = row % l.ny, k = row / l.ny;
    if (!(i + 1 < l.nx && j + 1 < l.ny && k + 1 < l.nz)) return false;
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        const uint32_t s = point_state(vol, l, p + corner_offset(l, c), min_views);
        if (s == 0u) return false;
        bits |= (s == 2u ? 1u : 0u) << c;
    }
    *inside = bits;
    return true;
}

__device__ __forceinline__ const TetCase &tet_case(uint32_t t, uint32_t inside) {
    // the tetrahedron's vertices are corners 0, 1 << a, 1 << a | 1 << b, 7 (the t-th permutation, lexicographic)
    const uint32_t a = t >> 1, b = (t & 1u) ? (a == 2u ? 1u : 2u) : (a == 0u ? 1u : 0u);
    const uint32_t c1 = 1u << a, c2 = c1 | (1u << b);
    const uint32_t m = (inside & 1u) | ((inside >> c1 & 1u) << 1) | ((inside >> c2 & 1u) << 2) | ((inside >> 7 & 1u) << 3);
    return c_tet_table.c[t][m];
}

// (d) the triangles of every cell
__global__ __launch_bounds__(kThreads) void k_tsdf_tri_count(Lattice l, const uint32_t *__restrict__ vol,
                                                             uint32_t min_views, uint32_t *__restrict__ counts) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= l.n) return;
    uint32_t inside = 0u, n = 0u;
    if (cell_inside_bits(vol, l, p, min_views, &inside) && inside != 0u && inside != 255u) {
#pragma unroll
        for (uint32_t t = 0; t < 6; t++) n += tet_case(t, inside).ntri;
    }
    counts[p] = n;
}

// (f) the faces, in cell order, then tetrahedron, then triangle
__global__ __launch_bounds__(kThreads) void k_tsdf_faces(Lattice l, const uint32_t *__restrict__ vol,
                                                         uint32_t min_views, const uint8_t *__restrict__ mask,
                                                         const uint32_t *__restrict__ vert_incl,
                                                         const uint32_t *__restrict__ tri_counts,
                                                         const uint32_t *__restrict__ tri_incl, uint32_t num_faces,
                                                         uint32_t *__restrict__ faces) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= l.n) return;
    const uint32_t n = tri_counts[p];
    if (n == 0u) return;
    uint32_t inside = 0u;
    if (!cell_inside_bits(vol, l, p, min_views, &inside)) return;  // (never: n != 0)
    uint32_t out = tri_incl[p] - n;
    for (uint32_t t = 0; t < 6; t++) {
        const TetCase &tc = tet_case(t, inside);
        for (uint32_t f = 0; f < tc.ntri; f++, out++) {
            if (out >= num_faces) return;  // (never, with the totals of the count call)
#pragma unroll
            for (uint32_t q = 0; q < 3; q++) {
                const uint32_t e = tc.edge[f * 3 + q], owner = p + corner_offset(l, e >> 3), slot = e & 7u;
                const uint32_t bits = mask[owner];
                faces[(size_t)out * 3 + q] = vert_incl[owner] - __popc(bits) + __popc(bits & ((1u << slot) - 1u));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- host
bool grid_ok(const BrushTsdfGrid *g) {
    if (!g) return false;
    const float inf = __builtin_inff();
    if (!(g->voxel > 0.0f && g->voxel < inf && g->trunc > 0.0f && g->trunc < inf)) return false;
    for (int a = 0; a < 3; a++)
        if (!(g->origin[a] > -inf && g->origin[a] < inf)) return false;
    const uint32_t side[3] = {g->nx, g->ny, g->nz};
    uint64_t n = 1;
    for (int a = 0; a < 3; a++) {
        if (side[a] < 1u || side[a] > BRUSH_TSDF_MAX_SIDE) return false;
        n *= side[a];
    }
    return n <= BRUSH_TSDF_MAX_VOXELS;
}

struct MeshWs {
    uint8_t *mask;
    uint32_t *counts, *vert_incl, *tri_incl;
    void *scan;
    size_t bytes;
};

MeshWs carve_mesh_ws(void *ws, uint32_t n) {
    Carver c(ws);
    MeshWs w;
    w.mask = c.take<uint8_t>(n);
    w.counts = c.take<uint32_t>(n);  // the edge counts, then the triangle counts
    w.vert_incl = c.take<uint32_t>(n);
    w.tri_incl = c.take<uint32_t>(n);
    w.scan = c.take<char>(scan_workspace_bytes(n));
    w.bytes = c.bytes();
    return w;
}

}  // namespace
}  // namespace brush

using namespace brush;

extern "C" int brush_tsdf_integrate_ex(const BrushTsdfGrid *h_grid, uint32_t *volume, const BrushFilterView *views,
                                       const BrushTsdfViewData *h_data, uint32_t num_views, float alpha_min,
                                       float max_depth, float near_z, uint32_t flags, brush_stream_t stream) {
    if ((flags & ~BRUSH_TSDF_DEPTH_METRIC) != 0u) return BRUSH_ERR_INVALID_ARG;
    if (!grid_ok(h_grid) || !volume || !views || !h_data) return BRUSH_ERR_INVALID_ARG;
    if (num_views < 1u || num_views > kMaxViews) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(volume, 16) || misaligned(views, 16)) return BRUSH_ERR_INVALID_ARG;
    const float inf = __builtin_inff();
    if (!(alpha_min > 0.0f && alpha_min < inf) || !(near_z >= 0.0f && near_z < inf) || !(max_depth > 0.0f))
        return BRUSH_ERR_INVALID_ARG;
    ViewPointers data{};
    for (uint32_t v = 0; v < num_views; v++) {
        const BrushTsdfViewData &d = h_data[v];
        if (!d.img || !d.depth || misaligned(d.img, 16) || misaligned(d.depth, 4)) return BRUSH_ERR_INVALID_ARG;
        data.v[v] = d;
    }
    const uint32_t nvox = h_grid->nx * h_grid->ny * h_grid->nz;
    const auto kernel = (flags & BRUSH_TSDF_DEPTH_METRIC) ? k_tsdf_integrate<true> : k_tsdf_integrate<false>;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(nvox, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       *h_grid, nvox, volume, views, data, num_views, alpha_min, max_depth, near_z);
    BRUSH_HIP_CHECK(hipGetLastError());
    return BRUSH_OK;
}

extern "C" int brush_tsdf_integrate(const BrushTsdfGrid *h_grid, uint32_t *volume, const BrushFilterView *views,
                                    const BrushTsdfViewData *h_data, uint32_t num_views, float alpha_min,
                                    float max_depth, float near_z, brush_stream_t stream) {
    return brush_tsdf_integrate_ex(h_grid, volume, views, h_data, num_views, alpha_min, max_depth, near_z, 0u, stream);
}

extern "C" int brush_tsdf_mesh_workspace_size(uint32_t nx, uint32_t ny, uint32_t nz, size_t *bytes) {
    const BrushTsdfGrid g = {{0.0f, 0.0f, 0.0f}, 1.0f, 1.0f, nx, ny, nz};
    if (!bytes || !grid_ok(&g)) return BRUSH_ERR_INVALID_ARG;
    *bytes = carve_mesh_ws(nullptr, nx * ny * nz).bytes;
    return BRUSH_OK;
}

extern "C" int brush_tsdf_mesh_count(const BrushTsdfGrid *h_grid, const uint32_t *volume, uint32_t min_views,
                                     uint32_t *totals, void *workspace, size_t workspace_bytes,
                                     brush_stream_t stream) {
    if (!grid_ok(h_grid) || !volume || !totals || !workspace || min_views < 1u) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(volume, 16) || misaligned(totals, 4) || misaligned(workspace, 256)) return BRUSH_ERR_INVALID_ARG;
    const Lattice l = {h_grid->nx, h_grid->ny, h_grid->nz, h_grid->nx * h_grid->ny * h_grid->nz};
    const MeshWs w = carve_mesh_ws(workspace, l.n);
    if (workspace_bytes < w.bytes) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(l.n, kThreads)), block(kThreads);
    hipLaunchKernelGGL(k_tsdf_edge_mask, grid, block, 0, s, l, volume, min_views, w.mask, w.counts);
    BRUSH_HIP_CHECK(hipGetLastError());
    BRUSH_HIP_CHECK(scan_launch(w.counts, w.vert_incl, l.n, nullptr, totals, 0xFFFFFFFFu, nullptr, w.scan, s));
    hipLaunchKernelGGL(k_tsdf_tri_count, grid, block, 0, s, l, volume, min_views, w.counts);
    BRUSH_HIP_CHECK(hipGetLastError());
    BRUSH_HIP_CHECK(scan_launch(w.counts, w.tri_incl, l.n, nullptr, totals + 1, 0xFFFFFFFFu, nullptr, w.scan, s));
    return BRUSH_OK;
}

extern "C" int brush_tsdf_mesh_emit(const BrushTsdfGrid *h_grid, const uint32_t *volume, uint32_t min_views,
                                    uint32_t num_vertices, uint32_t num_faces, float *vertices, uint8_t *colors,
                                    uint32_t *faces, void *workspace, size_t workspace_bytes, brush_stream_t stream) {
    if (!grid_ok(h_grid) || !volume || !workspace || min_views < 1u) return BRUSH_ERR_INVALID_ARG;
    if (num_vertices != 0u && (!vertices || !colors)) return BRUSH_ERR_INVALID_ARG;
    if (num_faces != 0u && !faces) return BRUSH_ERR_INVALID_ARG;
    if (misaligned(volume, 16) || misaligned(vertices, 4) || misaligned(faces, 4) || misaligned(workspace, 256))
        return BRUSH_ERR_INVALID_ARG;
    const Lattice l = {h_grid->nx, h_grid->ny, h_grid->nz, h_grid->nx * h_grid->ny * h_grid->nz};
    const MeshWs w = carve_mesh_ws(workspace, l.n);
    if (workspace_bytes < w.bytes) return BRUSH_ERR_WORKSPACE_SMALL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(ceil_div(l.n, kThreads)), block(kThreads);
    if (num_vertices != 0u) {
        hipLaunchKernelGGL(k_tsdf_vertices, grid, block, 0, s, *h_grid, l, volume, w.mask, w.vert_incl, num_vertices,
                           vertices, colors);
        BRUSH_HIP_CHECK(hipGetLastError());
    }
    if (num_faces != 0u) {
        hipLaunchKernelGGL(k_tsdf_faces, grid, block, 0, s, l, volume, min_views, w.mask, w.vert_incl, w.counts,
                           w.tri_incl, num_faces, faces);
        BRUSH_HIP_CHECK(hipGetLastError());
    }
    return BRUSH_OK;
}
