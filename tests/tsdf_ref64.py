"""float64 restatement of the mesh export kernels (include/brush_hip.h: brush_tsdf_integrate, brush_tsdf_mesh_count,
brush_tsdf_mesh_emit): the same formulas, the same decomposition and the same orders, in NumPy float64 / int64.

`integrate` also reports, per voxel and view, whether a decision quantity of the pair lies within a relative 1e-5 of its
edge: there the f32 kernel may legitimately decide the other way, and the GPU test leaves the pair out.
`fusion_case` is the scene both tests/test_tsdf_cpu.py (which checks the share of such pairs) and
tests/test_gpu_tsdf.py (which compares the kernel with `integrate` on it) use.
"""
import math

import numpy as np

SDF_ONE = 32767
EDGE_REL = 1e-5
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def f32(x):
    """What the kernels receive of a host scalar or array: its float32 rounding, as float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------- integration
def voxel_centres(origin, voxel, dims):
    """[nvox, 3] float64, x fastest."""
    nx, ny, nz = dims
    o, s = f32(origin), float(f32(voxel))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], 1).astype(np.float64)
    return o[None, :] + (idx + 0.5) * s


def _near(q, edge, scale=None):
    scale = np.abs(edge) if scale is None else scale
    return np.abs(q - edge) <= EDGE_REL * scale


def integrate(origin, voxel, dims, trunc, records, imgs, depths, masks=None, *, alpha_min=0.5, max_depth=None,
              near=0.2):
    """records: float32 [V, 24] (filter3d.view_records); imgs [h, w, 4] / depths [h, w] float32, masks uint8 or None.
    Returns {"count", "sdf_sum", "rgb_sum" [nvox, 3], "rgb_count"} as int64 with every sdf / colour term rounded from
    its float64 value, {"contrib" [V, nvox]: the pair added to count, "uncertain" [V, nvox]: a decision of the pair is
    within EDGE_REL of its edge}."""
    x = voxel_centres(origin, voxel, dims)
    nvox, nv = x.shape[0], records.shape[0]
    trunc, alpha_min, near = float(f32(trunc)), float(f32(alpha_min)), float(f32(near))
    max_depth = math.inf if max_depth is None else float(f32(max_depth))
    count, rgb_count = np.zeros(nvox, np.int64), np.zeros(nvox, np.int64)
    sdf_sum, rgb_sum = np.zeros(nvox, np.int64), np.zeros((nvox, 3), np.int64)
    contrib, uncertain = np.zeros((nv, nvox), bool), np.zeros((nv, nvox), bool)
    words = records.view(np.uint32)
    for v in range(nv):
        m = records[v, :16].astype(np.float64).reshape(4, 4).T  # column-major record -> row-major matrix
        fx, fy, cx, cy = (float(t) for t in records[v, 16:20])
        w, h = int(words[v, 20]), int(words[v, 21])
        p = x @ m[:3, :3].T + m[:3, 3]
        pz = p[:, 2]
        alive = pz > near
        unc = _near(pz, near)
        with np.errstate(divide="ignore", invalid="ignore"):
            u, t = fx * p[:, 0] / pz + cx, fy * p[:, 1] / pz + cy
        u, t = np.where(alive, u, 0.0), np.where(alive, t, 0.0)
        # (a projection more than a pixel outside the image is outside whichever way its floor is rounded)
        close = alive & (u > -1.0) & (u < w + 1.0) & (t > -1.0) & (t < h + 1.0)
        for q in (u, t):
            r = np.rint(q)
            unc |= close & _near(q, r, np.maximum(1.0, np.abs(r)))
        fu, fv = np.floor(u), np.floor(t)
        inside = (fu >= 0) & (fu < w) & (fv >= 0) & (fv < h)
        alive &= inside
        ix, iy = np.where(alive, fu, 0).astype(np.int64), np.where(alive, fv, 0).astype(np.int64)
        if masks is not None and masks[v] is not None:
            alive &= masks[v][iy, ix] != 0
        img, dep = imgs[v].astype(np.float64), depths[v].astype(np.float64)
        a = img[iy, ix, 3]
        unc |= alive & _near(a, alpha_min)
        alive &= a >= alpha_min
        a = np.where(alive, a, 1.0)
        d = dep[iy, ix] / a
        if math.isfinite(max_depth):
            unc |= alive & _near(d, max_depth)
        alive &= (d > 0) & (d <= max_depth)
        s = d - pz
        unc |= alive & (_near(s, -trunc, trunc) | _near(s, trunc, trunc))
        alive &= s >= -trunc
        q = np.rint(np.minimum(1.0, s / trunc) * SDF_ONE).astype(np.int64)
        count += alive
        sdf_sum += np.where(alive, q, 0)
        surf = alive & (np.abs(s) <= trunc)
        c = np.rint(255.0 * np.clip(img[iy, ix, :3] / a[:, None], 0.0, 1.0)).astype(np.int64)
        rgb_sum += np.where(surf[:, None], c, 0)
        rgb_count += surf
        contrib[v], uncertain[v] = alive, unc
    return {"count": count, "sdf_sum": sdf_sum, "rgb_sum": rgb_sum, "rgb_count": rgb_count, "contrib": contrib,
            "uncertain": uncertain}


def look_at_record(position, target, up, fx, fy, cx, cy, w, h):
    """One float32 [24] view record: a camera at `position` whose +z looks at `target` (x right, y down)."""
    p, t, u = (np.asarray(a, dtype=np.float64) for a in (position, target, up))
    f = (t - p) / np.linalg.norm(t - p)
    r = np.cross(u, f)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([r, d, f], 0)
    w2c[:3, 3] = -w2c[:3, :3] @ p
    rec = np.zeros(24, dtype=np.float32)
    rec[:16] = w2c.astype(np.float32).T.reshape(16)
    rec[16:20] = fx, fy, cx, cy
    rec.view(np.uint32)[20:22] = w, h
    return rec


FUSION_SEED = 5


def fusion_case(seed=FUSION_SEED, dims=(24, 20, 16)):
    """A sphere of radius 0.55 at (0.05, -0.03, 0.02) in front of a slanted backdrop, seen by five 67 x 45 views: three
    plain ones, one that sees the volume only partly, one that looks away from it (the volume is behind the camera) and
    carries nothing, and the second view has a mask.  Depth maps are analytic (ray / sphere at the pixel centres),
    alphas random in [0.3, 1] (so some pixels fall below alpha_min), colours random in [0, 1.15] (so some clamp)."""
    rng = np.random.default_rng(seed)
    w, h = 67, 45
    voxel = 0.1
    origin = tuple(-0.5 * voxel * n + o for n, o in zip(dims, (0.013, -0.021, 0.007)))
    centre, radius = np.array([0.05, -0.03, 0.02]), 0.55
    cams = [((2.6, 0.4, 0.3), (0.0, 0.0, 0.0)), ((-0.5, 2.4, 1.1), (0.1, 0.0, 0.0)), ((0.3, -1.0, 2.7), (0.0, 0.1, 0.0)),
            ((-2.2, -1.2, -0.6), (0.2, 2.0, 0.6)),   # aims beside the volume: sees it partly
            ((0.4, 0.3, -2.8), (0.8, 0.6, -5.6))]    # looks away: the volume is behind it
    recs, imgs, depths, masks = [], [], [], []
    for k, (pos, target) in enumerate(cams):
        rec = look_at_record(pos, target, (0.0, 0.0, 1.0) if k != 2 else (0.0, 1.0, 0.0), 70.0 + k, 68.5 - k,
                             33.2 + 0.3 * k, 22.7 - 0.2 * k, w, h)
        m = rec[:16].astype(np.float64).reshape(4, 4).T
        c_cam = m[:3, :3] @ centre + m[:3, 3]
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        d = np.stack([(xs - rec[18]) / rec[16], (ys - rec[19]) / rec[17], np.ones_like(xs)], -1)
        dd, dc = (d * d).sum(-1), (d * c_cam).sum(-1)
        disc = dc * dc - dd * ((c_cam * c_cam).sum() - radius * radius)
        hit = (disc > 0) & (dc > 0)
        z = np.where(hit, (dc - np.sqrt(np.maximum(disc, 0.0))) / dd, 3.2 + 1.0 * xs / w)  # the backdrop: 3.2 .. 4.2
        alpha = rng.uniform(0.3, 1.0, (h, w))
        colour = rng.uniform(0.0, 1.15, (h, w, 3))
        img = np.concatenate([colour * alpha[..., None], alpha[..., None]], -1).astype(np.float32)
        recs.append(rec)
        imgs.append(img)
        depths.append((z * img[..., 3].astype(np.float64)).astype(np.float32))
        masks.append((rng.uniform(size=(h, w)) > 0.3).astype(np.uint8) * np.uint8(200) if k == 1 else None)
    return {"origin": origin, "voxel": voxel, "dims": dims, "trunc": 4 * voxel, "records": np.stack(recs),
            "imgs": imgs, "depths": depths, "masks": masks, "alpha_min": 0.5, "max_depth": 4.0, "near": 0.2}


# ---------------------------------------------------------------------------- extraction
def tet_vertices(t):
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def tet_table():
    """[t][m] -> list of triangles, each three (lower corner, slot) pairs: the header's rule, evaluated."""
    table = []
    for t in range(6):
        tv = tet_vertices(t)
        row = []
        for m in range(16):
            ins = [p for p in range(4) if m >> p & 1]
            outs = [p for p in range(4) if not m >> p & 1]
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(i, outs[0]) for i in ins]]
            elif len(ins) == 2:
                quad = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            else:
                tris = []
            bits = lambda c: np.array([c & 1, c >> 1 & 1, c >> 2 & 1], dtype=np.float64)  # noqa: E731
            out = []
            for tri in tris:
                mid = [0.5 * (bits(tv[p]) + bits(tv[q])) for p, q in tri]
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                direction = (np.mean([bits(tv[p]) for p in outs], 0) - np.mean([bits(tv[p]) for p in ins], 0))
                if normal @ direction < 0:
                    tri = [tri[0], tri[2], tri[1]]
                enc = []
                for p, q in tri:
                    lo, hi = min(tv[p], tv[q]), max(tv[p], tv[q])
                    assert lo & hi == lo  # nested corner codes
                    enc.append((lo, (lo ^ hi) - 1))
                out.append(enc)
            row.append(out)
        table.append(row)
    return table


def extract(origin, voxel, count, sdf_sum, rgb_sum=None, rgb_count=None, min_views=2):
    """count / sdf_sum [nz, ny, nx]; returns (vertices float64 [V, 3], colors float64 [V, 3] (not rounded),
    faces int64 [F, 3]) in the kernels' orders."""
    count, sdf_sum = np.asarray(count).astype(np.int64), np.asarray(sdf_sum).astype(np.int64)
    nz, ny, nx = count.shape
    n = nx * ny * nz
    o, s = f32(origin), float(f32(voxel))
    cnt, sdf = count.reshape(-1), sdf_sum.reshape(-1)
    if rgb_sum is None:
        rsum, rcnt = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    else:
        rsum, rcnt = np.asarray(rgb_sum).astype(np.int64).reshape(n, 3), np.asarray(rgb_count).astype(np.int64).reshape(-1)
    valid, inside = cnt >= min_views, sdf < 0
    strides = (1, nx, nx * ny)
    lattice = np.stack(np.unravel_index(np.arange(n), (nz, ny, nx))[::-1], 1)  # (i, j, k) per point
    size = np.array([nx, ny, nz])

    def offset(code):
        return sum(strides[a] for a in range(3) if code >> a & 1)

    def colour(p, other):
        if rcnt[p]:
            return rsum[p] / rcnt[p]
        if rcnt[other]:
            return rsum[other] / rcnt[other]
        return np.full(3, 128.0)

    vertex_of, vertices, colors = {}, [], []
    for p in np.nonzero(valid)[0]:
        for e in range(7):
            code = e + 1
            step = np.array([code & 1, code >> 1 & 1, code >> 2 & 1])
            if ((lattice[p] + step) >= size).any():
                continue
            q = p + offset(code)
            if not valid[q] or inside[p] == inside[q]:
                continue
            m0, m1 = sdf[p] / cnt[p], sdf[q] / cnt[q]
            w = m0 / (m0 - m1)
            vertex_of[(int(p), e)] = len(vertices)
            vertices.append(o + ((lattice[p] + 0.5) + w * step) * s)
            c0, c1 = colour(p, q), colour(q, p)
            colors.append(np.clip(c0 + w * (c1 - c0), 0.0, 255.0))
    table = tet_table()
    faces = []
    for p in range(n):
        if ((lattice[p] + 1) >= size).any():
            continue
        corners = [p + offset(c) for c in range(8)]
        if not all(valid[c] for c in corners):
            continue
        for t in range(6):
            tv = tet_vertices(t)
            m = sum(int(inside[corners[tv[k]]]) << k for k in range(4))
            for tri in table[t][m]:
                faces.append([vertex_of[(corners[lo], slot)] for lo, slot in tri])
    return (np.array(vertices, dtype=np.float64).reshape(-1, 3), np.array(colors, dtype=np.float64).reshape(-1, 3),
            np.array(faces, dtype=np.int64).reshape(-1, 3))


def sphere_field(dims=(20, 18, 16), radius=6.0, trunc_voxels=4.0, views=3, centre=None):
    """(count, sdf_sum) [nz, ny, nx] of an analytic sphere of `radius` voxels: every voxel observed by `views` views,
    each adding rint(clip(distance / trunc, -1, 1) 32767).  centre: in lattice coordinates (default: the middle)."""
    nx, ny, nz = dims
    c = np.array([(nx - 1) / 2.0, (ny - 1) / 2.0, (nz - 1) / 2.0]) if centre is None else np.asarray(centre, float)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - radius
    q = np.rint(np.clip(dist / trunc_voxels, -1.0, 1.0) * SDF_ONE).astype(np.int64)
    return np.full((nz, ny, nx), views, dtype=np.int64), q * views
