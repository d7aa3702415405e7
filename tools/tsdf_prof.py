#!/usr/bin/env python3
"""Cost of the mesh export (brush_amd/tsdf.py) on one synthetic job (default: a 256^3 volume, 1080p views of a sphere in
front of a backdrop, 16 cameras on a circle), medians of `iters` rounds of event times, the callables in alternation:
  * one brush_tsdf_integrate launch of K = 1, 2, 4, 8 and 16 views, and its time per view: the volume's 24 B per voxel
    are read (and at most written) once per launch, so the time per view falls with K until the per-view arithmetic and
    the image gathers are what is left;
  * a device copy of the volume's bytes (24 B read + 24 B written per voxel): the floor of a launch that touches every
    voxel's words once, whatever K;
  * brush_tsdf_mesh_count (edge masks, scan, triangle counts, scan) and brush_tsdf_mesh_emit (vertices, faces) on the
    fused volume, with the vertex and face counts.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, in a run of its own, which gives k_tsdf_integrate and the
six extraction launches (k_tsdf_edge_mask, the scan kernels, k_tsdf_vertices, k_tsdf_tri_count, k_tsdf_faces) one by one.

    python tools/tsdf_prof.py [--resolution 256] [--width 1920] [--height 1080] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tsdf_prof.py --iters 5

profiles/tsdf_prof.json is the first form's output; profiles/tsdf_kernel_stats.csv the per-kernel statistics of a kernel
trace of the second.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd.filter3d import view_records  # noqa: E402
from brush_amd.tsdf import MAX_VIEWS, TsdfVolume  # noqa: E402


def _timed(fns, iters):
    """{name: median ms} for the callables of `fns`, called in alternation."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ts.items()}


def _orbit(count, w, h, radius):
    """`count` cameras on a circle of `radius` around the origin, looking at it."""
    views = []
    for i in range(count):
        a = 2.0 * math.pi * i / count
        pos = [radius * math.sin(a), 0.0, -radius * math.cos(a)]
        rot = [0.0, -math.sin(a / 2.0), 0.0, math.cos(a / 2.0)]  # about +y: the camera's +z axis points at the origin
        views.append((brush_amd.Camera(pos, rot, 2 * np.arctan(0.5), 2 * np.arctan(0.5 * h / w), (0.5, 0.5)), (w, h)))
    return views


def _sphere_render(rec, radius, backdrop, dev):
    """(img [h,w,4], depth [h,w]) of a unit-alpha sphere at the origin in front of a backdrop at camera depth
    `backdrop`, as the renderer would leave them (premultiplied colour, accumulated depth)."""
    w, h = int(rec.view(np.uint32)[20]), int(rec.view(np.uint32)[21])
    m = torch.from_numpy(rec[:16].reshape(4, 4).T.copy()).to(dev)
    c = m[:3, 3]  # the origin in camera space
    ys, xs = torch.meshgrid(torch.arange(h, device=dev) + 0.5, torch.arange(w, device=dev) + 0.5, indexing="ij")
    d = torch.stack([(xs - float(rec[18])) / float(rec[16]), (ys - float(rec[19])) / float(rec[17]),
                     torch.ones_like(xs)], -1)
    dd, dc = (d * d).sum(-1), (d * c).sum(-1)
    disc = dc * dc - dd * (float((c * c).sum()) - radius * radius)
    z = torch.where(disc > 0, (dc - torch.sqrt(disc.clamp(min=0))) / dd, torch.full_like(dd, backdrop))
    n = torch.nn.functional.normalize(z[..., None] * d - c, dim=-1)
    img = torch.cat([(0.5 + 0.5 * n).clamp(0, 1), torch.ones_like(z)[..., None]], -1).contiguous()
    return img, z.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, r = a.width, a.height, a.resolution
    voxel = 2.56 / r
    rec = view_records(_orbit(MAX_VIEWS, w, h, 3.0))
    renders = [_sphere_render(rec[v], 0.8, 4.5, dev) for v in range(MAX_VIEWS)]
    imgs, depths = [x[0] for x in renders], [x[1] for x in renders]

    def volume():
        return TsdfVolume((-1.28, -1.28, -1.28), voxel, (r, r, r), device=dev)

    vol = volume()
    fns = {}
    for k in (1, 2, 4, 8, 16):
        fns[f"integrate_{k}_views_ms"] = lambda k=k: vol.integrate(rec[:k], imgs[:k], depths[:k])
    src = torch.empty(vol.nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    fns["copy_24B_per_voxel_ms"] = lambda: dst.copy_(src)
    res = _timed(fns, a.iters)
    for k in (1, 2, 4, 8, 16):
        res[f"integrate_{k}_views_ms_per_view"] = res[f"integrate_{k}_views_ms"] / k
    del vol, src, dst

    vol = volume()
    vol.integrate(rec, imgs, depths)
    observed = float((vol.state[0] != 0).float().mean())
    lib, grid = _lib.lib(), vol._grid()
    nbytes = _lib.size_query("brush_tsdf_mesh_workspace_size", r, r, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = _lib.current_stream(dev)

    def count():
        _lib.check(lib.brush_tsdf_mesh_count(C.byref(grid), vol.state.data_ptr(), 2, totals.data_ptr(), ws.data_ptr(),
                                             nbytes, stream), "brush_tsdf_mesh_count")

    count()
    nv, nf = (int(x) for x in totals.cpu().tolist())
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((nv, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)

    def emit():
        _lib.check(lib.brush_tsdf_mesh_emit(C.byref(grid), vol.state.data_ptr(), 2, nv, nf, vertices.data_ptr(),
                                            colors.data_ptr(), faces.data_ptr(), ws.data_ptr(), nbytes, stream),
                   "brush_tsdf_mesh_emit")

    counts = torch.ones(r * r * r, dtype=torch.int32, device=dev)
    res.update(_timed({"mesh_count_ms": count, "mesh_emit_ms": emit,
                       "scan_of_one_word_per_voxel_ms": lambda: brush_amd.prefix_sum(counts)}, a.iters))
    line = {"resolution": r, "voxels": r * r * r, "volume_bytes": vol.nbytes, "width": w, "height": h, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), "observed_fraction": observed, "vertices": nv, "faces": nf,
            "mesh_workspace_bytes": nbytes, **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
