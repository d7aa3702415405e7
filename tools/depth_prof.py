#!/usr/bin/env python3
"""Times the depth instantiations next to the plain render: `iters` forward + backward passes of render_splats and as
many of render_splats_depth (gradients on the image and on the depth) on one synthetic scene, default S1 (1 M splats,
1080p, SH 3), in the default and the deterministic mode.  Meant to run under `rocprofv3 --kernel-trace --stats`, which
gives the per-kernel times (k_rasterize_quad / k_rasterize_backward_quad with and without their DepthOut / DepthGrad
argument, k_depth_means_grad, k_sum_isect_depth); it also prints event-timed medians of its own.

    python tools/depth_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h = a.width, a.height
    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    p = [torch.from_numpy(c[k]).to(dev).requires_grad_(True) for k in ("means", "log_scales", "quats", "sh",
                                                                         "raw_opac")]
    xy = torch.zeros((a.splats, 2), device=dev, requires_grad=True)
    params = [p[0], xy, p[1], p[2], p[3], p[4]]
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gen = torch.Generator(device="cpu").manual_seed(0)
    v_out = torch.rand((h, w, 4), generator=gen).to(dev)
    v_d = (torch.rand((h, w), generator=gen) * 1e-3).to(dev)

    def plain(det):
        img, _ = brush_amd.render_splats(cam, (w, h), *params, deterministic=det)
        torch.autograd.grad([img], params, [v_out])

    def depth(det):
        img, d, _ = brush_amd.render_splats_depth(cam, (w, h), *params, deterministic=det)
        torch.autograd.grad([img, d], params, [v_out, v_d])

    res = {}
    for det in (False, True):
        for name, fn in (("plain", plain), ("depth", depth)):
            for _ in range(3):
                fn(det)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(det)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            res[f"{name}{'_det' if det else ''}_ms"] = float(np.median(ts))
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters, **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
