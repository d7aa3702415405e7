#!/usr/bin/env python3
"""Times the median-depth replay next to the forward it replays: `iters` passes of one brush_render_forward_depth
followed by brush_render_median_depth, on two synthetic scenes: the bench's S1 (1 M splats, 1080p, SH 3) and the same
cloud made opaque (every raw opacity 6), where a pixel crosses the level after a few entries and the replay leaves the
lists early.  Meant to run under `rocprofv3 --kernel-trace --stats`, in a run of its own, which gives
k_median_depth_quad against k_rasterize_quad of the same run; it also prints event-timed medians of its own (forward
alone, forward + replay) and the fraction of pixels that have a median.

    python tools/median_depth_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20]
                                      [--level 0.5] [--scenes s1,opaque] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import render as R  # noqa: E402
from brush_amd.median_depth import median_depth_from_aux  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--level", type=float, default=0.5)
    ap.add_argument("--scenes", default="s1,opaque")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    scenes = a.scenes.split(",")
    if not scenes or any(s not in ("s1", "opaque") for s in scenes):
        ap.error("--scenes takes s1 and / or opaque, separated by a comma")
    dev = torch.device("cuda:0")
    w, h = a.width, a.height
    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    means, log_scales, quats, sh, raw_opac = (torch.from_numpy(c[k]).to(dev) for k in
                                              ("means", "log_scales", "quats", "sh", "raw_opac"))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    bufs = R._depth_buffers(a.splats, (w, h), dev)
    out = (torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.int32, device=dev))

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    lines = []
    for scene in scenes:
        opac = raw_opac if scene == "s1" else torch.full_like(raw_opac, 6.0)

        def forward():
            with torch.no_grad():
                return R._forward_impl(cam, (w, h), means, log_scales, quats, sh, opac, False, None,
                                       expect_backward=False, depth=bufs)

        def both():
            img, aux, u = forward()
            median_depth_from_aux(u, aux, bufs[1], level=a.level, out=out)
            return img, aux

        res = {"forward_ms": timed(forward), "forward_replay_ms": timed(both)}
        img, aux = both()
        torch.cuda.synchronize()
        line = {"scene": scene, "splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree,
                "iters": a.iters, "level": a.level, **res, "replay_ms": res["forward_replay_ms"] - res["forward_ms"],
                "num_visible": aux.read_num_visible(), "num_intersections": aux.read_num_intersections(),
                "pixels_with_median": float((out[1] >= 0).float().mean()),
                "mean_alpha": float(img[..., 3].mean())}
        print(json.dumps(line))
        lines.append(line)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
