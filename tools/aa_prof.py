#!/usr/bin/env python3
"""Cost of the antialiased mode (BRUSH_AUX_ANTIALIASED) next to the plain render, alternating the two in one process:
  * `iters` forward + backward passes of render_splats on one synthetic scene (default S1: 1 M splats, 1080p, SH 3),
    default and deterministic mode;
  * `iters` SplatTrainer steps (fused backward + Adam with the deferred SH block, the bench's path; no refinement).
Plain and antialiased calls alternate call by call, so clock and thermal drift hit both alike; medians of event times.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives the per-kernel times of the cull and VJP
instantiations with (DM = degree | 8) and without the mode.

    python tools/aa_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/aa_prof.py --iters 10

profiles/antialias_prof.json is the first form's output; profiles/antialias_kernel_stats.csv the per-kernel statistics
(calls, total / mean / median / min / max ns, registers, scratch) of a kernel trace of the second.
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

    def render(det, aa):
        def fn():
            img, _ = brush_amd.render_splats(cam, (w, h), *params, deterministic=det, antialiased=aa)
            torch.autograd.grad([img], params, [v_out])
        return fn

    res = {}
    for det in (False, True):
        t = _timed({"plain": render(det, False), "antialiased": render(det, True)}, a.iters)
        sfx = "_det" if det else ""
        res[f"fwd_bwd_plain{sfx}_ms"], res[f"fwd_bwd_antialiased{sfx}_ms"] = t["plain"], t["antialiased"]

    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    steps = {}
    for aa in (False, True):
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0, antialiased=aa))
        steps["antialiased" if aa else "plain"] = (lambda s=s, tr=tr: tr.step(s, cam, gt))
    t = _timed(steps, a.iters)
    res["train_step_plain_ms"], res["train_step_antialiased_ms"] = t["plain"], t["antialiased"]
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
