#!/usr/bin/env python3
"""Cost of the 3D smoothing filter (TrainConfig.filter3d) on one synthetic scene (default S1: 1 M splats, 1080p, SH 3),
alternating call by call in one process, medians of `iters` rounds of event times:
  * the training step with the filter set against the separate-call step it extends (fused_backward off, eager SH
    Adam): the like-for-like price of brush_filter3d_apply + brush_filter3d_backward;
  * the same against the default step (fused backward + Adam, deferred SH block): what a user gives up until the two
    maps are folded into the cull and the VJP kernels;
  * brush_filter3d_rates at 100 and 300 views;
  * device copies moving the byte counts of the two per-step maps (apply: 20 B read + 16 B written per splat;
    transpose: 36 B read + 16 B written), as a yardstick for their kernel times.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, in a run of its own, which gives k_filter3d_apply /
k_filter3d_backward / k_filter3d_rates / k_filter3d_fill_unseen next to the copy kernels and the step's own.

    python tools/filter3d_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/filter3d_prof.py --iters 10

profiles/filter3d_prof.json is the first form's output; profiles/filter3d_kernel_stats.csv the per-kernel statistics of a
kernel trace of the second.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd.filter3d import view_records  # noqa: E402
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


def _orbit(count, w, h):
    """`count` cameras on a circle of radius 8 around the cloud, looking at its centre."""
    views = []
    for i in range(count):
        a = 2.0 * math.pi * i / count
        pos = [8.0 * math.sin(a), 0.0, -8.0 * math.cos(a)]
        rot = [0.0, -math.sin(a / 2.0), 0.0, math.cos(a / 2.0)]  # about +y: the camera's +z axis points at the origin
        views.append((brush_amd.Camera(pos, rot, 2 * np.arctan(0.5), 2 * np.arctan(0.5 * h / w), (0.5, 0.5)), (w, h)))
    return views


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
    w, h, n = a.width, a.height, a.splats
    c = synthetic_cloud(n, a.sh_degree, seed=4)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gen = torch.Generator(device="cpu").manual_seed(0)
    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    means = torch.from_numpy(c["means"]).to(dev)
    records = {k: torch.from_numpy(view_records(_orbit(k, w, h))).to(dev) for k in (100, 300)}
    filt = brush_amd.filter3d_rates(means, records[100])
    seen = float((filt < filt.max()).float().mean())

    def trainer(**kw):
        fused = kw.pop("fused", True)
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0, **kw))
        tr.fused_backward = fused
        return s, tr

    steps = {}
    s, tr = trainer(filter3d=True)
    tr.set_filter3d(filt)
    steps["filter3d"] = lambda s=s, tr=tr: tr.step(s, cam, gt)
    s, tr = trainer(fused=False, deferred_sh_adam=False)
    steps["separate"] = lambda s=s, tr=tr: tr.step(s, cam, gt)
    s, tr = trainer()
    steps["default"] = lambda s=s, tr=tr: tr.step(s, cam, gt)
    res = {f"train_step_{k}_ms": v for k, v in _timed(steps, a.iters).items()}

    rates = {f"rates_{k}_views_ms": (lambda r=r: brush_amd.filter3d_rates(means, r)) for k, r in records.items()}
    res.update(_timed(rates, a.iters))

    # the two per-step maps alone, and copies that move as many bytes (a copy of B bytes reads B and writes B)
    ls, ro = torch.from_numpy(c["log_scales"]).to(dev), torch.from_numpy(c["raw_opac"]).to(dev)
    v_l, v_o = torch.rand_like(ls), torch.rand_like(ro)
    from brush_amd import _lib
    from brush_amd.filter3d import apply_into, backward_into

    stream = _lib.current_stream(dev)
    src = {b: torch.empty(b * n // 2, dtype=torch.uint8, device=dev) for b in (36, 52)}
    dst = {b: torch.empty_like(t) for b, t in src.items()}
    alone = {"apply_ms": lambda: apply_into(ls, ro, filt, n, stream),
             "copy_36B_per_splat_ms": lambda: dst[36].copy_(src[36]),
             "backward_ms": lambda: backward_into(ls, ro, filt, n, v_l, v_o, stream),
             "copy_52B_per_splat_ms": lambda: dst[52].copy_(src[52])}
    res.update(_timed(alone, a.iters))
    line = {"splats": n, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), "fraction_of_splats_seen_by_100_views": seen, **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
