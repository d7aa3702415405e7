#!/usr/bin/env python3
"""Cost of the camera-pose gradient (brush_render_backward_pose / _adam_pose) next to the plain backward, alternating
the two call by call in one process, so clock and thermal drift hit both alike; medians of event times:
  * `iters` forward + backward passes through the C ABI on one synthetic scene (default S1: 1 M splats, 1080p, SH 3),
    default and deterministic mode, with and without the pose output (the forward is the same call in both);
  * `iters` SplatTrainer steps (fused backward + Adam with the deferred SH block, the bench's path; no refinement),
    without poses and with a PoseTable (its host-side update of the drawn view included).
The plain legs run the kernels the library had before the pose gradient existed (tools/kernel_diff.py: identical), so
"plain" is also the parent's figure on the same box in the same run.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_view_grad / k_view_grad_finalize next to
k_depth_means_grad / k_sum_isect_depth and the parameter VJP.

    python tools/pose_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pose_prof.py --iters 10

profiles/pose_prof.json is the first form's output; profiles/pose_kernel_stats.csv the per-kernel statistics of a kernel
trace of the second.
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
from brush_amd.pose import PoseTable  # noqa: E402
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
    means, log_scales, quats, sh, raw = (torch.from_numpy(c[k]).to(dev) for k in ("means", "log_scales", "quats", "sh",
                                                                                   "raw_opac"))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gen = torch.Generator(device="cpu").manual_seed(0)
    v_out = torch.rand((h, w, 4), generator=gen).to(dev)
    pose = R.pose_buffers(a.splats, dev)
    block = torch.empty(R.grad_block_layout(a.splats, sh.shape[1])[1], device=dev)

    def fwd_bwd(det, with_pose):
        def fn():
            img, aux, u = R._forward_impl(cam, (w, h), means, log_scales, quats, sh, raw, False, None, deterministic=det)
            R._backward_impl(u, aux, means, log_scales, quats, raw, sh.shape[1], img, v_out, block=block,
                             pose=pose if with_pose else None)
        return fn

    res = {}
    for det in (False, True):
        t = _timed({"plain": fwd_bwd(det, False), "pose": fwd_bwd(det, True)}, a.iters)
        sfx = "_det" if det else ""
        res[f"fwd_bwd_plain{sfx}_ms"], res[f"fwd_bwd_pose{sfx}_ms"] = t["plain"], t["pose"]

    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    steps = {}
    for with_pose in (False, True):
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0))
        if with_pose:
            # two views drawn in turn: the update of a view waits for a copy issued one step earlier, as in a run
            table = PoseTable(2, 1e-3, 5e-4, 1e-6)
            turn = [0]

            def fn(s=s, tr=tr, table=table, turn=turn):
                turn[0] ^= 1
                tr.step(s, cam, gt, view_index=turn[0], poses=table)
            steps["pose"] = fn
        else:
            steps["plain"] = (lambda s=s, tr=tr: tr.step(s, cam, gt))
    t = _timed(steps, a.iters)
    res["train_step_plain_ms"], res["train_step_pose_ms"] = t["plain"], t["pose"]
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
