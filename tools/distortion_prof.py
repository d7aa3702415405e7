#!/usr/bin/env python3
"""Cost of the depth-distortion term (brush_amd/distortion.py) next to its yardsticks of the same commit, alternating
the legs call by call in one process, so clock and thermal drift hit all alike; medians of event times:
  * `iters` calls of each replay alone on one finished depth forward of the scene (default S1: 1 M splats, 1080p):
    brush_render_distortion in both modes next to brush_render_features at C = 3 (the same walk, 3 outputs instead of
    4), brush_distortion_compact_grads in both modes next to brush_render_features_backward at C = 3 (the same walk, 3
    float atomics per record and quadrant instead of 7), and distortion_loss_into (torch: a fill and a float64 sum);
  * `iters` SplatTrainer steps on the same scene (no refinement): the depth-supervised separate-call step (the parent
    commit's step the term rides on), the step with the distortion term alone, and the step with both; the plain fused
    step (the bench's path) for reference.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_distortion_quad and k_distortion_grad_quad
next to the step's other kernels (the event times above include the launches).

    python tools/distortion_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/distortion_prof.py --iters 10

profiles/distortion_prof.json is the first form's output.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import distortion as D  # noqa: E402
from brush_amd import render as R  # noqa: E402
from brush_amd.features import feature_grads_from_aux, features_from_aux  # noqa: E402
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
    w, h, n = a.width, a.height, a.splats
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gen = torch.Generator(device="cpu").manual_seed(0)
    c = synthetic_cloud(n, a.sh_degree, seed=4)
    means, log_scales, sh, raw = (torch.from_numpy(c[k]).to(dev) for k in ("means", "log_scales", "sh", "raw_opac"))
    quats = torch.from_numpy(c["quats"]).to(dev)
    quats = (quats / quats.norm(dim=1, keepdim=True)).contiguous()

    # one finished depth forward, default mode: what every replay below walks
    bufs = R._depth_buffers(n, (w, h), dev)
    with torch.no_grad():
        img, aux, u = R._forward_impl(cam, (w, h), means, log_scales, quats, sh, raw, False, None, deterministic=False,
                                      expect_backward=False, depth=bufs)
    cfgs = {"depth": D.distortion_config("depth"), "ndc": D.distortion_config("ndc", 0.2, 1000.0)}
    stats = {k: D.distortion_from_aux(u, aux, bufs[1], cfg) for k, cfg in cfgs.items()}
    out = torch.empty((h, w, 4), device=dev)
    v = torch.full((h, w), 1.0 / (w * h), device=dev)
    rows = torch.zeros((n, D.COMPACT_STRIDE), device=dev)
    feats = torch.rand((n, 3), generator=gen).to(dev)
    v_img = torch.randn((h, w, 3), generator=gen).to(dev)
    v_feats = torch.zeros((n, 3), device=dev)
    accum = torch.zeros(1, device=dev)
    abi = {
        "features_c3": lambda: features_from_aux(u, aux, feats),
        "distortion_depth": lambda: D.distortion_from_aux(u, aux, bufs[1], cfgs["depth"], out=out),
        "distortion_ndc": lambda: D.distortion_from_aux(u, aux, bufs[1], cfgs["ndc"], out=out),
        "features_backward_c3": lambda: feature_grads_from_aux(u, aux, v_img, v_feats),
        "distortion_grads_depth": lambda: D.distortion_compact_grads_from_aux(u, aux, bufs[1], cfgs["depth"],
                                                                              stats["depth"], v, rows),
        "distortion_grads_ndc": lambda: D.distortion_compact_grads_from_aux(u, aux, bufs[1], cfgs["ndc"], stats["ndc"],
                                                                            v, rows),
        "distortion_loss_into": lambda: D.distortion_loss_into(stats["depth"], v, weight=100.0, loss_accum=accum),
    }
    res = {f"abi_{name}_ms": t for name, t in _timed(abi, a.iters).items()}
    res.update(num_visible=aux.read_num_visible(), num_intersections=aux.read_num_intersections(),
               mean_distortion_depth=float(stats["depth"][..., 0].mean()))

    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    t32 = (5.0 + 1.5 * xs / w - 1.0 * ys / h).to(dev).contiguous()
    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    steps = {}
    for name, fused, target, dw in (("plain_fused", True, None, 0.0), ("depth_f32", True, t32, 0.0),
                                    ("distortion", True, None, 100.0), ("depth_f32_and_distortion", True, t32, 100.0)):
        s = brush_amd.Splats(*(torch.from_numpy(c[key]).to(dev) for key in ("means", "sh", "quats", "raw_opac",
                                                                            "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0, depth_weight=0.1, distortion_weight=dw,
                                                             distortion_from_step=0))
        tr.fused_backward = fused
        steps[name] = (lambda s=s, tr=tr, target=target: tr.step(s, cam, gt, gt_depth=target))
    old = R.DETERMINISTIC
    R.DETERMINISTIC = False  # the term's only mode
    try:
        res.update({f"train_step_{name}_ms": t for name, t in _timed(steps, a.iters).items()})
    finally:
        R.DETERMINISTIC = old
    line = {"splats": n, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
