#!/usr/bin/env python3
"""Cost of a training step under TrainConfig.strategy = "mcmc" next to the two steps the library already had, alternating
the three call by call in one process, so clock and thermal drift hit all alike; medians of event times over `iters`
SplatTrainer steps on one synthetic scene (default S1: 1 M splats, 1080p, SH 3; no refinement in range):
  * fused     the default step: brush_render_backward_adam with the deferred SH block (the bench's path);
  * separate  fused_backward = False, deferred_sh_adam = False: brush_render_backward + brush_adam_step;
  * mcmc      the separate-call step plus brush_mcmc_reg_grads and brush_mcmc_inject_noise.
mcmc - separate is what the two new kernels cost in situ; mcmc - fused is the price of leaving the fused path (the
number that decides whether the regularisers get folded into the fused backward).
With --e2e DATASET instead: that scene (the tests' end-to-end scene, written out as a NeRF-synthetic tree) trained
with both strategies on the same seed (final PSNR and splat count, recorded, never gated).
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_mcmc_inject_noise / k_mcmc_reg_grads next to
k_adam.

    python tools/mcmc_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    python tools/mcmc_prof.py --e2e DATASET [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mcmc_prof.py --iters 10

profiles/mcmc_prof.json is the first form's output, profiles/mcmc_e2e.json the second's; profiles/mcmc_kernel_stats.csv
the per-kernel statistics of a kernel trace of the third.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def e2e(dataset):
    from brush_amd.train_loop import load_dataset, train_scene

    out = {}
    data, _ = load_dataset(dataset)
    for name, cfg in (("default", brush_amd.TrainConfig(warmup_steps=50, refine_every=50)),
                      ("mcmc", brush_amd.TrainConfig(strategy="mcmc", warmup_steps=50, refine_every=50,
                                                     mcmc_cap_max=3000))):
        rows = []
        _, log = train_scene(data, cfg, steps=600, init_count=2000, sh_degree=3, seed=5, eval_every=200,
                             on_eval=lambda r, s: rows.append(r))
        out[name] = {"psnr": [r.psnr for r in rows], "splats": [r.splats for r in rows],
                     "train_seconds": log.train_seconds, "final_loss": float(np.mean(log.losses[-50:]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e2e", metavar="DATASET", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.e2e:
        line = {"scene": "the tests' end-to-end scene (16 train / 4 eval views of 3000 known splats), 600 steps, seed 5, "
                         "2000 initial splats", "device": torch.cuda.get_device_name(dev), **e2e(a.e2e)}
    else:
        w, h = a.width, a.height
        c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
        cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                               2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
        gt = torch.rand((h, w, 3), generator=torch.Generator(device="cpu").manual_seed(0)).to(dev)
        steps = {}
        for name, cfg, fused in (
                ("fused", brush_amd.TrainConfig(max_refine_step=0), True),
                ("separate", brush_amd.TrainConfig(max_refine_step=0, deferred_sh_adam=False), False),
                ("mcmc", brush_amd.TrainConfig(max_refine_step=0, strategy="mcmc"), True)):
            s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                              "log_scales")))
            tr = brush_amd.SplatTrainer(s, cfg)
            tr.fused_backward = fused
            steps[name] = (lambda s=s, tr=tr: tr.step(s, cam, gt))
        t = _timed(steps, a.iters)
        line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
                "device": torch.cuda.get_device_name(dev), **{f"train_step_{k}_ms": v for k, v in t.items()}}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
