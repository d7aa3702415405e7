#!/usr/bin/env python3
"""Times the training loop against the bare trainer step on the headline shape (1920x1080 RGB, 1 048 576 splats,
SH degree 3, the S1 cloud of bench.py), in one process, the variants alternating round by round:

  step_f32_resident  SplatTrainer.step with a resident f32 torch.rand target (bench's training-iteration shape)
  step_u8_resident   the same step with a resident u8 target (brush_l1_ssim_loss_gt)
  train_loop         TrainLoop.step over a resident multi-view synthetic dataset (random view, u8 image, loss log)
  step_f32_upload    for comparison only: step_f32_resident with its f32 target copied from host memory every step
                     (the reference's image_to_tensor upload per view)

Refinement is off (max_refine_step = 0) so that every variant runs the same splat count.  Prints one line per variant
(median, min and max ms/step over the rounds) and writes them to --json.

    python tools/train_loop_prof.py [--steps 20] [--rounds 7] [--views 8] [--json profiles/train_loop_prof.json]
    python tools/train_loop_prof.py --loss-only [--iters 50]   # u8 / f32 loss calls only, for
        rocprofv3 --kernel-trace --stats (k_ssim_forward, k_ssim_backward, k_l1_backward of each element type)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd.dataset import Dataset, Scene, SceneView  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402
from brush_amd.train import l1_ssim_loss  # noqa: E402
from brush_amd.train_loop import TrainLoop  # noqa: E402

N, W, H, DEG = 1 << 20, 1920, 1080, 3


def orbit_camera(k):
    """bench.py's camera (render_bench.rs:163-174) orbited about y by 0.35 k."""
    focal = brush_amd.fov_to_focal(math.pi * 0.5, W)
    ang = 0.35 * k
    return brush_amd.Camera([-8.0 * math.sin(ang), 0.0, -8.0 * math.cos(ang)], [0.0, math.sin(ang / 2), 0.0,
                            math.cos(ang / 2)], brush_amd.focal_to_fov(focal, W), brush_amd.focal_to_fov(focal, H),
                            (0.5, 0.5))


def loss_only(iters):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.random((H, W, 4), dtype=np.float32)).to(dev)
    gt8 = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    gt32 = gt8.float() / 255.0
    for _ in range(iters):
        for gt in (gt8, gt32):
            l1_ssim_loss(pred, gt, 0.2, 11)  # k_ssim_forward / k_ssim_backward
            l1_ssim_loss(pred, gt, 0.0, 11)  # k_l1_backward
    torch.cuda.synchronize()
    print(f"loss-only: {iters} x (u8, f32) x (ssim 0.2, L1 only) at {W}x{H}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per variant per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--views", type=int, default=8, help="training views of the loop's synthetic dataset")
    ap.add_argument("--json", default=None)
    ap.add_argument("--loss-only", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.loss_only:
        return loss_only(a.iters)
    dev = torch.device("cuda:0")
    cloud = synthetic_cloud(N, DEG, seed=4)
    p = {k: torch.from_numpy(v).to(dev) for k, v in cloud.items()}
    cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0)
    cam = orbit_camera(0)

    splats = brush_amd.Splats(p["means"], p["sh"], p["quats"], p["raw_opac"], p["log_scales"])
    trainer = brush_amd.SplatTrainer(splats, cfg)
    gt32 = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
    gt8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    host32 = np.random.default_rng(1).random((H, W, 3), dtype=np.float32)  # pageable host memory

    rng = np.random.default_rng(2)
    views = [SceneView(f"v{k}", orbit_camera(k), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
             for k in range(a.views)]
    total = (a.rounds + 1) * a.steps
    loop = TrainLoop(Dataset(Scene(views)), cfg, steps=total,
                     init=brush_amd.Splats(p["means"], p["sh"], p["quats"], p["raw_opac"], p["log_scales"]), seed=3)

    variants = {
        "step_f32_resident": lambda: trainer.step(splats, cam, gt32),
        "step_u8_resident": lambda: trainer.step(splats, cam, gt8),
        "train_loop": loop.step,
        "step_f32_upload": lambda: trainer.step(splats, cam, torch.from_numpy(host32).to(dev)),
    }
    times = {k: [] for k in variants}
    for r in range(a.rounds + 1):  # round 0 warms up (first launches, allocator, tables)
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                variants[k]()
            torch.cuda.synchronize()
            if r > 0:
                times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    trainer.sync(splats)
    _, log = loop.finish()
    res = {"shape": f"{W}x{H} RGB, {N} splats, SH {DEG}", "steps_per_round": a.steps, "rounds": a.rounds,
           "loop_views": a.views, "loop_image_bytes": log.image_bytes,
           "upload_bytes_per_step": int(host32.nbytes), "variants": {}}
    for k, ts in times.items():
        res["variants"][k] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)),
                              "max_ms": float(np.max(ts)), "rounds_ms": [round(t, 4) for t in ts]}
        print(f"{k:20s} median {np.median(ts):.4f} ms/step  (min {np.min(ts):.4f}, max {np.max(ts):.4f}, "
              f"{len(ts)} rounds of {a.steps})")
    assert np.isfinite(log.losses).all()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
