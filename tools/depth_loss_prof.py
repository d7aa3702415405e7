#!/usr/bin/env python3
"""Cost of depth supervision (brush_depth_loss) next to the same loss written as PyTorch ops and next to the plain
training step, alternating the legs call by call in one process, so clock and thermal drift hit all alike; medians of
event times:
  * `iters` calls of brush_depth_loss alone on one image (default 1080p), with a u16 and with an f32 target, in both
    modes, and metrics-only (no gradient outputs); beside them the same loss and gradients as PyTorch elementwise ops
    (`torch_ops_*`: what a user would write between the depth forward and backward without the kernel, the f32 target
    already on the device) and brush_l1_ssim_loss with ssim_weight = 0 (k_l1_backward: one image-sized streaming pass,
    the yardstick for the bytes; `*_bytes` in the output are the bytes each pass must move, whole lines of pred and
    v_pred counted for the stride-16 alpha accesses);
  * `iters` SplatTrainer steps on one synthetic scene (default S1: 1 M splats, 1080p, SH 3; no refinement): the plain
    fused step (the bench's path), the separate-call step without depth (fused_backward = False: what a supervised
    step is built from) and the supervised step (depth forward, brush_depth_loss, depth backward, brush_adam_step).
The plain legs run the kernels the library had before the option existed (tools/kernel_diff.py: identical).
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_depth_loss / k_depth_loss_finalize next to
k_l1_backward and the elementwise kernels of the PyTorch form (the event times above include the launches).

    python tools/depth_loss_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/depth_loss_prof.py --iters 10

profiles/depth_loss_prof.json is the first form's output; profiles/depth_loss_kernel_stats.csv the per-kernel
statistics of a kernel trace of the second.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd.depth_loss import depth_loss_into, workspace_bytes  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402
from brush_amd.train import l1_ssim_loss  # noqa: E402


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


def torch_depth_loss(pred, depth, target, v_pred, weight, scale, offset, alpha_min, mode):
    """brush_depth_loss as PyTorch ops: (loss, v_depth), v_pred's alpha channel updated in place."""
    a = pred[..., 3]
    t = target * scale + offset
    valid = torch.isfinite(target) & (target > 0) & (t > 0) & (depth > 0) & (a >= alpha_min)
    c = weight / a.numel()
    if mode == "depth":
        d = depth / a
        r = d - t
        g = c * torch.sign(r)
        v_d, v_a = g / a, -(g * d) / a
    else:
        q = a / depth
        r = q - t
        g = c * torch.sign(r)
        v_d, v_a = -(g * q) / depth, g / depth
    zero = torch.zeros_like(r)
    loss = c * torch.where(valid, r.abs(), zero).sum(dtype=torch.float64)
    v_pred[..., 3] += torch.where(valid, v_a, zero)
    return loss, torch.where(valid, v_d, zero)


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
    npix = w * h
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.rand((h, w, 4), generator=gen).to(dev)
    depth = (pred[..., 3] * (0.5 + 8.0 * torch.rand((h, w), generator=gen).to(dev))).contiguous()
    mm = (500.0 + 8000.0 * torch.rand((h, w), generator=gen)).numpy()
    mm[torch.rand((h, w), generator=gen).numpy() < 0.2] = 0.0
    t16 = torch.from_numpy(mm.astype(np.uint16)).to(dev)
    t32 = torch.from_numpy((mm * 0.001).astype(np.float32)).to(dev)
    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    v_pred = torch.zeros_like(pred)
    ws = torch.empty(workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    accum = torch.zeros(1, device=dev)

    def k(target, scale, mode, grads=True):
        return lambda: depth_loss_into(pred, depth, target, v_pred if grads else None, weight=0.1, scale=scale,
                                       mode=mode, loss_accum=accum, want_v_depth=grads, workspace=ws)

    abi = {
        "kernel_u16_depth": k(t16, 0.001, "depth"), "kernel_f32_depth": k(t32, 1.0, "depth"),
        "kernel_u16_disparity": k(t16, 0.001, "disparity"), "kernel_f32_disparity": k(t32, 1.0, "disparity"),
        "kernel_u16_metrics_only": k(t16, 0.001, "depth", False),
        "torch_ops_f32_depth": lambda: torch_depth_loss(pred, depth, t32, v_pred, 0.1, 1.0, 0.0, 0.5, "depth"),
        "torch_ops_f32_disparity": lambda: torch_depth_loss(pred, depth, t32, v_pred, 0.1, 1.0, 0.0, 0.5, "disparity"),
        "l1_loss": lambda: l1_ssim_loss(pred, gt, 0.0),
    }
    res = {f"abi_{name}_ms": v for name, v in _timed(abi, a.iters).items()}
    res.update(kernel_u16_bytes=58 * npix, kernel_f32_bytes=60 * npix, kernel_metrics_only_u16_bytes=22 * npix,
               l1_backward_bytes=(16 + 12 + 16) * npix)

    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    steps = {}
    for name, fused, target, scale in (("plain_fused", True, None, 1.0), ("plain_separate", False, None, 1.0),
                                       ("depth_u16", True, t16, 0.001), ("depth_f32", True, t32, 1.0)):
        s = brush_amd.Splats(*(torch.from_numpy(c[key]).to(dev) for key in ("means", "sh", "quats", "raw_opac",
                                                                            "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0, depth_weight=0.1))
        tr.fused_backward = fused
        steps[name] = (lambda s=s, tr=tr, target=target, scale=scale:
                       tr.step(s, cam, gt, gt_depth=target, depth_scale=scale))
    res.update({f"train_step_{name}_ms": v for name, v in _timed(steps, a.iters).items()})
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
