#!/usr/bin/env python3
"""Cost of a background colour and a loss mask (brush_compose_forward / _backward) next to the plain training step, the
variants alternating call by call in one process, so clock and thermal drift hit all alike; medians of device-event
times around runs that end in a synchronise:
  * `iters` calls of the two ABI entry points alone on one image (default 1080p, u8 RGB target, mask and background),
    with brush_l1_ssim_loss at ssim_weight = 0 beside them: k_l1_backward, one image-sized streaming pass, the yardstick
    for the bytes the compose kernels move (`*_bytes` in the output are the bytes each pass must move);
  * `iters` SplatTrainer steps (fused backward + Adam with the deferred SH block, the bench's path; no refinement) on
    one synthetic scene (default S1: 1 M splats, 1080p, SH 3): no option, a fixed background, a random background, a
    mask, and both.
The plain leg issues the launches the library issued before the option existed.  --plain-only times that leg alone:
run with BRUSH_HIP_LIB pointing at another build of the library, in turn with the product one, it compares two builds.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_compose_forward / k_compose_backward next
to k_l1_backward and the SSIM kernels (the event times above include the launches).

    python tools/compose_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/compose_prof.py --iters 10

profiles/compose_prof.json is the first form's output; profiles/compose_kernel_stats.csv the per-kernel statistics of a
kernel trace of the second.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402
from brush_amd.train import l1_ssim_loss  # noqa: E402


def _timed(fns, iters):
    """{name: (median ms, min ms, max ms)} for the callables of `fns`, called in alternation."""
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
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true", help="time the plain training step alone")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h = a.width, a.height
    npix = w * h
    gen = torch.Generator(device="cpu").manual_seed(0)
    gt = (torch.rand((h, w, 3), generator=gen) * 255).to(torch.uint8).to(dev)
    mask = ((torch.rand((h, w), generator=gen) > 0.25).to(torch.uint8) * 255).to(dev)
    res = {}
    if a.plain_only:  # a build from before the option lacks its entry points: leave what it lacks unbound
        import ctypes

        handle = ctypes.CDLL(_lib.LIB_PATH)
        _lib._SYMBOLS[:] = [sym for sym in _lib._SYMBOLS if hasattr(handle, sym[0])]
    if not a.plain_only:
        from brush_amd import compose_backward, compose_forward

        pred = torch.rand((h, w, 4), generator=gen).to(dev)
        v_out = (torch.rand((h, w, 4), generator=gen) - 0.5).to(dev)
        bg = torch.tensor([0.25, 0.5, 1.0]).to(dev)
        bufs = (torch.empty_like(pred), torch.empty((h, w, 3), device=dev))
        v_pred = torch.empty_like(pred)
        gt32 = gt.float() / 255
        abi = {
            "forward": lambda: compose_forward(pred, gt, background=bg, mask=mask, out=bufs),
            "backward": lambda: compose_backward(v_out, background=bg, mask=mask, out=v_pred),
            "l1_loss": lambda: l1_ssim_loss(pred, gt32, 0.0),
        }
        for k, (med, lo, hi) in _timed(abi, a.iters).items():
            res[f"abi_{k}_ms"] = med
        res.update(forward_bytes=(16 + 3 + 1 + 16 + 12) * npix, backward_bytes=(16 + 1 + 16) * npix,
                   l1_backward_bytes=(16 + 12 + 16) * npix)

    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    variants = {"plain": {}}
    if not a.plain_only:
        variants.update(background={"background": (0.25, 0.5, 1.0)}, random={"background": "random"},
                        mask={"gt_mask": mask}, both={"background": "random", "gt_mask": mask})
    steps = {}
    for name, kw in variants.items():
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0))
        steps[name] = (lambda s=s, tr=tr, kw=kw: tr.step(s, cam, gt, **kw))
    for k, (med, lo, hi) in _timed(steps, a.iters).items():
        res[f"train_step_{k}_ms"] = med
        res[f"train_step_{k}_min_max_ms"] = [lo, hi]
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "library": _lib.version(), "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
