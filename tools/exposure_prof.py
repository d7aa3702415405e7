#!/usr/bin/env python3
"""Cost of per-view exposure compensation (brush_exposure_forward / _backward_adam) next to the plain training step,
alternating the two call by call in one process, so clock and thermal drift hit both alike; medians of event times:
  * `iters` calls of the three ABI entry points alone on one image (default 1080p), with brush_l1_ssim_loss on the same
    image beside them, once as the trainer calls it and once with ssim_weight = 0, which is k_l1_backward: one
    image-sized streaming pass (pred and a 3-channel f32 target in, v_pred out), the yardstick for the bytes the
    exposure kernels move (`*_bytes` in the output are the bytes each pass must move);
  * `iters` SplatTrainer steps (fused backward + Adam with the deferred SH block, the bench's path; no refinement) on
    one synthetic scene (default S1: 1 M splats, 1080p, SH 3), without the option and with an ExposureTable of two views
    drawn in turn.
The plain leg runs the kernels the library had before the option existed (tools/kernel_diff.py: identical), so "plain" is
also the parent's figure on the same box in the same run.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_exposure_forward / k_exposure_backward /
k_exposure_finalize next to k_l1_backward and the SSIM kernels (the event times above include the launches).

    python tools/exposure_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/exposure_prof.py --iters 10

profiles/exposure_prof.json is the first form's output; profiles/exposure_kernel_stats.csv the per-kernel statistics of
a kernel trace of the second.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd.exposure import ExposureTable, workspace_bytes  # noqa: E402
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
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.rand((h, w, 4), generator=gen).to(dev)
    v_out = (torch.rand((h, w, 4), generator=gen) - 0.5).to(dev)
    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    E = torch.tensor([0.9, 0.02, 0.0, 0.01, 0.0, 0.8, 0.01, 0.02, 0.03, 0.0, 0.95, 0.0], device=dev)
    m1, m2, v_E = torch.zeros(12, device=dev), torch.zeros(12, device=dev), torch.zeros(12, device=dev)
    out, v_pred = torch.empty_like(pred), torch.empty_like(pred)
    nbytes = workspace_bytes(w, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    l = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    cfg = _lib.BrushExposureAdam(1e-4, 0.9, 0.999, 1e-15, 1e-6, 1)
    abi = {
        "forward": lambda: _lib.check(l.brush_exposure_forward(pred.data_ptr(), E.data_ptr(), w, h, out.data_ptr(),
                                                               stream), "forward"),
        "backward": lambda: _lib.check(l.brush_exposure_backward(pred.data_ptr(), v_out.data_ptr(), E.data_ptr(), w, h,
                                                                 v_pred.data_ptr(), v_E.data_ptr(), ws.data_ptr(),
                                                                 nbytes, stream), "backward"),
        "backward_adam": lambda: _lib.check(l.brush_exposure_backward_adam(
            pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), w, h, v_pred.data_ptr(), E.data_ptr(), m1.data_ptr(),
            m2.data_ptr(), v_E.data_ptr(), ws.data_ptr(), nbytes, stream), "backward_adam"),
        "l1_ssim_loss": lambda: l1_ssim_loss(pred, gt, 0.2),
        "l1_loss": lambda: l1_ssim_loss(pred, gt, 0.0),
    }
    res = {f"abi_{k}_ms": v for k, v in _timed(abi, a.iters).items()}
    npix = w * h
    res.update(forward_bytes=32 * npix, backward_bytes=48 * npix, l1_backward_bytes=(16 + 12 + 16) * npix)

    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    steps = {}
    for with_table in (False, True):
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0))
        if with_table:
            table = ExposureTable(2, dev, 1e-2, 1e-6)
            turn = [0]

            def fn(s=s, tr=tr, table=table, turn=turn):
                turn[0] ^= 1
                tr.step(s, cam, gt, view_index=turn[0], exposures=table)
            steps["exposure"] = fn
        else:
            steps["plain"] = (lambda s=s, tr=tr: tr.step(s, cam, gt))
    t = _timed(steps, a.iters)
    res["train_step_plain_ms"], res["train_step_exposure_ms"] = t["plain"], t["exposure"]
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
