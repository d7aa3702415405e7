#!/usr/bin/env python3
"""Cost of the per-view bilateral grids (brush_bilagrid_forward / _backward_adam) next to the plain training step and
next to exposure compensation, alternating the legs call by call in one process, so clock and thermal drift hit all
alike; medians of event times:
  * `iters` calls of the three ABI entry points alone on one image (default 1080p, grid 16 x 16 x 8), with the exposure
    entry points on the same image beside them (the yardstick: the same streaming passes with one 3x4 map).  The image
    is uniform noise, so every wave touches every luminance level: the worst case for both kernels; `*_smooth_ms` are
    the same calls on a low-frequency image, where a wave touches two or three levels, as in a photograph;
  * `iters` SplatTrainer steps (fused backward + Adam with the deferred SH block, the bench's path; no refinement) on
    one synthetic scene (default S1: 1 M splats, 1080p, SH 3), without a colour model, with an ExposureTable and with
    a BilagridTable of two views drawn in turn.
The plain leg runs the kernels the library had before the option existed (tools/kernel_diff.py: identical), so "plain" is
also the parent's figure on the same box in the same run.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_bilagrid_forward / k_bilagrid_backward /
k_bilagrid_finalize next to k_exposure_forward / k_exposure_backward (the event times above include the launches).

    python tools/bilagrid_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--shape 16,16,8] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bilagrid_prof.py --iters 10

profiles/bilagrid_prof.json is the first form's output; profiles/bilagrid_kernel_stats.csv the per-kernel statistics of
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
from brush_amd import bilagrid as BG  # noqa: E402
from brush_amd.exposure import ExposureTable, workspace_bytes  # noqa: E402
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
    ap.add_argument("--shape", default="16,16,8", help="GW,GH,GL")
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
    shape = BG.check_shape([int(x) for x in a.shape.split(",")])
    gw, gh, gl = shape
    G = (BG.bilagrid_identity(shape) + 0.05 * torch.randn((gl, gh, gw, 12), generator=gen)).to(dev)
    g1, g2, v_G = torch.zeros_like(G), torch.zeros_like(G), torch.zeros_like(G)
    gbytes = BG.workspace_bytes(w, h, shape)
    gws = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    gcfg = _lib.BrushBilagridAdam(1e-4, 0.9, 0.999, 1e-15, 10.0, 1)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    smooth = torch.stack([0.5 + 0.45 * torch.sin(6.0 * xx + 2.0 * yy), 0.5 + 0.45 * torch.sin(3.0 * xx - 5.0 * yy + 1.0),
                          0.5 + 0.45 * torch.cos(4.0 * xx + 4.0 * yy), torch.ones_like(xx)], dim=-1).contiguous().to(dev)
    abi = {
        "bilagrid_forward_smooth": lambda: _lib.check(l.brush_bilagrid_forward(
            smooth.data_ptr(), G.data_ptr(), gw, gh, gl, w, h, out.data_ptr(), stream), "forward"),
        "bilagrid_backward_smooth": lambda: _lib.check(l.brush_bilagrid_backward(
            smooth.data_ptr(), v_out.data_ptr(), G.data_ptr(), gw, gh, gl, w, h, v_pred.data_ptr(), v_G.data_ptr(),
            gws.data_ptr(), gbytes, stream), "backward"),
        "bilagrid_forward": lambda: _lib.check(l.brush_bilagrid_forward(pred.data_ptr(), G.data_ptr(), gw, gh, gl, w, h,
                                                                        out.data_ptr(), stream), "forward"),
        "bilagrid_backward": lambda: _lib.check(l.brush_bilagrid_backward(
            pred.data_ptr(), v_out.data_ptr(), G.data_ptr(), gw, gh, gl, w, h, v_pred.data_ptr(), v_G.data_ptr(),
            gws.data_ptr(), gbytes, stream), "backward"),
        "bilagrid_backward_adam": lambda: _lib.check(l.brush_bilagrid_backward_adam(
            pred.data_ptr(), v_out.data_ptr(), C.byref(gcfg), gw, gh, gl, w, h, v_pred.data_ptr(), G.data_ptr(),
            g1.data_ptr(), g2.data_ptr(), v_G.data_ptr(), gws.data_ptr(), gbytes, stream), "backward_adam"),
        "exposure_forward": lambda: _lib.check(l.brush_exposure_forward(pred.data_ptr(), E.data_ptr(), w, h, out.data_ptr(),
                                                               stream), "forward"),
        "exposure_backward": lambda: _lib.check(l.brush_exposure_backward(pred.data_ptr(), v_out.data_ptr(), E.data_ptr(), w, h,
                                                                 v_pred.data_ptr(), v_E.data_ptr(), ws.data_ptr(),
                                                                 nbytes, stream), "backward"),
        "exposure_backward_adam": lambda: _lib.check(l.brush_exposure_backward_adam(
            pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), w, h, v_pred.data_ptr(), E.data_ptr(), m1.data_ptr(),
            m2.data_ptr(), v_E.data_ptr(), ws.data_ptr(), nbytes, stream), "backward_adam"),
    }
    res = {f"abi_{k}_ms": v for k, v in _timed(abi, a.iters).items()}
    npix = w * h
    res.update(forward_bytes=32 * npix, backward_bytes=48 * npix, grid_bytes=int(G.numel()) * 4,
               bilagrid_workspace_bytes=gbytes)

    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    steps = {}
    for with_table in (False, True, "bilagrid"):
        s = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                          "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0))
        if with_table == "bilagrid":
            table = BG.BilagridTable(2, dev, 2e-3, shape, 10.0)
            turn = [0]

            def fn(s=s, tr=tr, table=table, turn=turn):
                turn[0] ^= 1
                tr.step(s, cam, gt, view_index=turn[0], bilagrids=table)
            steps["bilagrid"] = fn
        elif with_table:
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
    res["train_step_bilagrid_ms"] = t["bilagrid"]
    line = {"shape": list(shape), "splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
