#!/usr/bin/env python3
"""Cost of the depth-normal consistency term (brush_amd/normal_loss.py) next to the depth-supervised step and the plain
separate-call step of the same commit, alternating the legs call by call in one process, so clock and thermal drift hit
all alike; medians of event times:
  * `iters` calls of each of the three kernels alone: brush_splat_normals and brush_splat_normals_backward on the
    scene's splats (default 1 M), brush_normal_loss on one image (default 1080p) with every gradient output and in the
    normals-only form; beside them brush_depth_loss on the same image (one image-sized streaming pass with an alpha
    read-modify-write: the yardstick for the bytes; `*_bytes` are the bytes each pass must move, whole lines of pred
    and v_pred counted for the stride-16 alpha accesses);
  * `iters` SplatTrainer steps on one synthetic scene (default S1: 1 M splats, 1080p, SH 3; no refinement): the plain
    separate-call step (fused_backward = False), the depth-supervised step, the step with the normal term, and the step
    with both; the plain fused step (the bench's path) for reference.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, which gives k_normal_loss / k_normal_loss_finalize /
k_splat_normals / k_splat_normals_backward and the two feature replays next to the step's other kernels (the event times
above include the launches).

    python tools/normal_loss_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/normal_loss_prof.py --iters 10

profiles/normal_loss_prof.json is the first form's output.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import normal_loss as NL  # noqa: E402
from brush_amd.depth_loss import depth_loss_into  # noqa: E402
from brush_amd.render import pack_uniforms  # noqa: E402
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
    npix = w * h
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    u = pack_uniforms(cam, (w, h), a.sh_degree, n)
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.rand((h, w, 4), generator=gen).to(dev)
    # a smooth surface under an alpha on either side of the threshold: about three pixels in four count
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    z = (5.0 + 1.5 * xs / w - 1.0 * ys / h + 0.05 * torch.sin(0.09 * xs) * torch.cos(0.07 * ys)).to(dev)
    pred[..., 3] = 0.35 + 0.65 * pred[..., 3]
    depth = (pred[..., 3] * z).contiguous()
    nimg = torch.randn((h, w, 3), generator=gen).to(dev) * 0.3
    nimg[..., 2] -= 1.0
    nimg = (nimg / nimg.norm(dim=2, keepdim=True) * pred[..., 3:4]).contiguous()
    t32 = (z * (0.9 + 0.2 * torch.rand((h, w), generator=gen).to(dev))).contiguous()
    gt = torch.rand((h, w, 3), generator=gen).to(dev)
    v_pred = torch.zeros_like(pred)
    ws = torch.empty(NL.workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    dn = torch.empty((h, w, 3), device=dev)
    accum = torch.zeros(1, device=dev)

    c = synthetic_cloud(n, a.sh_degree, seed=4)
    means, log_scales = (torch.from_numpy(c[k]).to(dev) for k in ("means", "log_scales"))
    quats = torch.from_numpy(c["quats"]).to(dev)
    quats = (quats / quats.norm(dim=1, keepdim=True)).contiguous()
    normals = torch.empty((n, 3), device=dev)
    v_normals = torch.randn((n, 3), generator=gen).to(dev)
    v_quats = torch.zeros((n, 4), device=dev)

    def normals_only():
        stats = torch.empty(2, device=dev)
        cfg = brush_amd._lib.BrushNormalLoss(0.0, 0.5)
        import ctypes as C
        brush_amd._lib.check(brush_amd._lib.lib().brush_normal_loss(
            C.byref(u), pred.data_ptr(), depth.data_ptr(), None, C.byref(cfg), dn.data_ptr(), None, None, None,
            stats.data_ptr(), None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "normals")

    abi = {
        "splat_normals": lambda: NL.splat_normals_from(u, means, log_scales, quats, out=normals),
        "splat_normals_backward": lambda: NL.splat_normals_backward_into(u, means, log_scales, quats, v_normals,
                                                                         v_quats),
        "normal_loss": lambda: NL.normal_loss_into(u, pred, depth, nimg, v_pred, weight=0.05, loss_accum=accum,
                                                   workspace=ws),
        "normals_only": normals_only,
        "depth_loss_f32": lambda: depth_loss_into(pred, depth, t32, v_pred, weight=0.1, loss_accum=accum),
    }
    res = {f"abi_{name}_ms": v for name, v in _timed(abi, a.iters).items()}
    _, _, stats = NL.normal_loss_into(u, pred, depth, nimg, None, weight=0.05)
    res.update(valid_fraction=float(stats[1]),
               normal_loss_bytes=(16 + 4 + 12 + 4 + 12 + 16 + 16) * npix, normals_only_bytes=(16 + 4 + 12) * npix,
               depth_loss_f32_bytes=60 * npix, splat_normals_bytes=(12 + 12 + 16 + 12) * n,
               splat_normals_backward_bytes=(12 + 12 + 16 + 12 + 16 + 16) * n)

    steps = {}
    for name, fused, target, nw in (("plain_fused", True, None, 0.0), ("plain_separate", False, None, 0.0),
                                    ("depth_f32", True, t32, 0.0), ("normal", True, None, 0.05),
                                    ("depth_f32_and_normal", True, t32, 0.05)):
        s = brush_amd.Splats(*(torch.from_numpy(c[key]).to(dev) for key in ("means", "sh", "quats", "raw_opac",
                                                                            "log_scales")))
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(max_refine_step=0, depth_weight=0.1, normal_weight=nw,
                                                             normal_from_step=0))
        tr.fused_backward = fused
        steps[name] = (lambda s=s, tr=tr, target=target: tr.step(s, cam, gt, gt_depth=target))
    res.update({f"train_step_{name}_ms": v for name, v in _timed(steps, a.iters).items()})
    line = {"splats": n, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters,
            "device": torch.cuda.get_device_name(dev), **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
