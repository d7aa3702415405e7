#!/usr/bin/env python3
"""Measures the device image pyramid (brush_amd/pyramid.py) and what a downscale schedule does to a training iteration.

  kernel   brush_area_resize_u8 at 1920x1080, RGB and RGBA, factors 2, 4, 8: `--calls` launches over as many distinct
           resident sources (more bytes than the chip's caches hold, so every call streams from HBM), captured into one
           graph and replayed, event-timed; beside it, in the same run, a device-to-device copy that moves the same
           bytes (read + written) over the same number of distinct buffers.  The ratio is kernel time / copy time.
  switch   SceneLoader.set_downscale(2) on `--views` resident 1080p RGB views (eager launches, event- and wall-timed).
  iter     TrainLoop.step on the shape of tools/train_loop_prof.py (1920x1080 RGB, 1 048 576 splats, SH 3, 8 views,
           refinement off): no schedule, and a constant factor of 1, 2 and 4, alternating round by round.
  psnr     (--psnr) one deterministic run with and one without a schedule on a 128x128 scene (16 training and 4 held-out
           renders of a known cloud): held-out PSNR / SSIM at the end, at equal steps.

    python tools/pyramid_prof.py [--calls 64] [--views 100] [--steps 20] [--rounds 7] [--psnr] [--only kernel,switch,iter]
                                 [--json profiles/pyramid_times.json]
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
from brush_amd import _lib  # noqa: E402
from brush_amd.dataset import Dataset, Scene, SceneView  # noqa: E402
from brush_amd.pyramid import downscaled_size  # noqa: E402
from brush_amd.scene_loader import SceneLoader  # noqa: E402
from brush_amd.train_loop import TrainLoop  # noqa: E402

W, H = 1920, 1080


def graph_ms(fn, reps=5):
    """Median milliseconds of one replay of `fn` captured into a graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def kernel_times(calls):
    dev = torch.device("cuda:0")
    l = _lib.lib()
    rows = []
    for channels in (3, 4):
        srcs = [torch.randint(0, 256, (H, W, channels), dtype=torch.uint8, device=dev) for _ in range(calls)]
        for factor in (2, 4, 8):
            ow, oh = downscaled_size(W, H, factor)
            read, written = W * H * channels, ow * oh * channels
            dsts = [torch.empty((oh, ow, channels), dtype=torch.uint8, device=dev) for _ in range(calls)]
            half = (read + written) // 2  # a copy of n bytes reads n and writes n
            copies = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(calls)]

            def resize():
                st = torch.cuda.current_stream().cuda_stream
                for s, d in zip(srcs, dsts):
                    _lib.check(l.brush_area_resize_u8(s.data_ptr(), W, H, channels, d.data_ptr(), ow, oh, st), "resize")

            def copy():
                for s, d in zip(srcs, copies):
                    d.copy_(s.view(-1)[:half])

            k_ms, c_ms = graph_ms(resize) / calls, graph_ms(copy) / calls
            rows.append({"channels": channels, "factor": factor, "out": [ow, oh], "bytes_read": read,
                         "bytes_written": written, "kernel_us": k_ms * 1e3, "copy_us": c_ms * 1e3,
                         "kernel_over_copy": k_ms / c_ms, "kernel_GBps": (read + written) / (k_ms * 1e6),
                         "copy_GBps": 2 * half / (c_ms * 1e6)})
            print(f"area_resize {W}x{H}x{channels} / {factor}: {k_ms * 1e3:8.2f} us   copy of the same bytes "
                  f"{c_ms * 1e3:8.2f} us   ratio {k_ms / c_ms:.2f}")
            del dsts, copies
        del srcs
    return rows


def switch_times(views, rounds=5):
    dev = torch.device("cuda:0")
    img = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 1.0, 0.6, (0.5, 0.5))
    loader = SceneLoader(Scene([SceneView(f"v{k}", cam, img) for k in range(views)]), 0, dev)
    ev, wall = [], []
    for r in range(rounds + 1):  # round 0 warms up
        loader.set_downscale(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        loader.set_downscale(2)
        e1.record()
        issued = time.perf_counter() - t0
        e1.synchronize()
        if r > 0:
            ev.append(e0.elapsed_time(e1)), wall.append(issued * 1e3)
    res = {"views": views, "factor": 2, "resident_bytes": loader.total_bytes, "level_bytes": loader.level_bytes,
           "device_ms": float(np.median(ev)), "host_issue_ms": float(np.median(wall))}
    print(f"set_downscale(2) on {views} 1080p RGB views: {res['device_ms']:.3f} ms on the device, "
          f"{res['host_issue_ms']:.3f} ms to issue")
    return res


def iteration_times(steps, rounds, views=8):
    from brush_amd.synthetic import synthetic_cloud

    dev = torch.device("cuda:0")
    n, deg = 1 << 20, 3
    cloud = synthetic_cloud(n, deg, seed=4)
    focal = brush_amd.fov_to_focal(math.pi * 0.5, W)

    def camera(k):
        ang = 0.35 * k
        return brush_amd.Camera([-8.0 * math.sin(ang), 0.0, -8.0 * math.cos(ang)],
                                [0.0, math.sin(ang / 2), 0.0, math.cos(ang / 2)], brush_amd.focal_to_fov(focal, W),
                                brush_amd.focal_to_fov(focal, H), (0.5, 0.5))

    rng = np.random.default_rng(2)
    data = Dataset(Scene([SceneView(f"v{k}", camera(k), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
                          for k in range(views)]))
    total = (rounds + 1) * steps

    def loop(schedule):
        p = {k: torch.from_numpy(v).to(dev) for k, v in cloud.items()}
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, downscale_schedule=schedule)
        return TrainLoop(data, cfg, steps=total, seed=3,
                         init=brush_amd.Splats(p["means"], p["sh"], p["quats"], p["raw_opac"], p["log_scales"]))

    loops = {"no_schedule": loop(()), "factor_1": loop(((0, 1),)), "factor_2": loop(((0, 2),)),
             "factor_4": loop(((0, 4),))}
    times = {k: [] for k in loops}
    for r in range(rounds + 1):  # round 0 warms up (and takes the level switch)
        for k in (list(loops) if r % 2 == 0 else list(loops)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loops[k].step()
            torch.cuda.synchronize()
            if r > 0:
                times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {"shape": f"{W}x{H} RGB, {n} splats, SH {deg}, {views} views", "steps_per_round": steps, "rounds": rounds,
           "variants": {}}
    for k, ts in times.items():
        _, log = loops[k].finish()
        assert np.isfinite(log.losses).all()
        res["variants"][k] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)),
                              "max_ms": float(np.max(ts)), "rounds_ms": [round(t, 4) for t in ts]}
        print(f"{k:12s} median {np.median(ts):.4f} ms/step  (min {np.min(ts):.4f}, max {np.max(ts):.4f}, "
              f"{len(ts)} rounds of {steps})")
    return res


def ring_dataset(dev, w=128, h=128, n_train=16, n_eval=4):
    """Renders of a known cloud (3000 splats in a box around the origin) from two rings of cameras, as u8 views."""
    from brush_amd.dataset import nerf_camera

    known = brush_amd.Splats.from_random_config(3000, 0, (np.full(3, -0.8), np.full(3, 0.8)), np.random.default_rng(11),
                                                dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.06))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))

    def views(n, offset):
        out = []
        for i in range(n):
            ang = 2.0 * math.pi * i / n + offset
            eye = np.array([4.0 * math.cos(ang), 4.0 * math.sin(ang), 1.0])
            z = eye / np.linalg.norm(eye)  # an OpenGL camera looks down -z, at the origin
            x = np.cross([0.0, 0.0, 1.0], z)
            x /= np.linalg.norm(x)
            c2w = np.eye(4)
            c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, eye
            cam = nerf_camera(c2w, 0.6911112070083618, w, h)
            with torch.no_grad():
                pred, _ = known.render(cam, (w, h), False)
            img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            out.append(SceneView(f"r_{i}", cam, img))
        return out

    return Dataset(Scene(views(n_train, 0.1)), Scene(views(n_eval, 0.5)))


def psnr_runs(steps=600):
    """One run with and one without a schedule on ring_dataset, deterministic, equal steps."""
    from brush_amd import render as R
    from brush_amd.train_loop import train_scene

    dev = torch.device("cuda:0")
    R.DETERMINISTIC = True
    res = {"steps": steps, "scene": "ring_dataset: 128x128, 16 training and 4 eval views of a known 3000-splat cloud"}
    data = ring_dataset(dev)
    for name, schedule in (("no_schedule", ()), ("schedule", ((0, 4), (steps // 4, 2), (steps // 2, 1)))):
        cfg = brush_amd.TrainConfig(warmup_steps=50, refine_every=50, downscale_schedule=schedule)
        splats, log = train_scene(data, cfg, steps=steps, init_count=2000, sh_degree=3, seed=5, eval_every=steps)
        res[name] = {"downscale_schedule": [list(p) for p in schedule], "psnr": log.evals[-1].psnr,
                     "ssim": log.evals[-1].ssim, "splats": log.num_splats, "train_seconds": log.train_seconds}
        print(f"{name:12s} {steps} steps: psnr {log.evals[-1].psnr:.3f} ssim {log.evals[-1].ssim:.4f} "
              f"splats {log.num_splats} in {log.train_seconds:.2f} s")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=64, help="distinct 1080p sources per timed graph")
    ap.add_argument("--views", type=int, default=100, help="resident views of the level switch")
    ap.add_argument("--steps", type=int, default=20, help="steps per variant per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="kernel,switch,iter")
    ap.add_argument("--psnr", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    only = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in only:
        res["area_resize"] = kernel_times(a.calls)
    if "switch" in only:
        res["level_switch"] = switch_times(a.views)
    if "iter" in only:
        res["iteration"] = iteration_times(a.steps, a.rounds)
    if a.psnr:
        res["psnr_at_equal_steps"] = psnr_runs()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
