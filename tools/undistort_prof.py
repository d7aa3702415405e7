#!/usr/bin/env python3
"""Measures the undistortion kernels (brush_amd/undistort.py, brush_amd/csrc/undistort.hip).

  kernel   brush_undistort_u8 at 1920x1080, RGB and RGBA, a mild and a strong OPENCV warp at its fitted scale, with and
           without the validity mask; brush_undistort_nearest on uint16 and float32 depth maps of the same size.
           `--calls` launches over as many distinct resident sources (more bytes than the chip's caches hold, so every
           call streams from HBM), captured into one graph and replayed, event-timed; beside it, in the same run and
           alternating with it round by round, a device-to-device copy that moves the same bytes (source read +
           destination written) over the same number of distinct buffers.  Every figure is the median over `--rounds`
           rounds, with the minimum and maximum beside it: the run-to-run spread a difference has to exceed.
  load     undistort_dataset on `--views` 1080p RGB views sharing one camera: wall time per view of the whole round
           trip (upload, kernel, copy back), the load-time cost a user pays once.

    python tools/undistort_prof.py [--calls 64] [--rounds 7] [--views 16] [--only kernel,load]
                                   [--json profiles/undistort_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd.dataset import Dataset, Scene, SceneView  # noqa: E402
from brush_amd.undistort import Distortion, fit_scale, undistort_dataset, undistort_map  # noqa: E402

W, H = 1920, 1080
WARPS = {
    "mild": Distortion("OPENCV", W, H, 1400.0, 1410.0, 951.0, 547.0, k1=-0.05, k2=0.01, p1=1e-3, p2=-1e-3),
    "strong": Distortion("OPENCV", W, H, 1400.0, 1410.0, 951.0, 547.0, k1=-0.3, k2=0.08, p1=0.02, p2=-0.015),
}


def capture(fn):
    """`fn` warmed up on a side stream, then captured into a graph."""
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
    return g


def replay_ms(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(graphs, rounds):
    """{name: [ms per round]}: the graphs replayed in turn, the order reversed every other round; round 0 warms up."""
    times = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for k in (list(graphs) if r % 2 == 0 else list(graphs)[::-1]):
            t = replay_ms(graphs[k])
            if r > 0:
                times[k].append(t)
    return times


def stats(ts, calls):
    us = np.asarray(ts) * 1e3 / calls
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max())}


def kernel_times(calls, rounds):
    dev = torch.device("cuda:0")
    l = _lib.lib()
    rows = []
    for what in ("rgb", "rgba", "u16", "f32"):
        if what in ("rgb", "rgba"):
            channels = 3 if what == "rgb" else 4
            srcs = [torch.randint(0, 256, (H, W, channels), dtype=torch.uint8, device=dev) for _ in range(calls)]
            px_bytes = channels
        else:
            dtype = torch.uint16 if what == "u16" else torch.float32
            px_bytes = 2 if what == "u16" else 4
            srcs = [torch.randint(0, 60000, (H, W), device=dev).to(dtype) for _ in range(calls)]
        dsts = [torch.empty_like(s) for s in srcs]
        masks = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(calls)]
        copies = [torch.empty(W * H * px_bytes, dtype=torch.uint8, device=dev) for _ in range(calls)]
        flat = [s.view(-1).view(torch.uint8) for s in srcs]

        def copy():
            for s, d in zip(flat, copies):
                d.copy_(s)

        graphs = {"copy": capture(copy)}
        for wname, d in WARPS.items():
            m = undistort_map(d, fit_scale(d))
            for with_mask in ((False, True) if what in ("rgb", "rgba") else (False,)):

                def run(m=m, with_mask=with_mask):
                    st = torch.cuda.current_stream().cuda_stream
                    for i in range(calls):
                        if what in ("rgb", "rgba"):
                            _lib.check(l.brush_undistort_u8(srcs[i].data_ptr(), W, H, px_bytes, dsts[i].data_ptr(), W, H,
                                                            masks[i].data_ptr() if with_mask else None, m, st), "u8")
                        else:
                            _lib.check(l.brush_undistort_nearest(srcs[i].data_ptr(), px_bytes, W, H, dsts[i].data_ptr(),
                                                                 W, H, m, st), "nearest")

                graphs[wname + ("+mask" if with_mask else "")] = capture(run)
        times = alternate(graphs, rounds)
        copy_stats = stats(times["copy"], calls)
        for k, ts in times.items():
            if k == "copy":
                continue
            row = {"what": what, "warp": k, "scale": fit_scale(WARPS[k.split("+")[0]]), "bytes_read": W * H * px_bytes,
                   "bytes_written": W * H * (px_bytes + (1 if k.endswith("+mask") else 0)), "kernel": stats(ts, calls),
                   "copy": copy_stats}
            row["kernel_over_copy"] = row["kernel"]["median_us"] / copy_stats["median_us"]
            row["kernel_GBps"] = (row["bytes_read"] + row["bytes_written"]) / (row["kernel"]["median_us"] * 1e3)
            rows.append(row)
            kst = row["kernel"]
            print(f"{what:4s} {k:12s} {kst['median_us']:8.2f} us (min {kst['min_us']:.2f}, max {kst['max_us']:.2f})   "
                  f"copy of the image's bytes {copy_stats['median_us']:7.2f} us (min {copy_stats['min_us']:.2f}, max "
                  f"{copy_stats['max_us']:.2f})   ratio {row['kernel_over_copy']:.2f}   {row['kernel_GBps']:.0f} GB/s")
        del srcs, dsts, masks, copies, flat, graphs
    return rows


def load_times(views):
    dev = torch.device("cuda:0")
    d = WARPS["mild"]
    rng = np.random.default_rng(0)
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 1.2, 0.75, (d.cx / W, d.cy / H))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    data = Dataset(Scene([SceneView(f"v{k}", cam, img, distortion=d) for k in range(views)]))
    undistort_dataset(Dataset(Scene(data.train.views[:1])), dev)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    undistort_dataset(data, dev)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / views
    print(f"undistort_dataset on {views} 1080p RGB views: {ms:.2f} ms per view (upload, kernel, copy back)")
    return {"views": views, "ms_per_view": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=64, help="distinct 1080p sources per timed graph")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--only", default="kernel,load")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    only = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    if "kernel" in only:
        res["kernels"] = kernel_times(a.calls, a.rounds)
    if "load" in only:
        res["load"] = load_times(a.views)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
