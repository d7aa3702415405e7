#!/usr/bin/env python3
"""Times the per-splat error replay next to the forward it replays and the contribution replay it restates: `iters`
passes of one forward (float image), brush_l1_error_map against a seeded target, a same-size device copy,
brush_render_error_scores and brush_render_contributions on one synthetic scene, default S1 (1 M splats, 1080p, SH 3).
Meant to run under `rocprofv3 --kernel-trace --stats`, in a run of its own, which gives k_error_quad beside
k_contribution_quad and k_rasterize_quad, and k_l1_error_map beside the copy, from the same run; it also prints
event-timed medians of its own (forward alone, forward + map + replay, and `--views` such passes in a row: one score
pass of TrainConfig.densify_error_views).

    python tools/error_score_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20]
                                     [--views 32] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import render as R  # noqa: E402
from brush_amd.contribution import ContributionBuffers, contributions_from_aux  # noqa: E402
from brush_amd.error_score import ErrorScoreBuffers, error_scores_from_aux, l1_error_map  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--views", type=int, default=32, help="views of the timed score pass")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h = a.width, a.height
    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    means, log_scales, quats, sh, raw_opac = (torch.from_numpy(c[k]).to(dev) for k in
                                              ("means", "log_scales", "quats", "sh", "raw_opac"))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gt = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev,
                       generator=torch.Generator(device=dev).manual_seed(4))
    emap = torch.empty((h, w), dtype=torch.float32, device=dev)
    copy_dst = torch.empty_like(emap)
    bufs = ErrorScoreBuffers(a.splats, dev)
    cbufs = ContributionBuffers(a.splats, dev)

    def forward():
        with torch.no_grad():
            return R._forward_impl(cam, (w, h), means, log_scales, quats, sh, raw_opac, False, None,
                                   expect_backward=False)

    def view():
        img, aux, u = forward()
        l1_error_map(img, gt, out=emap)
        error_scores_from_aux(u, aux, emap, bufs)
        return img, aux, u

    def view_and_neighbours():
        img, aux, u = view()
        copy_dst.copy_(emap)  # the same-size copy k_l1_error_map is read against
        contributions_from_aux(u, aux, img, cbufs, check=False)

    def score_pass():
        for _ in range(a.views):
            view()

    def timed(fn, iters):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    res = {"forward_ms": timed(forward, a.iters), "forward_map_replay_ms": timed(view, a.iters)}
    timed(view_and_neighbours, a.iters)  # for the kernel trace: the copy and the contribution replay of the same run
    res["score_pass_ms"] = timed(score_pass, 3)
    one = ErrorScoreBuffers(a.splats, dev)
    img, aux, u = forward()
    error_scores_from_aux(u, aux, l1_error_map(img, gt), one)
    got = one.read()
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters, "views": a.views,
            **res, "map_replay_ms": res["forward_map_replay_ms"] - res["forward_ms"],
            "splats_with_error": int((got.views_seen > 0).sum()), "summed_error_px": float(got.sum.sum()),
            "largest_share_px": float(got.max.max())}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
