#!/usr/bin/env python3
"""Times the feature replays next to the forward they replay: on one synthetic scene, default S1 (1 M splats, 1080p,
SH 3), one finished forward and, at C = 1, 3, 4, 16, 17 and 64, event-timed medians of brush_render_features (the
forward replay), brush_render_features_backward (the float transpose) and brush_render_feature_sums (the exact
transpose, f32 maps; at C = 16 the label kind too), beside the plain forward (all of it, and
its stages: the compositing stage is what the replays restate) and C separate brush_render_error_scores calls on the same forward: the only way to the exact sums without this
kernel.  Prints one JSON line; `--json OUT` also writes it.

    python tools/features_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 10]
                                  [--channels 1,3,4,16,17,64] [--json OUT]
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
from brush_amd import render as R  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd.features import feature_grads_from_aux, feature_sums_from_aux, features_from_aux  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--channels", default="1,3,4,16,17,64")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h, n = a.width, a.height, a.splats
    c = synthetic_cloud(n, a.sh_degree, seed=4)
    means, log_scales, quats, sh, raw_opac = (torch.from_numpy(c[k]).to(dev) for k in
                                              ("means", "log_scales", "quats", "sh", "raw_opac"))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))
    gen = torch.Generator(device=dev).manual_seed(4)

    def forward():
        with torch.no_grad():
            return R._forward_impl(cam, (w, h), means, log_scales, quats, sh, raw_opac, False, None,
                                   expect_backward=False)

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

    res = {"forward_ms": timed(forward, a.iters)}
    from brush_amd.profiler import StageProfiler

    with StageProfiler() as prof:  # the forward's own stages: the compositing kernel is the one the replays restate
        _, aux, u = forward()
        res["forward_stages_ms"] = {k: v for k, v in prof.read_ms().items() if v > 0.0}
    view_err = torch.zeros(n, dtype=torch.int64, device=dev)
    emap = torch.rand((h, w), dtype=torch.float32, device=dev, generator=gen)
    st = aux._as_struct()

    def error_scores():  # the bare entry, without error_score.py's fold
        _lib.check(_lib.lib().brush_render_error_scores(C.byref(u), C.byref(st), emap.data_ptr(), view_err.data_ptr(), n,
                                                        _lib.current_stream(dev)), "brush_render_error_scores")

    res["error_scores_ms"] = timed(error_scores, a.iters)
    rows = []
    for ch in (int(x) for x in a.channels.split(",")):
        feats = torch.rand((n, ch), dtype=torch.float32, device=dev, generator=gen)
        maps = torch.rand((h, w, ch), dtype=torch.float32, device=dev, generator=gen)
        out = torch.empty((h, w, ch), dtype=torch.float32, device=dev)
        v_f = torch.zeros((n, ch), dtype=torch.float32, device=dev)
        sums = torch.zeros((n, ch), dtype=torch.int64, device=dev)

        def error_calls():
            for _ in range(ch):
                error_scores()

        row = {"C": ch,
               "features_ms": timed(lambda: features_from_aux(u, aux, feats, out=out), a.iters),
               "grad_f32_ms": timed(lambda: feature_grads_from_aux(u, aux, maps, v_f), a.iters),
               "sums_q24_ms": timed(lambda: feature_sums_from_aux(u, aux, maps, sums), a.iters),
               "error_scores_x_C_ms": timed(error_calls, max(2, a.iters // 4))}
        if ch == 16:
            labels = torch.randint(0, ch, (h, w), dtype=torch.uint8, device=dev, generator=gen)
            row["sums_label_ms"] = timed(lambda: feature_sums_from_aux(u, aux, labels, sums), a.iters)
        rows.append(row)
        del feats, maps, out, v_f, sums
    line = {"splats": n, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters, **res, "channels": rows}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
