#!/usr/bin/env python3
"""Times the contribution replay next to the forward it replays: `iters` passes of one forward (float image) followed by
brush_render_contributions on one synthetic scene, default S1 (1 M splats, 1080p, SH 3).  Meant to run under
`rocprofv3 --kernel-trace --stats`, in a run of its own, which gives k_contribution_quad against k_rasterize_quad of the
same run; it also prints event-timed medians of its own (forward alone, forward + replay) and what the replay found
(splats added somewhere, splats that only stopped pixels, splats under RadSplat's 0.01).

    python tools/contrib_prof.py [--splats 1048576] [--width 1920] [--height 1080] [--sh-degree 3] [--iters 20]
                                 [--check] [--json OUT]
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
from brush_amd.contribution import ContributionBuffers, contributions_from_aux, prune_mask  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check", action="store_true", help="run the replay's self-check too (reads the image back)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w, h = a.width, a.height
    c = synthetic_cloud(a.splats, a.sh_degree, seed=4)
    means, log_scales, quats, sh, raw_opac = (torch.from_numpy(c[k]).to(dev) for k in
                                              ("means", "log_scales", "quats", "sh", "raw_opac"))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 2 * np.arctan(0.5 * w / (0.5 * w)),
                           2 * np.arctan(0.5 * h / (0.5 * w)), (0.5, 0.5))

    def forward():
        with torch.no_grad():
            return R._forward_impl(cam, (w, h), means, log_scales, quats, sh, raw_opac, False, None,
                                   expect_backward=False)

    def both(bufs):
        img, aux, u = forward()
        contributions_from_aux(u, aux, img, bufs, check=a.check)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    scratch = ContributionBuffers(a.splats, dev)
    res = {"forward_ms": timed(forward), "forward_replay_ms": timed(lambda: both(scratch))}
    one = ContributionBuffers(a.splats, dev)  # one view, for the figures
    both(one)
    con, bad = one.read()
    line = {"splats": a.splats, "width": w, "height": h, "sh_degree": a.sh_degree, "iters": a.iters, **res,
            "replay_ms": res["forward_replay_ms"] - res["forward_ms"], "check": bool(a.check), "mismatch": bad,
            "splats_added": int((con.hits > 0).sum()), "splats_only_stopping": int(((con.hits == 0) & (con.stops > 0)).sum()),
            "splats_untouched": int(prune_mask(con, min_max=0.0).sum()),
            "splats_max_below_0.01": int(prune_mask(con, min_max=0.01).sum()),
            "hits": int(con.hits.sum()), "stops": int(con.stops.sum())}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
