#!/usr/bin/env python3
"""Times brush_eval_metrics next to the training loss at one image size: `views` eval calls (u8 ground truth, as
eval_stats uploads it) and as many l1_ssim_loss calls (ssim_weight 0.2).  Meant to run under
`rocprofv3 --kernel-trace --stats`, which gives the per-kernel times (k_eval_metrics / k_eval_finalize next to
k_ssim_forward / k_ssim_backward); it also prints event-timed medians of its own.

    python tools/eval_prof.py [--width 1920] [--height 1080] [--views 8] [--window 11]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from brush_amd import eval_metrics  # noqa: E402
from brush_amd.train import l1_ssim_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--window", type=int, default=11)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    w, h = a.width, a.height
    preds = [torch.from_numpy(rng.random((h, w, 4), dtype=np.float32)).to(dev) for _ in range(a.views)]
    gts = [torch.from_numpy((rng.random((h, w, 3)) * 255).astype(np.uint8)).to(dev) for _ in range(a.views)]
    gts_f = [g.float() / 255.0 for g in gts]
    out = torch.empty((a.views, 3), device=dev)
    for i in range(a.views):  # warm-up (first launches, allocator)
        eval_metrics(preds[i], gts[i], a.window, out=out[i])
        l1_ssim_loss(preds[i], gts_f[i], 0.2, a.window)
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("eval_metrics", lambda i: eval_metrics(preds[i], gts[i], a.window, out=out[i])),
                     ("l1_ssim_loss", lambda i: l1_ssim_loss(preds[i], gts_f[i], 0.2, a.window))):
        ts = []
        for i in range(a.views):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name] = float(np.median(ts))
    print(f"{w}x{h} window {a.window}, {a.views} views: " +
          ", ".join(f"{k} median {v:.1f} us" for k, v in res.items()))


if __name__ == "__main__":
    main()
