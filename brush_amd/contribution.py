"""Rendered contribution of every splat over a set of views, and pruning by it (build extension; RadSplat's max
blending weight and LightGaussian's summed weight are the models).

For each view one forward and one replay of its compositing walk (include/brush_hip.h: brush_render_contributions,
csrc/contribution.hip) accumulate four order-independent integers per splat into device buffers that stay across the
views: the bits of the largest weight fac = alpha T the splat was added with, the sum of rint(fac 2^24), the number of
pixels it was added to (hits) and the number of pixels it ended without being added (stops, the forward's stop quirk:
rasterize.wgsl:88-91).  A splat with hits == 0 and stops == 0 in every view can be removed without changing one bit of
any of those views.

    c = splat_contributions(splats, scene.views)          # one read-back, at the end
    pruned = splats.select(~prune_mask(c, min_max=0.01))   # RadSplat's rule

Command line: `python -m brush_amd.prune` (brush_amd/prune.py).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

Q24 = float(1 << 24)  # the fixed point of the summed weight (brush_render_contributions: sum_q24)


@dataclass
class Contributions:
    """Per-splat statistics over `views` views, as CPU tensors of N rows.
    max: float32, the largest fac = alpha T over all pixels of all views (0 where the splat was never added).
    sum: float64, sum_q24 / 2^24: the summed fac, each added pixel rounded to a unit of 2^-24.
    hits / stops: int64, pixels the splat was added to / ended without being added."""
    max: torch.Tensor
    sum: torch.Tensor
    hits: torch.Tensor
    stops: torch.Tensor
    views: int = 0

    def accumulate(self, other: "Contributions") -> "Contributions":
        """The statistics over both sets of views: elementwise max of `max`, sums of the rest.  A new object."""
        if other.max.shape != self.max.shape:
            raise ValueError(f"cannot accumulate contributions of {other.max.shape[0]} splats into "
                             f"{self.max.shape[0]}")
        return Contributions(torch.maximum(self.max, other.max), self.sum + other.sum, self.hits + other.hits,
                             self.stops + other.stops, self.views + other.views)


class ContributionBuffers:
    """The device side of a Contributions in the making: max_bits [N] i32, counts [N,3] i64 (sum_q24, hits, stops) and
    mismatch [1] i32, zeroed once here; brush_render_contributions only accumulates."""

    def __init__(self, n: int, device):
        self.n = int(n)
        self.max_bits = torch.zeros(max(self.n, 1), dtype=torch.int32, device=device)
        self.counts = torch.zeros((max(self.n, 1), 3), dtype=torch.int64, device=device)
        self.mismatch = torch.zeros(1, dtype=torch.int32, device=device)
        self.views = 0

    def read(self):
        """(Contributions, accumulated mismatch count): the one read-back (synchronises)."""
        counts = self.counts[:self.n].cpu()
        mx = self.max_bits[:self.n].cpu().view(torch.float32)
        bad = int(self.mismatch.cpu().item())
        return Contributions(mx, counts[:, 0].to(torch.float64) / Q24, counts[:, 1].clone(), counts[:, 2].clone(),
                             self.views), bad


def contributions_from_aux(uniforms, aux, img: Optional[torch.Tensor], out: ContributionBuffers, check: bool = True):
    """The bare call: replays the finished forward (`uniforms`, `aux`: what render._forward_impl returned, or
    render.pack_uniforms of the same camera and size beside a render's RenderAux) and accumulates into `out`.
    `img`: that forward's float image [h,w,4]; needed with `check`, which makes every pixel compare its replayed alpha
    and last entry with the forward's and counts the differences in out.mismatch.  Runs on the current stream; does
    not synchronise."""
    dev = out.max_bits.device
    assert dev.type == "cuda", "brush_amd has no CPU path: the buffers must live on the GPU"
    if check:
        if img is None:
            raise ValueError("check=True needs the forward's image")
        h, w = int(uniforms.img_size[1]), int(uniforms.img_size[0])
        if tuple(img.shape) != (h, w, 4) or img.dtype != torch.float32 or not img.is_contiguous():
            raise ValueError(f"img must be the forward's contiguous float32 [{h},{w},4] image, got {img.dtype} "
                             f"{tuple(img.shape)}")
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_contributions(
            C.byref(uniforms), C.byref(s), img.data_ptr() if check else None, out.max_bits.data_ptr(),
            out.counts.data_ptr(), out.mismatch.data_ptr() if check else None, out.n, _lib.current_stream(dev)),
            "brush_render_contributions")
    out.views += 1
    return out


def splat_contributions(splats, views, *, antialiased: bool = False, downscale: int = 1,
                        check: bool = True) -> Contributions:
    """The contributions of `splats` over `views`, each a dataset.SceneView (rendered at its image's size) or a
    (Camera, (w, h)) pair: per view one forward and one replay into the same device buffers, one read-back after the
    last view.  `antialiased`: render in that mode; `downscale` = f > 1: at pyramid.downscaled_size of each size.
    `check`: the replay's self-check; a RuntimeError if any pixel of any view differs from its forward."""
    from . import render as R
    from .pyramid import check_factor

    downscale = check_factor(downscale)
    parts = splats.frozen()  # one sync, as Splats.render does per call
    bufs = ContributionBuffers(splats.num_splats(), parts[0].device)
    with torch.no_grad():
        for v in views:
            cam, size, _, _ = R.view_parts(v, downscale=downscale)
            img, aux, u = R.forward_frozen(parts, cam, size, antialiased)
            contributions_from_aux(u, aux, img, bufs, check)
    c, bad = bufs.read()
    if check and bad != 0:
        raise RuntimeError(f"brush_render_contributions: {bad} pixels of the replay differ from their forward")
    return c


def prune_mask(c: Contributions, *, min_max: Optional[float] = None, keep_fraction: Optional[float] = None,
               by: str = "max") -> torch.Tensor:
    """A boolean [N] tensor, True where a splat is PRUNED.  Exactly one rule:
    min_max = 0.0: the exact rule, hits == 0 and stops == 0 (removing these changes no bit of the views);
    min_max = t > 0: max < t (RadSplat: t = 0.01);
    keep_fraction = f in [0, 1]: keep the ceil(f N) largest by `by` ("max" or "sum"), ties broken by lower index.
    Pure torch; works on CPU tensors."""
    if (min_max is None) == (keep_fraction is None):
        raise ValueError("give exactly one of min_max and keep_fraction")
    if by not in ("max", "sum"):
        raise ValueError(f"by must be 'max' or 'sum', got {by!r}")
    n = int(c.max.shape[0])
    if min_max is not None:
        t = float(min_max)
        if not (0.0 <= t <= 1.0):  # (a NaN fails too)
            raise ValueError(f"min_max must be in [0, 1], got {min_max!r}")
        if t == 0.0:
            return (c.hits == 0) & (c.stops == 0)
        return c.max < t
    f = float(keep_fraction)
    if not (0.0 <= f <= 1.0):
        raise ValueError(f"keep_fraction must be in [0, 1], got {keep_fraction!r}")
    k = min(n, int(math.ceil(f * n)))
    key = (c.max if by == "max" else c.sum).to(torch.float64)
    order = torch.sort(key, descending=True, stable=True).indices  # stable: among equals the lower index comes first
    mask = torch.ones(n, dtype=torch.bool, device=key.device)
    mask[order[:k]] = False
    return mask


def max_histogram(c: Contributions, decades: int = 8) -> dict:
    """Counts of `max` in decades: {"0": never added, "<1e-7": ..., "[1e-7,1e-6)": ..., ..., "[1e-1,1]": ...}."""
    mx = c.max.to(torch.float64)
    out = {"0": int((mx == 0).sum())}
    lo = 10.0 ** -(decades - 1)
    out[f"<1e-{decades - 1}"] = int(((mx > 0) & (mx < lo)).sum())
    for d in range(decades - 1, 0, -1):
        a, b = 10.0 ** -d, 10.0 ** -(d - 1)
        last = d == 1
        sel = (mx >= a) & ((mx <= b) if last else (mx < b))
        out[f"[1e-{d},{'1]' if last else f'1e-{d - 1})'}"] = int(sel.sum())
    return out
