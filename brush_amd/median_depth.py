"""Median depth and the splat under every pixel (build extension; the depth 2DGS, GOF, RaDe-GS and gsplat's 2DGS path
fuse into their meshes).

The median depth of a pixel is the camera-space z of the splat at which the accumulated opacity first reaches `level`
(one half): the first entry the forward added after which the transmittance is at or below 1 - level.  Unlike the
expected depth D / alpha it never lies between a foreground and the background behind it, so a fused volume grows no
skirts at silhouettes.  One forward with the depth output and one replay of its compositing walk
(include/brush_hip.h: brush_render_median_depth, csrc/median_depth.hip) produce it, together with the global id of that
splat ("which splat is under this pixel").

    img, depth, median, ids, aux = splats.render_median_depth(camera, (w, h))

NOT DIFFERENTIABLE: the median is a pick, not a blend.  Everything here runs under no_grad and the results carry no
autograd history; supervise depth through render_splats_depth.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib


def check_level(level) -> float:
    """`level` as a float, or a ValueError: the accumulated opacity at which a pixel's depth is taken, 0 < level < 1."""
    try:
        x = float(level)
    except (TypeError, ValueError):
        x = math.nan
    if not (math.isfinite(x) and 0.0 < x < 1.0):
        raise ValueError(f"level must be finite with 0 < level < 1, got {level!r}")
    return x


def median_depth_from_aux(uniforms, aux, compact_depth: torch.Tensor, *, level: float = 0.5, want_ids: bool = True,
                          out: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None):
    """The bare call: replays the finished depth forward (`uniforms`, `aux`: what render._forward_impl returned;
    `compact_depth`: the float32 [N] buffer it filled with every visible splat's z) and returns (median [h,w] f32,
    ids [h,w] i32 or None).  `out`: (median, ids) tensors to write into instead of fresh ones (ids None without
    want_ids).  Every pixel is written.  Runs on the current stream; does not synchronise.  Not differentiable."""
    level = check_level(level)
    dev = compact_depth.device
    assert dev.type == "cuda", "brush_amd has no CPU path: the buffers must live on the GPU"
    h, w = int(uniforms.img_size[1]), int(uniforms.img_size[0])
    n = int(uniforms.total_splats)
    if compact_depth.dtype != torch.float32 or compact_depth.dim() != 1 or compact_depth.shape[0] < max(n, 1) \
            or not compact_depth.is_contiguous():
        raise ValueError(f"compact_depth must be the forward's contiguous float32 [{max(n, 1)}] buffer, got "
                         f"{compact_depth.dtype} {tuple(compact_depth.shape)}")
    if out is None:
        median = torch.empty((h, w), dtype=torch.float32, device=dev)
        ids = torch.empty((h, w), dtype=torch.int32, device=dev) if want_ids else None
    else:
        median, ids = out[0], (out[1] if want_ids else None)
        for t, dtype, what in ((median, torch.float32, "median"),) + (((ids, torch.int32, "ids"),) if want_ids else ()):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (h, w) or t.dtype != dtype or t.device != dev \
                    or not t.is_contiguous():
                raise ValueError(f"out: {what} must be a contiguous {dtype} [{h},{w}] tensor on {dev}")
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_median_depth(
            C.byref(uniforms), C.byref(s), compact_depth.data_ptr(), level, median.data_ptr(),
            None if ids is None else ids.data_ptr(), n, _lib.current_stream(dev)), "brush_render_median_depth")
    return median, ids


def render_median_depth(camera, img_size, means, log_scales, quats, sh_coeffs, raw_opacity, *, level: float = 0.5,
                        antialiased: bool = False, max_intersects: Optional[int] = None):
    """One brush_render_forward_depth plus the replay, under no_grad: (img [h,w,4], depth [h,w], median [h,w],
    ids [h,w] i32, aux).  img, depth and aux are bitwise those of render.render_splats_depth of the same arguments
    (depth: the ACCUMULATED depth D); median: the z of the splat at which the accumulated opacity first reaches `level`,
    0 where it never does; ids: that splat's global id, -1 where there is none.  `quats` must be unit quaternions, as
    for render_splats.  Not differentiable: no result carries autograd history."""
    from . import render as R

    level = check_level(level)
    R._check_inputs(means, None, log_scales, quats, sh_coeffs, raw_opacity)
    with torch.no_grad():
        bufs = R._depth_buffers(means.shape[0], img_size, means.device)
        img, aux, u = R._forward_impl(camera, img_size, means.detach(), log_scales.detach(), quats.detach(),
                                      sh_coeffs.detach(), raw_opacity.detach(), False, max_intersects,
                                      expect_backward=False, depth=bufs, antialiased=antialiased)
        median, ids = median_depth_from_aux(u, aux, bufs[1], level=level)
    return img, bufs[0], median, ids, aux
