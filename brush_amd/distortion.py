"""The depth-distortion term of surface splatting (build extension; 2DGS, GOF, RaDe-GS and gsplat's 2DGS path are the
models), with gradients into the geometry.

Per pixel, over the entries the forward added (blending weights w_i = alpha_i T_i, z_i the camera-space depth of splat
i's mean),

    L(p) = sum over unordered pairs of w_i w_j (m_i - m_j)^2,    m = z ("depth") or far / (far - near) (1 - near / z) ("ndc")

It pulls the splats a ray crosses onto one surface: what removes floaters and "thick" surfaces before TSDF fusion.  A
replay of a finished depth forward gives the per-pixel totals (include/brush_hip.h: brush_render_distortion), a second
replay adds the term's per-record VJP into the compact gradient rows of the render backward
(brush_distortion_compact_grads, brush_render_backward_distortion), and the unchanged parameter backward carries it to
means, scales, rotations and opacities.  Unlike the normal-consistency term, NOTHING IS FROZEN here: the gradient goes
through the blending weights too.

    img, depth, dist, aux = splats.render_distortion(camera, (w, h))       # all three differentiable
    loss = colour_loss(img) + 100.0 * dist.mean()

The gradient replay accumulates with float atomics: order dependent in its last bits.  Deterministic mode keeps one
gradient row per intersection and has no place for the term: every gradient form here raises ValueError in it.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from . import render as R
from .render import check_tensor

MODES = {"depth": _lib.DISTORTION_DEPTH, "ndc": _lib.DISTORTION_NDC}
DEFAULT_NEAR = 0.2
COMPACT_STRIDE = 16  # floats per compact gradient row (csrc/common.hpp: kCompactStride)


def distortion_config(mode: str = "depth", near: float = DEFAULT_NEAR, far: Optional[float] = None) -> _lib.BrushDistortion:
    """The BrushDistortion of (`mode`, `near`, `far`), or a ValueError: mode "depth" or "ndc"; "ndc" needs finite
    0 < near < far (`far` is required there; "depth" reads neither)."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'depth' or 'ndc', got {mode!r}")
    if mode == "depth":
        return _lib.BrushDistortion(MODES[mode], 0.0, 0.0)
    if far is None:
        raise ValueError("mode 'ndc' needs far (the far plane of the depth mapping)")
    try:
        nz, fz = float(near), float(far)
    except (TypeError, ValueError):
        nz = fz = math.nan
    if not (math.isfinite(nz) and math.isfinite(fz) and 0.0 < nz < fz):
        raise ValueError(f"mode 'ndc' needs finite 0 < near < far, got near={near!r}, far={far!r}")
    return _lib.BrushDistortion(MODES[mode], nz, fz)


def _frame(uniforms, compact_depth):
    dev = compact_depth.device
    assert dev.type == "cuda", "brush_amd has no CPU path: the buffers must live on the GPU"
    h, w, n = int(uniforms.img_size[1]), int(uniforms.img_size[0]), int(uniforms.total_splats)
    if compact_depth.dtype != torch.float32 or compact_depth.dim() != 1 or compact_depth.shape[0] < max(n, 1) \
            or not compact_depth.is_contiguous():
        raise ValueError(f"compact_depth must be the forward's contiguous float32 [{max(n, 1)}] buffer, got "
                         f"{compact_depth.dtype} {tuple(compact_depth.shape)}")
    return h, w, n, dev


def _refuse_deterministic(aux):
    if aux.deterministic:
        raise ValueError("the distortion term has no deterministic mode: that mode keeps one gradient row per "
                         "intersection, the term adds into per-splat rows (render with deterministic=False)")


def distortion_from_aux(uniforms, aux, compact_depth: torch.Tensor, cfg: Optional[_lib.BrushDistortion] = None, *,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bare forward replay (brush_render_distortion) of a finished depth forward (`uniforms`, `aux`: what
    render._forward_impl returned; `compact_depth`: the float32 [N] buffer it filled): stats [h,w,4] float32 =
    (L, W, M1, M2) per pixel, L in channel 0.  `cfg`: distortion_config(...) (default: "depth").  `out`: a tensor to
    write into.  Every pixel is written; bitwise repeatable; current stream, no synchronisation, no autograd."""
    h, w, n, dev = _frame(uniforms, compact_depth)
    cfg = distortion_config() if cfg is None else cfg
    if out is None:
        out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    else:
        check_tensor(out, torch.float32, (h, w, 4), "out", dev)
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_distortion(C.byref(uniforms), C.byref(s), compact_depth.data_ptr(),
                                                      C.byref(cfg), n, out.data_ptr(), _lib.current_stream(dev)),
                   "brush_render_distortion")
    return out


def distortion_compact_grads_from_aux(uniforms, aux, compact_depth: torch.Tensor, cfg, stats: torch.Tensor,
                                      v_distortion: torch.Tensor, v_compact: torch.Tensor) -> torch.Tensor:
    """The bare gradient replay (brush_distortion_compact_grads): ADDS the term's per-record VJP for the upstream
    `v_distortion` [h,w] on L into `v_compact` (float32 [>= N, 16], rows by compact id: words 0-4, 8 and 9) and
    returns it.  `stats`: distortion_from_aux of the same forward and cfg.  ValueError in deterministic mode."""
    h, w, n, dev = _frame(uniforms, compact_depth)
    _refuse_deterministic(aux)
    check_tensor(stats, torch.float32, (h, w, 4), "stats", dev)
    check_tensor(v_distortion, torch.float32, (h, w), "v_distortion", dev)
    if not isinstance(v_compact, torch.Tensor) or v_compact.dim() != 2 or v_compact.shape[1] != COMPACT_STRIDE \
            or v_compact.shape[0] < max(n, 1) or v_compact.dtype != torch.float32 or v_compact.device != dev \
            or not v_compact.is_contiguous():
        raise ValueError(f"v_compact must be a contiguous float32 [>= {max(n, 1)}, {COMPACT_STRIDE}] tensor on {dev}")
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_distortion_compact_grads(
            C.byref(uniforms), C.byref(s), compact_depth.data_ptr(), C.byref(cfg), stats.data_ptr(),
            v_distortion.data_ptr(), n, v_compact.data_ptr(), _lib.current_stream(dev)),
            "brush_distortion_compact_grads")
    return v_compact


def backward_distortion(u, aux, means, log_scales, quats, raw_opacity, ncoef, out_img, v_out, compact_depth, v_depth,
                        cfg, stats, v_distortion, block: Optional[torch.Tensor] = None):
    """brush_render_backward_distortion on one finished depth forward: render._backward_impl's results (the dict of
    dense gradients and their block) for the gradients `v_out` [h,w,4] on the image, `v_depth` [h,w] on the accumulated
    depth and `v_distortion` [h,w] on L together."""
    _refuse_deterministic(aux)
    check_tensor(stats, torch.float32, (int(u.img_size[1]), int(u.img_size[0]), 4), "stats", means.device)
    return R._backward_impl(u, aux, means, log_scales, quats, raw_opacity, ncoef, out_img, v_out, block,
                            depth=(compact_depth, v_depth), distortion=(cfg, stats, v_distortion))


def render_distortion(camera, img_size, means, log_scales, quats, sh_coeffs, raw_opacity, *, mode: str = "depth",
                      near: float = DEFAULT_NEAR, far: Optional[float] = None, antialiased: bool = False,
                      max_intersects: Optional[int] = None):
    """One render_splats_depth plus the distortion replay of THAT forward: (img [h,w,4], depth [h,w],
    distortion [h,w], aux).  img, depth and aux are bitwise render_splats_depth's (default mode); distortion is L(p) of
    the module docstring.  All three outputs are differentiable with respect to all five parameter tensors, through
    the blending weights too; `sh_coeffs` receives zeros from the distortion.  mode, near, far: distortion_config (`far`
    is required for "ndc").  Raises ValueError in deterministic mode (render.DETERMINISTIC / BRUSH_DETERMINISTIC).
    `quats` must be unit quaternions, as for render_splats."""
    cfg = distortion_config(mode, near, far)
    R._check_inputs(means, None, log_scales, quats, sh_coeffs, raw_opacity)
    if R.deterministic_default():
        raise ValueError("render_distortion has no deterministic mode: that mode keeps one gradient row per "
                         "intersection, the term adds into per-splat rows")
    (img, depth, dist), holder = R._render_op(camera, img_size, means, None, log_scales, quats, sh_coeffs, raw_opacity,
                                              max_intersects=max_intersects, deterministic=False,
                                              antialiased=antialiased, distortion=cfg)
    return img, depth, dist, holder["aux"]


def distortion_loss_into(stats: torch.Tensor, v_distortion_out: torch.Tensor, *, weight: float,
                         mask: Optional[torch.Tensor] = None, loss_accum: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The trainer's form of weight * mean over ALL pixels of L: with kappa = weight / (w h), fills `v_distortion_out`
    [h,w] float32 with kappa (0 where the uint8 [h,w] `mask` is 0) and returns (v_distortion_out, term), term = kappa
    times the (masked) sum of stats[..., 0], summed in float64, a 0-dim float32 device tensor; a float32 [1]
    `loss_accum` receives `+= term`.  No graph, no read-back, no synchronisation."""
    if not isinstance(stats, torch.Tensor) or stats.dim() != 3 or stats.shape[2] != 4 or stats.dtype != torch.float32:
        raise ValueError("stats must be the float32 [h,w,4] result of distortion_from_aux")
    h, w, dev = int(stats.shape[0]), int(stats.shape[1]), stats.device
    check_tensor(v_distortion_out, torch.float32, (h, w), "v_distortion_out", dev)
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"weight must be finite and >= 0, got {weight!r}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (h, w)
                             or mask.dtype != torch.uint8 or mask.device != dev):
        raise ValueError(f"mask must be a uint8 [h,w] = {(h, w)} tensor on the stats' device")
    if loss_accum is not None and (loss_accum.numel() != 1 or loss_accum.dtype != torch.float32
                                   or loss_accum.device != dev):
        raise ValueError("loss_accum must be one float32 word on the stats' device")
    kappa = weight / (w * h)
    with torch.no_grad():
        L = stats[..., 0]
        if mask is None:
            v_distortion_out.fill_(kappa)
        else:
            keep = mask != 0
            v_distortion_out.copy_(keep.to(torch.float32) * kappa)
            L = torch.where(keep, L, torch.zeros((), dtype=torch.float32, device=dev))
        term = (L.sum(dtype=torch.float64) * kappa).to(torch.float32)
        if loss_accum is not None:
            loss_accum.view(-1).add_(term)
    return v_distortion_out, term
