"""Depth supervision: an L1 loss between the rendered expected depth and a per-view depth map.

The renderer's depth output is the accumulated depth D = sum T alpha z (render_splats_depth); with a the alpha of the
same render, D / a is the expected depth of the covered part of a pixel.  For a target t = raw * scale + offset from a
uint16 or float32 map (a millimetre 16-bit PNG is scale = 0.001), a pixel counts when the map holds a measurement there
(raw != 0; float32: finite and > 0), t > 0, D > 0 and a >= alpha_min, and

    mode "depth"      r = D / a - t        mode "disparity"   r = a / D - t       (t given in the space of the loss)
    loss = weight / (w h) * sum over the counted pixels of |r|

The mean runs over all w h pixels, as the 3DGS trainer's depth term does, not over the counted ones: one pass over the
pixels then yields the loss and both gradients (include/brush_hip.h: brush_depth_loss; brush_amd/csrc/depth_loss.hip).
The 3DGS trainer's depth regulariser (on inverse depth) and gsplat's depth_loss are the models.

`depth_loss` is the differentiable form for callers who build their own objective; `depth_loss_into` is what the
trainer uses: it adds the alpha gradient into the colour loss's gradient image in place and returns the depth gradient,
without an autograd graph, an upload, a read-back or a synchronisation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib

MODES = {"depth": _lib.DEPTH_LOSS_DEPTH, "disparity": _lib.DEPTH_LOSS_DISPARITY}
# alpha_min = 0.5 reads "mostly covered": a hyper-parameter default, not a measured number.
DEFAULT_ALPHA_MIN = 0.5


def workspace_bytes(w: int, h: int) -> int:
    return _lib.size_query("brush_depth_loss_workspace_size", int(w), int(h))


def _mode(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be 'depth' or 'disparity', got {mode!r}")
    return MODES[mode]


def _target(target: torch.Tensor, h: int, w: int, device) -> Tuple[torch.Tensor, int]:
    """The target as the kernel reads it (uint16 or float32, contiguous) and its gt_dtype."""
    if target.dtype not in (torch.uint16, torch.float32):
        raise ValueError(f"target must be uint16 or float32, got {target.dtype}")
    if tuple(target.shape) != (h, w) or target.device != device:
        raise ValueError(f"target must be [h,w] = {(h, w)} on the render's device, got {tuple(target.shape)} on "
                         f"{target.device}")
    return target.contiguous(), (_lib.DEPTH_GT_U16 if target.dtype == torch.uint16 else _lib.DEPTH_GT_F32)


def depth_loss_into(pred: torch.Tensor, depth: torch.Tensor, target: torch.Tensor, v_pred: Optional[torch.Tensor], *,
                    weight: float = 1.0, scale: float = 1.0, offset: float = 0.0, alpha_min: float = DEFAULT_ALPHA_MIN,
                    mode: str = "depth", loss_accum: Optional[torch.Tensor] = None, want_v_depth: bool = True,
                    workspace: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """brush_depth_loss on one render: returns (v_depth [h,w] float32, stats [2] float32 = {loss, valid fraction}),
    both on the device; does not synchronise.

    pred: [h,w,4] float32, the raw render (its alpha is read); depth: [h,w] float32, the accumulated depth of the same
    render; target: [h,w] uint16 or float32 on the same device.  v_pred: None, or the contiguous [h,w,4] float32
    gradient image the colour loss has written: the alpha gradient of the depth term is added into its alpha channel in
    place (pixels that do not count keep their bits).  loss_accum: optional float32 [1] device tensor that receives
    `+= loss`.  want_v_depth=False with v_pred=None is the metrics-only call (v_depth is returned as None).
    workspace: optional uint8 device tensor of at least workspace_bytes(w, h) bytes to use as scratch."""
    assert pred.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if pred.dim() != 3 or pred.shape[2] != 4 or pred.dtype != torch.float32:
        raise ValueError(f"pred must be a float32 [h,w,4] tensor, got {tuple(pred.shape)} {pred.dtype}")
    h, w = int(pred.shape[0]), int(pred.shape[1])
    dev = pred.device
    if tuple(depth.shape) != (h, w) or depth.dtype != torch.float32 or depth.device != dev:
        raise ValueError(f"depth must be a float32 [h,w] = {(h, w)} tensor on pred's device")
    target, gt_dtype = _target(target, h, w, dev)
    if v_pred is not None and (tuple(v_pred.shape) != (h, w, 4) or v_pred.dtype != torch.float32
                               or not v_pred.is_contiguous() or v_pred.device != dev):
        raise ValueError("v_pred must be a contiguous float32 [h,w,4] tensor on pred's device (it is updated in place)")
    if loss_accum is not None and (loss_accum.numel() != 1 or loss_accum.dtype != torch.float32
                                   or loss_accum.device != dev):
        raise ValueError("loss_accum must be one float32 word on pred's device")
    if not float(alpha_min) > 0.0:
        raise ValueError(f"alpha_min must be > 0, got {alpha_min}")
    cfg = _lib.BrushDepthLoss(float(weight), float(scale), float(offset), float(alpha_min), _mode(mode), gt_dtype)
    pred, depth = pred.contiguous(), depth.contiguous()
    nbytes = workspace_bytes(w, h)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < nbytes or workspace.device != dev:
        raise ValueError(f"workspace must hold {nbytes} bytes on pred's device")
    v_depth = torch.empty((h, w), dtype=torch.float32, device=dev) if want_v_depth else None
    stats = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_depth_loss(
            pred.data_ptr(), depth.data_ptr(), target.data_ptr(), C.byref(cfg), w, h,
            None if v_depth is None else v_depth.data_ptr(), None if v_pred is None else v_pred.data_ptr(),
            stats.data_ptr(), None if loss_accum is None else loss_accum.data_ptr(), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), _lib.current_stream(dev)),
            "brush_depth_loss")
    return v_depth, stats


class _DepthLoss(torch.autograd.Function):
    """The kernel's two gradients are formed in the forward pass (the loss is L1: they do not depend on the incoming
    scalar) and scaled by it in the backward pass."""

    @staticmethod
    def forward(ctx, img, depth, target, weight, scale, offset, alpha_min, mode):
        img_c = img.detach()
        v_img = torch.zeros_like(img_c, memory_format=torch.contiguous_format)
        v_depth, stats = depth_loss_into(img_c, depth.detach(), target, v_img, weight=weight, scale=scale,
                                         offset=offset, alpha_min=alpha_min, mode=mode)
        ctx.save_for_backward(v_img, v_depth)
        return stats[0]

    @staticmethod
    def backward(ctx, v_loss):
        v_img, v_depth = ctx.saved_tensors
        return v_img * v_loss, v_depth * v_loss, None, None, None, None, None, None


def depth_loss(img: torch.Tensor, depth: torch.Tensor, target: torch.Tensor, *, weight: float = 1.0,
               scale: float = 1.0, offset: float = 0.0, alpha_min: float = DEFAULT_ALPHA_MIN,
               mode: str = "depth") -> torch.Tensor:
    """The depth loss of a render as a differentiable scalar (a 0-dim float32 device tensor).

    img, depth: the two outputs of render_splats_depth ([h,w,4] and [h,w] float32); target: [h,w] uint16 or float32 on
    the same device, read as raw * scale + offset, 0 (float32: anything not finite and positive) meaning "no
    measurement".  mode "depth" compares depth / alpha with the target, "disparity" alpha / depth (the target is then
    an inverse depth).  Pixels with alpha < alpha_min, a non-positive rendered depth or target do not count; the mean
    runs over all pixels (see the module's docstring).  Gradients flow to img's alpha channel and to depth."""
    return _DepthLoss.apply(img, depth, target, float(weight), float(scale), float(offset), float(alpha_min), mode)
