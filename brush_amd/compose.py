"""Background colour and loss masks: two element-wise maps around the colour loss.

The op renders a premultiplied image with no background and the datasets hold straight-alpha targets.  `compose_forward`
composes the render, and the target, over a background colour b and zeroes the pixels a mask leaves out:

    out.c = img.c + (1 - alpha) b_c        target.c = G_c G_a + (1 - G_a) b_c   (an RGB target is copied)

(include/brush_hip.h: brush_compose_forward / _backward; kernels in brush_amd/csrc/compose.hip).  The loss is taken on
(out, target); `compose_backward` turns its gradient into the gradient at the raw render.  A pixel is kept when there is
no mask or mask != 0, which is COLMAP's and nerfstudio's convention; a pixel that is not kept is +0 in every word of
both images and of the gradient.  With a background the target is opaque RGB ([h,w,3]) and alpha is not compared, as in
gsplat; the loss's mean stays over all pixels, as nerfstudio's (pred * mask, gt * mask).

`compose` is the differentiable form for callers with a loss of their own; the trainer calls the two wrappers directly
(SplatTrainer.step's `background` / `gt_mask`).  The background is a float32 [3] DEVICE tensor, so a colour drawn per
step (`TrainConfig.background = "random"`) costs neither an upload nor a synchronisation.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

_GT_DTYPES = {torch.uint8: _lib.EVAL_GT_U8, torch.float32: _lib.EVAL_GT_F32}
_NAMED = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}


def parse_background(text: str):
    """A command line's --background value: 'white', 'black', 'random' or 'R,G,B' (three floats) -> the name or an
    (r, g, b) tuple, as TrainConfig.background takes it.  ValueError for anything else."""
    t = text.strip().lower()
    if t in ("white", "black", "random"):
        return t
    try:
        rgb = tuple(float(x) for x in t.split(","))
    except ValueError:
        rgb = ()
    if len(rgb) != 3 or not all(x == x and abs(x) != float("inf") for x in rgb):
        raise ValueError(f"--background takes white, black, random or R,G,B, got {text!r}")
    return rgb


def check_background(x):
    """TrainConfig.background / eval_stats' background as given, or a ValueError naming what is wrong with it."""
    if x is None or (isinstance(x, str) and x in ("white", "black", "random")):
        return x
    if isinstance(x, (tuple, list)) and len(x) == 3 and all(
            isinstance(v, (int, float)) and not isinstance(v, bool) for v in x):
        return tuple(float(v) for v in x)
    raise ValueError(f"background must be None, 'white', 'black', 'random' or an (r, g, b) tuple, got {x!r}")


def as_background(x, device, generator: Optional[torch.Generator] = None) -> Optional[torch.Tensor]:
    """None stays None; 'white', 'black' or an (r, g, b) tuple becomes a float32 [3] tensor on `device`; a float32 [3]
    tensor on `device` is passed through; 'random' draws torch.rand(3) from `generator` (a torch.Generator on `device`)
    and is refused without one."""
    if x is None:
        return None
    device = torch.device(device)
    if isinstance(x, torch.Tensor):
        if tuple(x.shape) != (3,) or x.dtype != torch.float32 or x.device != device or not x.is_contiguous():
            raise ValueError(f"a background tensor must be a contiguous float32 [3] tensor on {device}")
        return x
    if isinstance(x, str) and x == "random":
        if generator is None:
            raise ValueError("background 'random' needs a torch.Generator to draw from")
        return torch.rand(3, generator=generator, device=device, dtype=torch.float32)
    x = check_background(x)
    return torch.tensor(_NAMED.get(x, x), dtype=torch.float32).to(device)


def _check_options(img: torch.Tensor, mask, background, what: str):
    assert img.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if img.dim() != 3 or img.shape[2] != 4 or img.dtype != torch.float32 or img.numel() == 0:
        raise ValueError(f"{what} must be a non-empty float32 [h,w,4] tensor, got {tuple(img.shape)} {img.dtype}")
    if mask is None and background is None:
        raise ValueError("compose needs a mask, a background or both")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.device != img.device
                             or tuple(mask.shape) != tuple(img.shape[:2])):
        raise ValueError(f"mask must be a uint8 {tuple(img.shape[:2])} tensor on {what}'s device")
    if background is not None and (not isinstance(background, torch.Tensor) or background.dtype != torch.float32
                                   or background.device != img.device or tuple(background.shape) != (3,)):
        raise ValueError(f"background must be a float32 [3] tensor on {what}'s device (as_background makes one)")


def _check_out(out, shape, like: torch.Tensor, what: str):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
            or not out.is_contiguous() or out.device != like.device):
        raise ValueError(f"{what} must be a contiguous float32 {tuple(shape)} tensor on the image's device")
    return out


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def compose_forward(pred: torch.Tensor, gt: torch.Tensor, *, background: Optional[torch.Tensor] = None,
                    mask: Optional[torch.Tensor] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out_pred [h,w,4], out_gt [h,w,3 with a background, else gt's channels]), both float32, through
    brush_compose_forward; does not synchronise.  pred: [h,w,4] float32, the premultiplied render; gt: [h,w,3|4] uint8
    (read as b / 255) or float32, straight alpha; background: float32 [3] device tensor or None; mask: uint8 [h,w]
    device tensor (nonzero keeps the pixel) or None; at least one of the two.  `out`: an optional (out_pred, out_gt)
    pair of contiguous float32 tensors of those shapes to write into; out_pred may not be pred."""
    _check_options(pred, mask, background, "pred")
    h, w = int(pred.shape[0]), int(pred.shape[1])
    if (not isinstance(gt, torch.Tensor) or gt.dim() != 3 or tuple(gt.shape[:2]) != (h, w) or gt.shape[2] not in (3, 4)
            or gt.device != pred.device):
        raise ValueError(f"gt must be [h,w,3|4] = ({h}, {w}, 3|4) on pred's device, got "
                         f"{tuple(gt.shape) if isinstance(gt, torch.Tensor) else gt!r}")
    if gt.dtype not in _GT_DTYPES:
        raise ValueError(f"gt must be uint8 or float32, got {gt.dtype}")
    cg = int(gt.shape[2])
    out_pred, out_gt = (None, None) if out is None else out
    out_pred = _check_out(out_pred, (h, w, 4), pred, "out[0]")
    out_gt = _check_out(out_gt, (h, w, 3 if background is not None else cg), pred, "out[1]")
    pred, gt = pred.contiguous(), gt.contiguous()
    if out_pred.data_ptr() == pred.data_ptr():
        raise ValueError("out[0] may not be pred: the render backward needs the raw render")
    mask = None if mask is None else mask.contiguous()
    background = None if background is None else background.contiguous()
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().brush_compose_forward(pred.data_ptr(), gt.data_ptr(), _GT_DTYPES[gt.dtype], cg, _ptr(mask),
                                                    _ptr(background), w, h, out_pred.data_ptr(), out_gt.data_ptr(),
                                                    _lib.current_stream(pred.device)), "brush_compose_forward")
    return out_pred, out_gt


def compose_backward(v_out: torch.Tensor, *, background: Optional[torch.Tensor] = None,
                     mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient at the raw render from v_out = d L / d out_pred ([h,w,4] float32, contiguous), through
    brush_compose_backward; does not synchronise.  `out`: a contiguous float32 [h,w,4] tensor to write into; it may be
    v_out itself (in place)."""
    _check_options(v_out, mask, background, "v_out")
    if not v_out.is_contiguous():
        raise ValueError("v_out must be contiguous")
    h, w = int(v_out.shape[0]), int(v_out.shape[1])
    out = _check_out(out, (h, w, 4), v_out, "out")
    mask = None if mask is None else mask.contiguous()
    background = None if background is None else background.contiguous()
    with torch.cuda.device(v_out.device):
        _lib.check(_lib.lib().brush_compose_backward(v_out.data_ptr(), _ptr(mask), _ptr(background), w, h,
                                                     out.data_ptr(), _lib.current_stream(v_out.device)),
                   "brush_compose_backward")
    return out


class _Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, background, mask):
        out, target = compose_forward(img.detach(), gt, background=background, mask=mask)
        ctx.background, ctx.mask = background, mask
        ctx.mark_non_differentiable(target)
        return out, target

    @staticmethod
    def backward(ctx, v_out, _v_target):
        v_img = compose_backward(v_out.contiguous().float(), background=ctx.background, mask=ctx.mask)
        return v_img, None, None, None


def compose(img: torch.Tensor, gt: torch.Tensor, *, background: Optional[torch.Tensor] = None,
            mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, target) of compose_forward, differentiable with respect to `img` (the premultiplied render, [h,w,4]
    float32 on the GPU); `target` carries no gradient.  background / mask as compose_forward takes them."""
    return _Compose.apply(img, gt, background, mask)
