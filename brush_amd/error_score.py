"""Per-splat image error over a set of views: the signal of error-driven densification (build extension; Rota Bulo et
al., "Revising Densification in Gaussian Splatting", ECCV 2024, is the model).

For each view one forward, a per-pixel error map (the clamped mean absolute colour difference, brush_l1_error_map, or a
caller's own) and one replay of the forward's compositing walk (include/brush_hip.h: brush_render_error_scores,
csrc/error_score.hip) that hands every splat its share of the error: the sum over the pixels it was added to of
fac * e, fac = alpha T its blending weight and e the pixel's error in [0, 1], as an exact integer in units of 2^-24.
Per splat the views fold into the largest share (the paper's max over views), the sum and the number of views with a
non-zero share, all on the device and without a synchronisation:

    bufs = splat_error_scores(splats, scene.views)          # launches only
    trainer.set_densify_scores(bufs.scores("max"))           # TrainConfig.densify_by = "error"

A score is in "pixels of full error": 1.0 is one pixel whose colour is off by the whole range and that the splat alone
covers, or many pixels of small error.  The integers are order independent, so the same views give the same bits on
every run, in both aux modes.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _lib

Q24 = float(1 << 24)  # the fixed point of a share (brush_render_error_scores: view_err)
_GT_DTYPES = {torch.uint8: _lib.EVAL_GT_U8, torch.float32: _lib.EVAL_GT_F32}


@dataclass
class ErrorScores:
    """Per-splat error shares over `views` views, as CPU tensors of N rows.
    max: float64, the largest share of one view; sum: float64, the shares of all views summed (both in pixels of full
    error, exact multiples of 2^-24); views_seen: int32, the views in which the splat's share was not zero."""
    max: torch.Tensor
    sum: torch.Tensor
    views_seen: torch.Tensor
    views: int = 0


class ErrorScoreBuffers:
    """The device side of an ErrorScores in the making: view_err, score_max and score_sum [N] i64 and views_seen [N]
    i32, zeroed once here.  brush_render_error_scores accumulates one view into view_err; fold() moves it into the
    other three with torch operations in place and zeroes it again."""

    def __init__(self, n: int, device):
        self.n = int(n)
        rows = max(self.n, 1)
        self.view_err = torch.zeros(rows, dtype=torch.int64, device=device)
        self.score_max = torch.zeros(rows, dtype=torch.int64, device=device)
        self.score_sum = torch.zeros(rows, dtype=torch.int64, device=device)
        self.views_seen = torch.zeros(rows, dtype=torch.int32, device=device)
        self.views = 0

    def fold(self):
        """One view done: score_max = max(score_max, view_err), score_sum += view_err, views_seen += view_err != 0,
        view_err = 0.  Launches only."""
        torch.maximum(self.score_max, self.view_err, out=self.score_max)
        self.score_sum += self.view_err
        self.views_seen += self.view_err != 0
        self.view_err.zero_()
        self.views += 1

    def scores(self, by: str = "max") -> torch.Tensor:
        """A float32 [N] device tensor, nothing read back: int64 -> float64 / 2^24 -> float32 of score_max ("max"),
        score_sum ("sum") or score_sum over max(views_seen, 1) ("mean")."""
        if by not in ("max", "sum", "mean"):
            raise ValueError(f"by must be 'max', 'sum' or 'mean', got {by!r}")
        v = (self.score_max if by == "max" else self.score_sum)[:self.n].to(torch.float64) / Q24
        if by == "mean":
            v = v / self.views_seen[:self.n].clamp_min(1).to(torch.float64)
        return v.to(torch.float32)

    def read(self) -> ErrorScores:
        """The one read-back (synchronises)."""
        return ErrorScores(self.score_max[:self.n].cpu().to(torch.float64) / Q24,
                           self.score_sum[:self.n].cpu().to(torch.float64) / Q24, self.views_seen[:self.n].cpu(),
                           self.views)


def l1_error_map(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """min(((|dr| + |dg|) + |db|) / 3, 1) per pixel as a float32 [h,w] device tensor, 0 where `mask` is 0, through
    brush_l1_error_map; does not synchronise.  pred: [h,w,4] float32 (channels 0..2 are used); gt: [h,w,3|4] uint8 (read
    as b / 255) or float32; mask: uint8 [h,w] or None; out: a contiguous float32 [h,w] tensor to write into."""
    assert pred.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if pred.dim() != 3 or pred.shape[2] != 4 or pred.dtype != torch.float32 or pred.numel() == 0:
        raise ValueError(f"pred must be a non-empty float32 [h,w,4] tensor, got {tuple(pred.shape)} {pred.dtype}")
    h, w = int(pred.shape[0]), int(pred.shape[1])
    if (not isinstance(gt, torch.Tensor) or gt.dim() != 3 or tuple(gt.shape[:2]) != (h, w) or gt.shape[2] not in (3, 4)
            or gt.device != pred.device):
        raise ValueError(f"gt must be [h,w,3|4] = ({h}, {w}, 3|4) on pred's device, got "
                         f"{tuple(gt.shape) if isinstance(gt, torch.Tensor) else gt!r}")
    if gt.dtype not in _GT_DTYPES:
        raise ValueError(f"gt must be uint8 or float32, got {gt.dtype}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8
                             or mask.device != pred.device or tuple(mask.shape) != (h, w)):
        raise ValueError(f"mask must be a uint8 {(h, w)} tensor on pred's device")
    if out is None:
        out = torch.empty((h, w), dtype=torch.float32, device=pred.device)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (h, w) or out.dtype != torch.float32
          or not out.is_contiguous() or out.device != pred.device):
        raise ValueError(f"out must be a contiguous float32 {(h, w)} tensor on pred's device")
    pred, gt = pred.contiguous(), gt.contiguous()
    mask = None if mask is None else mask.contiguous()
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().brush_l1_error_map(pred.data_ptr(), gt.data_ptr(), _GT_DTYPES[gt.dtype],
                                                 int(gt.shape[2]), None if mask is None else mask.data_ptr(),
                                                 out.data_ptr(), w, h, _lib.current_stream(pred.device)),
                   "brush_l1_error_map")
    return out


def error_scores_from_aux(uniforms, aux, error_map: torch.Tensor, bufs: ErrorScoreBuffers) -> ErrorScoreBuffers:
    """The bare call and the fold: replays the finished forward (`uniforms`, `aux`: what render._forward_impl returned,
    or render.pack_uniforms of the same camera and size beside a render's RenderAux), distributes `error_map` (a
    contiguous float32 [h,w] device tensor of the forward's size; values are clamped to [0, 1], a NaN counts as 0) into
    bufs.view_err and folds that view into the maxima and sums.  Runs on the current stream; does not synchronise."""
    dev = bufs.view_err.device
    assert dev.type == "cuda", "brush_amd has no CPU path: the buffers must live on the GPU"
    h, w = int(uniforms.img_size[1]), int(uniforms.img_size[0])
    if (not isinstance(error_map, torch.Tensor) or tuple(error_map.shape) != (h, w)
            or error_map.dtype != torch.float32 or not error_map.is_contiguous() or error_map.device != dev):
        got = f"{error_map.dtype} {tuple(error_map.shape)}" if isinstance(error_map, torch.Tensor) else repr(error_map)
        raise ValueError(f"error_map must be a contiguous float32 [{h},{w}] tensor on the buffers' device, got {got}")
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_error_scores(C.byref(uniforms), C.byref(s), error_map.data_ptr(),
                                                        bufs.view_err.data_ptr(), bufs.n, _lib.current_stream(dev)),
                   "brush_render_error_scores")
    bufs.fold()
    return bufs


def splat_error_scores(splats, views, *, antialiased: bool = False, downscale: int = 1, background=None,
                       use_masks: bool = True, error: Optional[Callable] = None) -> ErrorScoreBuffers:
    """The error shares of `splats` over `views`, each a dataset.SceneView (uploaded here; `downscale` = f > 1: at
    pyramid.downscaled_size of its size) or a (Camera, gt, mask or None) triple of device tensors (gt uint8 or float32
    [h,w,3|4], mask uint8 [h,w]; rendered at gt's size, nothing is uploaded).  Per view: one forward; with a
    `background` (None, "white", "black", an (r, g, b) tuple or a float32 [3] device tensor) compose_forward on the
    render and the target; the error map, l1_error_map by default or `error(pred, gt) -> [h,w]` float32 device tensor
    (e.g. a D-SSIM map; it is given the composed pair, and zeroed under the mask here); the replay and the fold.
    `antialiased`: render in that mode.  The splats are synchronised once; with device-resident views and a device
    background nothing else synchronises.  Returns the ErrorScoreBuffers (scores() stays on the device, read() reads
    back)."""
    from . import render as R
    from .compose import as_background, compose_forward
    from .pyramid import check_factor

    downscale = check_factor(downscale)
    if isinstance(background, str) and background == "random":
        raise ValueError("an error pass has no 'random' background: score over a fixed colour")
    parts = splats.frozen()  # one sync, as Splats.render does per call
    dev = parts[0].device
    bufs = ErrorScoreBuffers(splats.num_splats(), dev)
    bg = as_background(background, dev)
    with torch.no_grad():
        for v in views:
            cam, size, gt, mask = R.view_parts(v, dev, downscale=downscale, gt=True, mask=use_masks)
            pred, aux, u = R.forward_frozen(parts, cam, size, antialiased)
            if bg is not None:
                pred, gt = compose_forward(pred, gt, background=bg, mask=mask)
            if error is None:
                emap = l1_error_map(pred, gt, mask)
            else:
                emap = error(pred, gt)
                if mask is not None:
                    emap = torch.where(mask != 0, emap, torch.zeros_like(emap))
                emap = emap.contiguous()
            error_scores_from_aux(u, aux, emap, bufs)
    return bufs
