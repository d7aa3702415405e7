"""Per-view bilateral grids: a low-resolution 3D lattice of affine colour maps per training view, indexed by pixel
position and by the pixel's own luminance, sliced through the render before the loss.

`ExposureTable` gives a view one global 3x4 map: auto-exposure and white balance.  What varies inside a photograph
(vignetting, local tone mapping, highlight roll-off, brightness-dependent ISP colour) needs a map per place and per
brightness.  A view i carries G_i [GL, GH, GW, 12] float32 (each vertex the row-major [A | b] of exposure.py, the
identity at the start); pixel (x, y) of the premultiplied render reads it trilinearly at (x, y, luminance) and the
resulting 3x4 map is applied as the exposure map is (include/brush_hip.h: brush_bilagrid_forward / _backward /
_backward_adam has the arithmetic; kernels in brush_amd/csrc/bilagrid.hip).  gsplat's use_bilateral_grid and Wang et al.,
"Bilateral Guided Radiance Field Processing" (SIGGRAPH 2024) are the models.

`apply_bilagrid` is the differentiable map for callers who drive a grid from a model of their own, `bilagrid_tv` the
total-variation prior in plain torch ops.  `BilagridTable` is what the trainer uses: every view's grid, its Adam
moments, the scratch and the output image live on the device, the gradient is finished and the prior added inside the
call that steps the grid, and a step neither uploads, reads back nor synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .exposure import IDENTITY, _check_image

DEFAULT_SHAPE = (16, 16, 8)  # (GW, GH, GL)


def check_shape(shape) -> Tuple[int, int, int]:
    """(GW, GH, GL) as three ints, or a ValueError: 2 <= GW, GH <= 64 and 2 <= GL <= 8."""
    try:
        gw, gh, gl = (int(s) for s in shape)
        ok = all(int(s) == s for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"a bilateral grid's shape is (GW, GH, GL), got {shape!r}") from None
    if not ok or not (2 <= gw <= 64 and 2 <= gh <= 64 and 2 <= gl <= 8):
        raise ValueError(f"a bilateral grid's shape (GW, GH, GL) needs 2 <= GW, GH <= 64 and 2 <= GL <= 8, got {shape!r}")
    return gw, gh, gl


def workspace_bytes(w: int, h: int, shape=DEFAULT_SHAPE) -> int:
    gw, gh, gl = check_shape(shape)
    return _lib.size_query("brush_bilagrid_workspace_size", int(w), int(h), gw, gh, gl)


def bilagrid_identity(shape=DEFAULT_SHAPE, device=None) -> torch.Tensor:
    """The grid that changes nothing: [GL, GH, GW, 12] float32, [I | 0] at every vertex."""
    gw, gh, gl = check_shape(shape)
    return torch.tensor(IDENTITY, dtype=torch.float32, device=device).repeat(gl, gh, gw, 1)


def bilagrid_tv(grid: torch.Tensor) -> torch.Tensor:
    """The total-variation prior: the sum over the three axes of the mean, over all adjacent vertex pairs along the axis
    and all 12 words, of the squared difference.  grid: [..., GL, GH, GW, 12]; plain torch ops, differentiable.  The
    table's Adam step adds tv times this function's gradient inside the kernel."""
    if grid.dim() < 4 or grid.shape[-1] != 12:
        raise ValueError(f"grid must be [..., GL, GH, GW, 12], got {tuple(grid.shape)}")
    dz = grid[..., 1:, :, :, :] - grid[..., :-1, :, :, :]
    dy = grid[..., :, 1:, :, :] - grid[..., :, :-1, :, :]
    dx = grid[..., :, :, 1:, :] - grid[..., :, :, :-1, :]
    return (dx * dx).mean() + (dy * dy).mean() + (dz * dz).mean()


def _grid_dims(grid: torch.Tensor, img: torch.Tensor):
    if grid.dim() != 4 or grid.shape[3] != 12 or grid.dtype != torch.float32 or grid.device != img.device:
        raise ValueError(f"grid must be a float32 [GL,GH,GW,12] tensor on img's device, got {tuple(grid.shape)} "
                         f"{grid.dtype}")
    return check_shape((grid.shape[2], grid.shape[1], grid.shape[0]))


class _ApplyBilagrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, grid):
        _check_image(img, "img")
        gw, gh, gl = _grid_dims(grid, img)
        img_c, g_c = img.detach().contiguous(), grid.detach().contiguous()
        h, w = int(img_c.shape[0]), int(img_c.shape[1])
        out = torch.empty_like(img_c)
        with torch.cuda.device(img_c.device):
            _lib.check(_lib.lib().brush_bilagrid_forward(img_c.data_ptr(), g_c.data_ptr(), gw, gh, gl, w, h,
                                                         out.data_ptr(), _lib.current_stream(img_c.device)),
                       "brush_bilagrid_forward")
        ctx.save_for_backward(img_c, g_c)
        return out

    @staticmethod
    def backward(ctx, v_out):
        img_c, g_c = ctx.saved_tensors
        gw, gh, gl = g_c.shape[2], g_c.shape[1], g_c.shape[0]
        h, w = int(img_c.shape[0]), int(img_c.shape[1])
        v_out = v_out.contiguous().float()
        v_img = torch.empty_like(img_c)
        v_g = torch.empty_like(g_c)
        nbytes = workspace_bytes(w, h, (gw, gh, gl))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img_c.device)
        with torch.cuda.device(img_c.device):
            _lib.check(_lib.lib().brush_bilagrid_backward(img_c.data_ptr(), v_out.data_ptr(), g_c.data_ptr(), gw, gh, gl,
                                                          w, h, v_img.data_ptr(), v_g.data_ptr(), ws.data_ptr(), nbytes,
                                                          _lib.current_stream(img_c.device)), "brush_bilagrid_backward")
        return v_img, v_g


def apply_bilagrid(img: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """`grid` ([GL,GH,GW,12] float32) sliced through the premultiplied image `img` ([h,w,4] float32 on the GPU, same
    device).  Differentiable with respect to both (the image also through its luminance, the grid's third coordinate)."""
    return _ApplyBilagrid.apply(img, grid)


class BilagridTable:
    """One grid per training view, stepped by Adam inside brush_bilagrid_backward_adam.

    lr: Adam learning rate (backward_step's `lr` overrides it per call, e.g. a schedule); shape: (GW, GH, GL);
    tv: weight of the total-variation prior, whose gradient (of the grid as it was before the step) is added to the
    data gradient in front of Adam and to no reported loss.  Betas 0.9 / 0.999 and eps 1e-15 as every other group of the
    trainer.  Device state: params, moment1, moment2 [V,GL,GH,GW,12], the last data gradient v_grid [GL,GH,GW,12], the
    scratch and the output image (reused while the size holds).  Host state: the per-view step count."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-15

    def __init__(self, num_views: int, device, lr: float, shape: Sequence[int] = DEFAULT_SHAPE, tv: float = 10.0):
        self.num_views = int(num_views)
        self.device = torch.device(device)
        assert self.device.type == "cuda", "brush_amd has no CPU path: the table lives on the GPU"
        self.shape = check_shape(shape)
        self.lr, self.tv = float(lr), float(tv)
        gw, gh, gl = self.shape
        self.params = bilagrid_identity(self.shape).repeat(self.num_views, 1, 1, 1, 1).to(self.device)
        self.moment1 = torch.zeros_like(self.params)
        self.moment2 = torch.zeros_like(self.params)
        self.v_grid = torch.zeros((gl, gh, gw, 12), dtype=torch.float32, device=self.device)
        self.steps = [0] * self.num_views
        self._view_bytes = gl * gh * gw * 48
        self._size = None   # (w, h) the scratch and the image below are sized for
        self._ws, self._ws_bytes, self._out = None, 0, None

    def _buffers(self, w: int, h: int):
        if self._size != (w, h):
            self._ws_bytes = workspace_bytes(w, h, self.shape)
            self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
            self._out = torch.empty((h, w, 4), dtype=torch.float32, device=self.device)
            self._size = (w, h)

    def _check(self, i: int, img: torch.Tensor, what: str):
        if not 0 <= i < self.num_views:
            raise IndexError(f"view {i} outside the table's {self.num_views} views")
        _check_image(img, what)
        if not img.is_contiguous() or img.device != self.device:
            raise ValueError(f"{what} must be contiguous and on the table's device")

    def forward(self, i: int, pred: torch.Tensor) -> torch.Tensor:
        """G_i sliced through the raw render.  The returned image is the table's own buffer: the next forward overwrites
        it."""
        self._check(i, pred, "pred")
        h, w = int(pred.shape[0]), int(pred.shape[1])
        self._buffers(w, h)
        gw, gh, gl = self.shape
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().brush_bilagrid_forward(pred.data_ptr(), self.params.data_ptr() + self._view_bytes * i,
                                                         gw, gh, gl, w, h, self._out.data_ptr(),
                                                         _lib.current_stream(self.device)), "brush_bilagrid_forward")
        return self._out

    def backward_step(self, i: int, pred: torch.Tensor, v_out: torch.Tensor, lr: Optional[float] = None) -> torch.Tensor:
        """d L / d pred from v_out = d L / d out (written into v_out's own storage and returned), and one Adam step of
        G_i from the gradient of the same call plus the prior's.  self.v_grid holds the data gradient (before the
        prior)."""
        self._check(i, pred, "pred")
        self._check(i, v_out, "v_out")
        if v_out.shape != pred.shape:
            raise ValueError("v_out must have pred's shape")
        h, w = int(pred.shape[0]), int(pred.shape[1])
        self._buffers(w, h)
        self.steps[i] += 1
        gw, gh, gl = self.shape
        cfg = _lib.BrushBilagridAdam(self.lr if lr is None else float(lr), self.BETA1, self.BETA2, self.EPS, self.tv,
                                     self.steps[i])
        off = self._view_bytes * i
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().brush_bilagrid_backward_adam(
                pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), gw, gh, gl, w, h, v_out.data_ptr(),
                self.params.data_ptr() + off, self.moment1.data_ptr() + off, self.moment2.data_ptr() + off,
                self.v_grid.data_ptr(), self._ws.data_ptr(), self._ws_bytes, _lib.current_stream(self.device)),
                "brush_bilagrid_backward_adam")
        return v_out

    def grids(self) -> np.ndarray:
        """[V,GL,GH,GW,12] float32: every view's grid as the table holds it now (one readback; synchronises)."""
        return self.params.detach().cpu().numpy()

    def state_dict(self) -> dict:
        return {"num_views": self.num_views, "shape": tuple(self.shape), "lr": self.lr, "tv": self.tv,
                "params": self.params.clone(), "moment1": self.moment1.clone(), "moment2": self.moment2.clone(),
                "steps": list(self.steps)}

    def load_state_dict(self, state: dict) -> None:
        if int(state["num_views"]) != self.num_views or tuple(state["shape"]) != tuple(self.shape):
            raise ValueError(f"the state holds {state['num_views']} views of shape {tuple(state['shape'])}, the table "
                             f"{self.num_views} of shape {tuple(self.shape)}")
        self.lr, self.tv = float(state["lr"]), float(state["tv"])
        for name in ("params", "moment1", "moment2"):
            getattr(self, name).copy_(state[name].to(self.device, torch.float32).reshape(self.params.shape))
        self.steps = [int(s) for s in state["steps"]]
