"""Per-view exposure compensation: a 3x4 affine colour map per training view, applied to the render before the loss.

Real captures come with auto-exposure and auto-white-balance, so every photograph has its own gain and tint.  A training
view i carries E_i = [A_i | b_i] (12 floats row-major, [I | 0] at the start); for a rendered premultiplied pixel
p = (r, g, b, alpha)

    out_c = A[c,0] r + A[c,1] g + A[c,2] b + alpha b_c        out_alpha = alpha

and the loss is taken on `out` (include/brush_hip.h: brush_exposure_forward / _backward / _backward_adam; kernels in
brush_amd/csrc/exposure.hip).  The 3DGS reference trainer's "exposure compensation" is the model; gsplat covers the same
ground with app_opt.

`apply_exposure` is the differentiable map for callers who drive E from a model of their own.  `ExposureTable` is what
the trainer uses: every view's E, its Adam moments, the scratch and the output image live on the device, the gradient is
a 12-word reduction finished inside the call that steps E, and a step neither uploads, reads back nor synchronises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _check_image(img: torch.Tensor, what: str):
    assert img.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if img.dim() != 3 or img.shape[2] != 4 or img.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 [h,w,4] tensor, got {tuple(img.shape)} {img.dtype}")


def workspace_bytes(w: int, h: int) -> int:
    return _lib.size_query("brush_exposure_workspace_size", int(w), int(h))


class _ApplyExposure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, E):
        _check_image(img, "img")
        if E.numel() != 12 or E.dtype != torch.float32 or E.device != img.device:
            raise ValueError("E must be 12 float32 words ([12] or [3,4]) on img's device")
        img_c, e_c = img.detach().contiguous(), E.detach().contiguous()
        h, w = int(img_c.shape[0]), int(img_c.shape[1])
        out = torch.empty_like(img_c)
        with torch.cuda.device(img_c.device):
            _lib.check(_lib.lib().brush_exposure_forward(img_c.data_ptr(), e_c.data_ptr(), w, h, out.data_ptr(),
                                                         _lib.current_stream(img_c.device)), "brush_exposure_forward")
        ctx.save_for_backward(img_c, e_c)
        ctx.e_shape = tuple(E.shape)
        return out

    @staticmethod
    def backward(ctx, v_out):
        img_c, e_c = ctx.saved_tensors
        h, w = int(img_c.shape[0]), int(img_c.shape[1])
        v_out = v_out.contiguous().float()
        v_img = torch.empty_like(img_c)
        v_e = torch.empty(12, dtype=torch.float32, device=img_c.device)
        nbytes = workspace_bytes(w, h)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=img_c.device)
        with torch.cuda.device(img_c.device):
            _lib.check(_lib.lib().brush_exposure_backward(img_c.data_ptr(), v_out.data_ptr(), e_c.data_ptr(), w, h,
                                                          v_img.data_ptr(), v_e.data_ptr(), ws.data_ptr(), nbytes,
                                                          _lib.current_stream(img_c.device)), "brush_exposure_backward")
        return v_img, v_e.reshape(ctx.e_shape)


def apply_exposure(img: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    """E applied to the premultiplied image `img` ([h,w,4] float32 on the GPU); E: [12] or [3,4] float32 on the same
    device.  Differentiable with respect to both."""
    return _ApplyExposure.apply(img, E)


class ExposureTable:
    """One E per training view, stepped by Adam inside brush_exposure_backward_adam.

    lr: Adam learning rate (backward_step's `lr` overrides it per call, e.g. a schedule); reg: weight of the coupled
    penalty reg/2 |E - [I|0]|^2, i.e. reg (E - [I|0]) is added to the gradient, which pins the gain the scene shares
    with its exposures.  Betas 0.9 / 0.999 and eps 1e-15 as every other group of the trainer.  Device state: params,
    moment1, moment2 [V,12], the last gradient [12], the scratch and the output image (reused while the size holds).
    Host state: the per-view step count."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-15

    def __init__(self, num_views: int, device, lr: float, reg: float = 0.0):
        self.num_views = int(num_views)
        self.device = torch.device(device)
        assert self.device.type == "cuda", "brush_amd has no CPU path: the table lives on the GPU"
        self.lr, self.reg = float(lr), float(reg)
        self.params = torch.tensor(IDENTITY, dtype=torch.float32).repeat(self.num_views, 1).to(self.device)
        self.moment1 = torch.zeros((self.num_views, 12), dtype=torch.float32, device=self.device)
        self.moment2 = torch.zeros_like(self.moment1)
        self.v_exposure = torch.zeros(12, dtype=torch.float32, device=self.device)
        self.steps = [0] * self.num_views
        self._size = None   # (w, h) the scratch and the images below are sized for
        self._ws, self._ws_bytes, self._out, self._v_pred = None, 0, None, None

    def _buffers(self, w: int, h: int):
        if self._size != (w, h):
            self._ws_bytes = workspace_bytes(w, h)
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
        """E_i applied to the raw render.  The returned image is the table's own buffer: the next forward overwrites it."""
        self._check(i, pred, "pred")
        h, w = int(pred.shape[0]), int(pred.shape[1])
        self._buffers(w, h)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().brush_exposure_forward(pred.data_ptr(), self.params.data_ptr() + 48 * i, w, h,
                                                         self._out.data_ptr(), _lib.current_stream(self.device)),
                       "brush_exposure_forward")
        return self._out

    def backward_step(self, i: int, pred: torch.Tensor, v_out: torch.Tensor, lr: Optional[float] = None) -> torch.Tensor:
        """d L / d pred from v_out = d L / d out (written into v_out's own storage and returned), and one Adam step of
        E_i from the gradient of the same call.  self.v_exposure holds the 12-word gradient (before the penalty)."""
        self._check(i, pred, "pred")
        self._check(i, v_out, "v_out")
        if v_out.shape != pred.shape:
            raise ValueError("v_out must have pred's shape")
        h, w = int(pred.shape[0]), int(pred.shape[1])
        self._buffers(w, h)
        self.steps[i] += 1
        cfg = _lib.BrushExposureAdam(self.lr if lr is None else float(lr), self.BETA1, self.BETA2, self.EPS, self.reg,
                                     self.steps[i])
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().brush_exposure_backward_adam(
                pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), w, h, v_out.data_ptr(),
                self.params.data_ptr() + 48 * i, self.moment1.data_ptr() + 48 * i, self.moment2.data_ptr() + 48 * i,
                self.v_exposure.data_ptr(), self._ws.data_ptr(), self._ws_bytes, _lib.current_stream(self.device)),
                "brush_exposure_backward_adam")
        return v_out

    def matrices(self) -> np.ndarray:
        """[V,3,4] float32: every view's E as the table holds it now (one readback; synchronises)."""
        return self.params.detach().cpu().numpy().reshape(self.num_views, 3, 4)

    def exposures(self) -> List[List[float]]:
        return [[float(x) for x in row] for row in self.matrices().reshape(self.num_views, 12)]

    def state_dict(self) -> dict:
        return {"num_views": self.num_views, "lr": self.lr, "reg": self.reg, "params": self.params.clone(),
                "moment1": self.moment1.clone(), "moment2": self.moment2.clone(), "steps": list(self.steps)}

    def load_state_dict(self, state: dict) -> None:
        if int(state["num_views"]) != self.num_views:
            raise ValueError(f"the state holds {state['num_views']} views, the table {self.num_views}")
        self.lr, self.reg = float(state["lr"]), float(state["reg"])
        for name in ("params", "moment1", "moment2"):
            getattr(self, name).copy_(state[name].to(self.device, torch.float32).reshape(self.num_views, 12))
        self.steps = [int(s) for s in state["steps"]]
