"""Camera-pose parametrisation and the per-view pose optimiser of the trainer (host side, torch on the CPU).

A training view's world-to-camera matrix is refined as a camera-frame twist on top of the matrix the dataset gave:

    viewmat_i = se3_exp(delta_i) @ viewmat0_i          delta = (omega, tau): rotation vector, then translation

`PoseTable` keeps one delta per training view with its Adam moments and step count.  The gradient of a step's loss with
respect to the view matrix comes from the render backward (brush_render_backward_pose / _adam_pose) as 12 words on the
device; `push` copies them into the view's pinned slot without blocking and `apply` — called when the view is next
drawn — waits for that copy, chains the gradient to the view's delta and takes one Adam step.  Updates are therefore
applied in a fixed order that depends only on the order views are drawn in: a seeded deterministic run repeats bit for
bit, and a step waits for the GPU only when the same view is drawn twice in a row.

gsplat's trainer (`pose_opt`, a per-camera embedding optimised by Adam with a small weight decay) is the model; the
parametrisation here is the plain twist, which needs no network and has the identity at delta = 0.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

_SERIES_BELOW = 1e-2  # theta^2 under which the coefficient series are used (their next term is < 3e-18 there)


def _hat(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3_exp(delta: torch.Tensor) -> torch.Tensor:
    """exp of the twist delta = (omega[3], tau[3]) as a [4,4] rigid transform [[R, V tau], [0, 1]]:
    R = I + A K + B K^2, V = I + B K + C K^2 with K = [omega]x, theta = |omega|, A = sin(theta) / theta,
    B = (1 - cos(theta)) / theta^2, C = (theta - sin(theta)) / theta^3.  Closed form, with the Taylor series of A, B, C
    in theta^2 below theta = 0.1 (no 0/0, no cancellation, and a finite gradient at delta = 0).  Evaluated in float64
    whatever the input type and returned as float64: the caller casts once.  Differentiable."""
    d = delta.to(torch.float64).reshape(6)
    w, tau = d[:3], d[3:]
    t2 = (w * w).sum()
    small = bool(t2.detach() < _SERIES_BELOW)
    if small:
        A = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
        B = 0.5 * (1.0 - t2 / 12.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0 * (1.0 - t2 / 90.0))))
        Cc = (1.0 / 6.0) * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0))))
    else:
        th = torch.sqrt(t2)
        A = torch.sin(th) / th
        half = torch.sin(0.5 * th) / (0.5 * th)
        B = 0.5 * half * half  # (1 - cos) / theta^2 without the cancellation
        Cc = (th - torch.sin(th)) / (th * t2)
    K = _hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=torch.float64)
    R = eye + A * K + B * K2
    V = eye + B * K + Cc * K2
    top = torch.cat([R, (V @ tau).reshape(3, 1)], dim=1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    return torch.cat([top, bottom], dim=0)


def apply_delta(viewmat0: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """se3_exp(delta) @ viewmat0: the world-to-camera matrix after the camera-frame twist `delta` (float64)."""
    return se3_exp(delta) @ viewmat0.to(torch.float64)


class PoseTable:
    """One twist per training view, refined by Adam from the render backward's view-matrix gradients.

    lr_rot / lr_trans: Adam learning rates of the rotation and translation halves of a delta; reg: weight of the
    (coupled) penalty reg/2 |delta|^2, i.e. reg * delta is added to the gradient, which keeps the refined poses near the
    dataset's and fixes the gauge the scene shares with its cameras.  All state is float64 on the CPU."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-15

    def __init__(self, num_views: int, lr_rot: float, lr_trans: float, reg: float = 0.0):
        self.num_views = int(num_views)
        self.lr = torch.tensor([lr_rot] * 3 + [lr_trans] * 3, dtype=torch.float64)
        self.reg = float(reg)
        self.delta = torch.zeros((self.num_views, 6), dtype=torch.float64)
        self.m1 = torch.zeros_like(self.delta)
        self.m2 = torch.zeros_like(self.delta)
        self.steps = [0] * self.num_views
        self._base: List[Optional[torch.Tensor]] = [None] * self.num_views  # viewmat0 per view (float64 [4,4])
        self._slots: Optional[torch.Tensor] = None                           # [num_views, 12] f32, pinned with a GPU
        self._events: List[Optional[object]] = [None] * self.num_views
        self._pending = [False] * self.num_views

    # ---- matrices
    def set_base(self, i: int, viewmat0) -> None:
        self._base[i] = torch.as_tensor(np.asarray(viewmat0, dtype=np.float64).reshape(4, 4)).clone()

    def viewmat(self, i: int, camera=None) -> torch.Tensor:
        """View i's current world-to-camera matrix, float32 [4,4] on the CPU; `camera` supplies the dataset's matrix
        (camera.world_to_local()) the first time the view is seen."""
        if self._base[i] is None:
            if camera is None:
                raise ValueError(f"view {i} has no base matrix yet: pass its camera")
            self.set_base(i, camera.world_to_local())
        with torch.no_grad():
            return apply_delta(self._base[i], self.delta[i]).to(torch.float32)

    # ---- gradients
    def _slot(self, i: int) -> torch.Tensor:
        if self._slots is None:
            self._slots = torch.zeros((self.num_views, 12), dtype=torch.float32,
                                      pin_memory=torch.cuda.is_available())
        return self._slots[i]

    def push(self, i: int, v_viewmat, stream=None) -> None:
        """Hands view i the 12 words of its view-matrix gradient (row-major 3x4).  A device tensor is copied into the
        view's pinned slot on `stream` (default: the current one) without blocking, and an event is recorded behind
        the copy; a host array is stored as is."""
        slot = self._slot(i)
        if isinstance(v_viewmat, torch.Tensor) and v_viewmat.is_cuda:
            s = torch.cuda.current_stream(v_viewmat.device) if stream is None else stream
            with torch.cuda.stream(s):
                slot.copy_(v_viewmat.reshape(12), non_blocking=True)
                if self._events[i] is None:
                    self._events[i] = torch.cuda.Event()
                self._events[i].record(s)
        else:
            slot.copy_(torch.as_tensor(np.asarray(v_viewmat, dtype=np.float32).reshape(12)))
            self._events[i] = None
        self._pending[i] = True

    def grad_delta(self, i: int, v_viewmat34: torch.Tensor) -> torch.Tensor:
        """d L / d delta_i from d L / d viewmat rows 0..2 ([3,4]), through apply_delta at the current delta."""
        d = self.delta[i].clone().requires_grad_(True)
        M = apply_delta(self._base[i], d)
        (M[:3] * v_viewmat34.to(torch.float64)).sum().backward()
        return d.grad

    def apply(self, i: int) -> bool:
        """Applies view i's pending gradient, if any: waits for its copy, chains it to delta_i, adds reg * delta_i and
        takes one Adam step.  Returns whether a step was taken."""
        if not self._pending[i]:
            return False
        if self._events[i] is not None:
            self._events[i].synchronize()
        self._pending[i] = False
        g = self.grad_delta(i, self._slot(i).reshape(3, 4).clone())
        g = g + self.reg * self.delta[i]
        self.steps[i] += 1
        t = self.steps[i]
        self.m1[i] = self.BETA1 * self.m1[i] + (1.0 - self.BETA1) * g
        self.m2[i] = self.BETA2 * self.m2[i] + (1.0 - self.BETA2) * g * g
        mhat = self.m1[i] / (1.0 - self.BETA1 ** t)
        vhat = self.m2[i] / (1.0 - self.BETA2 ** t)
        self.delta[i] = self.delta[i] - self.lr * mhat / (torch.sqrt(vhat) + self.EPS)
        return True

    def apply_all(self) -> int:
        """Applies every pending gradient in view order (the end of a run)."""
        return sum(1 for i in range(self.num_views) if self.apply(i))

    def deltas(self) -> List[List[float]]:
        return [[float(x) for x in row] for row in self.delta]
