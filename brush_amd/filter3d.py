"""The 3D smoothing filter of Mip-Splatting (Yu et al. 2024) — the world-space half of its antialiasing; the 2D half is
the antialiased render mode.

Every splat is low-passed at the highest rate any training view sampled it: a splat carries a filter length f
(`filter3d_rates`), the renderer sees the covariance Sigma + f^2 I and the opacity scaled by sqrt(det Sigma / det(Sigma +
f^2 I)) (`apply_filter3d`, a map of the log-scales and the raw opacity alone, so it sits in front of every render entry
point).  A splat that training shrank below what any training pixel could resolve then stays a blob, not a needle or a
hole, when the camera moves closer than the training views.  `Splats.bake_filter3d` writes the effective parameters into
a new Splats (Mip-Splatting's "fused" export: any viewer shows it correctly); TrainConfig.filter3d trains with it.

The three kernels are brush_filter3d_rates / _apply / _backward (include/brush_hip.h, brush_amd/csrc/filter3d.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .render import view_parts

VIEW_WORDS = C.sizeof(_lib.BrushFilterView) // 4  # 24: one record as float32 words
MIN_RAW_OPACITY = -87.33654  # BRUSH_FILTER3D_MIN_RAW_OPACITY: the floor of the effective raw opacity


def view_chunk() -> int:
    """C: the number of view records brush_filter3d_rates stages in LDS at a time."""
    return int(_lib.lib().brush_filter3d_view_chunk())


def view_records(views: Sequence) -> np.ndarray:
    """The views as brush_filter3d_rates reads them: a float32 [V, 24] host array (BrushFilterView per row; the two
    sizes are uint32 words).  `views`: SceneViews (camera and image size) or (Camera, (w, h)) pairs; sizes and
    intrinsics are those of the views as given, the matrix is Camera.world_to_local() stored column-major."""
    rec = np.zeros((len(views), VIEW_WORDS), dtype=np.float32)
    words = rec.view(np.uint32)
    for i, view in enumerate(views):
        cam, (w, h) = view_parts(view)[:2]
        if w < 1 or h < 1:
            raise ValueError(f"view {i}: the image size must be positive, got {(w, h)}")
        rec[i, :16] = np.asarray(cam.world_to_local(), dtype=np.float32).T.reshape(16)
        rec[i, 16:18] = cam.focal((w, h))
        rec[i, 18:20] = cam.center((w, h))
        words[i, 20], words[i, 21] = w, h
    return rec


def filter3d_rates(means: torch.Tensor, views, *, near: float = 0.2, margin: float = 0.15,
                   variance: float = 0.2) -> torch.Tensor:
    """The filter length of every splat, float32 [N] on the means' device (brush_filter3d_rates): sqrt(variance) over
    the largest fx / depth among the views that see the splat (depth > near, projection within `margin` of the image
    on each side); a splat no view sees takes the largest length among the seen ones; all 0 when nothing is seen or
    there is no view.  `views`: SceneViews or (Camera, (w, h)) pairs, or the float32 [V, 24] device tensor of their
    `view_records` (a caller that refreshes the filter often uploads them once: the call is then launches only)."""
    assert means.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"means must be [N,3], got {tuple(means.shape)}")
    for name, x in (("near", near), ("margin", margin), ("variance", variance)):
        if not (np.isfinite(x) and x >= 0):
            raise ValueError(f"{name} must be finite and >= 0, got {x!r}")
    if isinstance(views, torch.Tensor):
        rec = views
        if rec.dim() != 2 or rec.shape[1] != VIEW_WORDS or rec.dtype != torch.float32 or rec.device != means.device \
                or not rec.is_contiguous():
            raise ValueError(f"view records must be a contiguous float32 [V,{VIEW_WORDS}] tensor on the means' device")
    else:
        rec = torch.from_numpy(view_records(views)).to(means.device)
    means = means.detach().contiguous().float()
    n, nv = int(means.shape[0]), int(rec.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=means.device)
    with torch.cuda.device(means.device):
        _lib.check(_lib.lib().brush_filter3d_rates(means.data_ptr(), n, rec.data_ptr() if nv else None, nv, float(near),
                                                   float(margin), float(variance), out.data_ptr(),
                                                   _lib.current_stream()), "brush_filter3d_rates")
    return out


def check_filter(filter: torch.Tensor, n: int, device) -> torch.Tensor:
    """`filter` as the kernels read it, or a ValueError: a contiguous float32 [n] tensor on `device`."""
    if not isinstance(filter, torch.Tensor) or tuple(filter.shape) != (n,) or filter.dtype != torch.float32 \
            or filter.device != device or not filter.is_contiguous():
        got = (tuple(filter.shape), filter.dtype, filter.device) if isinstance(filter, torch.Tensor) else type(filter)
        raise ValueError(f"the 3D filter must be a contiguous float32 [{n}] tensor on {device} (one length per splat), "
                         f"got {got}")
    return filter


def apply_into(log_scales, raw_opacity, filter, n: int, stream) -> Tuple[torch.Tensor, torch.Tensor]:
    """brush_filter3d_apply on checked, contiguous float32 tensors: (effective log-scales, effective raw opacities)."""
    out_l, out_o = torch.empty_like(log_scales), torch.empty_like(raw_opacity)
    _lib.check(_lib.lib().brush_filter3d_apply(log_scales.data_ptr(), raw_opacity.data_ptr(), filter.data_ptr(), n,
                                               out_l.data_ptr(), out_o.data_ptr(), stream), "brush_filter3d_apply")
    return out_l, out_o


def backward_into(log_scales, raw_opacity, filter, n: int, v_scales, v_opac, stream):
    """brush_filter3d_backward: the gradients at the effective parameters become, in place, those at the raw ones."""
    _lib.check(_lib.lib().brush_filter3d_backward(log_scales.data_ptr(), raw_opacity.data_ptr(), filter.data_ptr(), n,
                                                  v_scales.data_ptr(), v_opac.data_ptr(), stream),
               "brush_filter3d_backward")


class _ApplyFilter3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_scales, raw_opacity, filter):
        n = int(log_scales.shape[0])
        l, o = log_scales.detach().contiguous(), raw_opacity.detach().contiguous()
        ctx.save_for_backward(l, o, filter)
        with torch.cuda.device(l.device):
            out_l, out_o = apply_into(l, o.view(-1), filter, n, _lib.current_stream())
        return out_l, out_o.view(raw_opacity.shape)

    @staticmethod
    def backward(ctx, v_l, v_o):
        l, o, filter = ctx.saved_tensors
        n = int(l.shape[0])
        # (fresh buffers: the kernel works in place, autograd's incoming gradients are not ours to overwrite)
        v_l = torch.zeros_like(l) if v_l is None else v_l.float().contiguous().clone()
        v_o = torch.zeros_like(o) if v_o is None else v_o.float().contiguous().clone()
        with torch.cuda.device(l.device):
            backward_into(l, o.view(-1), filter, n, v_l, v_o.view(-1), _lib.current_stream())
        return v_l, v_o, None


def apply_filter3d(log_scales: torch.Tensor, raw_opacity: torch.Tensor,
                   filter: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(effective log-scales [N,3], effective raw opacities [N]) under the filter lengths `filter` [N]: the parameters a
    renderer that knows nothing of the filter draws correctly.  l'_k = ln sqrt(s_k^2 + f^2), raw' = logit(sigmoid(raw)
    prod_k s_k / sqrt(s_k^2 + f^2)).  Differentiable in the first two arguments (brush_filter3d_backward); rows with
    f == 0 go through bit for bit, in values and in gradients.  Where the opacity factor underflows the result is
    MIN_RAW_OPACITY, never NaN or -inf."""
    assert log_scales.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    n = int(log_scales.shape[0])
    if tuple(log_scales.shape) != (n, 3) or int(raw_opacity.numel()) != n or raw_opacity.shape[0] != n:
        raise ValueError(f"expected log_scales [N,3] and raw_opacity [N], got {tuple(log_scales.shape)} / "
                         f"{tuple(raw_opacity.shape)}")
    if log_scales.dtype != torch.float32 or raw_opacity.dtype != torch.float32:
        raise ValueError("log_scales and raw_opacity must be float32")
    filter = check_filter(filter.detach() if isinstance(filter, torch.Tensor) else filter, n, log_scales.device)
    return _ApplyFilter3dFn.apply(log_scales, raw_opacity, filter)
