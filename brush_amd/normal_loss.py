"""Normal maps and the depth-normal consistency loss (build extension; 2DGS, GOF, RaDe-GS and PGSR are the models).

    L_n = sum_i w_i (1 - n_i . N)

n_i: the normal of splat i, its shortest axis in camera space turned towards the camera (brush_splat_normals);
w_i = alpha_i T_i its blending weight; N: the normal of the surface the rendered depth map implies.  The sum over the
splats is a feature replay of the finished forward (features.features_from_aux with the per-splat normals as the three
channels): per pixel the term is A - Nr . Nd, A the render's alpha, Nr the rendered normal map, Nd the normal from the
depth map, and

    loss = weight / (w h) * sum over the valid pixels of (A - Nr . Nd)

the mean over ALL pixels, as depth_loss has it.  A pixel counts when A >= alpha_min, the accumulated depth D is > 0 and
both are finite; its point is P = (D / A) ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1); an interior pixel whose four
edge neighbours count too is valid when c = (P(x,y+1) - P(x,y-1)) x (P(x+1,y) - P(x-1,y)) has a finite positive squared
length, and Nd = c / |c| (a fronto-parallel plane gives (0, 0, -1): facing the camera, like the splat normals).
include/brush_hip.h (brush_normal_loss) has every gradient; brush_amd/csrc/normal_loss.hip the evaluation order.

THE BLENDING WEIGHTS ARE FROZEN in the rendered normal map: it is a replay of a finished forward, differentiable with
respect to the per-splat normals (hence the quaternions) ALONE.  The loss still reaches the geometry through the depth
map (v_depth) and the alpha channel; what it does not have is the gradient of Nr with respect to means, scales and
opacities through w_i.  The replay's transpose uses float atomics, so gradients that pass through it are order dependent
in their last bits, in deterministic mode too.

    img, depth, normals_img, aux = splats.render_normals(camera, (w, h))
    loss = normal_consistency_loss(camera, (w, h), img, depth, normals_img)

`normal_loss_into` is what the trainer uses (TrainConfig.normal_weight): no graph, no upload, no read-back, no
synchronisation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib

# alpha_min = 0.5 reads "mostly covered", as depth_loss's: a hyper-parameter default, not a measured number.
DEFAULT_ALPHA_MIN = 0.5


def workspace_bytes(w: int, h: int) -> int:
    return _lib.size_query("brush_normal_loss_workspace_size", int(w), int(h))


def _uniforms(camera_or_uniforms, img_size=None) -> _lib.BrushUniforms:
    """A BrushUniforms as it is, or the one render.pack_uniforms builds from a Camera and an image size."""
    if isinstance(camera_or_uniforms, _lib.BrushUniforms):
        return camera_or_uniforms
    if img_size is None:
        raise ValueError("a Camera needs img_size=(w, h); only BrushUniforms carry their own")
    from .render import pack_uniforms

    return pack_uniforms(camera_or_uniforms, img_size, 0, 0)


def _check_splat_rows(means, log_scales, quats) -> int:
    for name, t, k in (("means", means, 3), ("log_scales", log_scales, 3), ("quats", quats, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != k or t.dtype != torch.float32:
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else repr(t)
            raise ValueError(f"{name} must be a float32 [N,{k}] tensor, got {got}")
    n = int(means.shape[0])
    if int(log_scales.shape[0]) != n or int(quats.shape[0]) != n:
        raise ValueError(f"means, log_scales and quats must have the same number of rows, got {n}, "
                         f"{int(log_scales.shape[0])} and {int(quats.shape[0])}")
    for name, t in (("means", means), ("log_scales", log_scales), ("quats", quats)):
        if not t.is_cuda or t.device != means.device:
            raise ValueError(f"brush_amd has no CPU path: {name} must live on the GPU, with the others")
    return n


def splat_normals_from(uniforms, means, log_scales, quats, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bare kernel: brush_splat_normals on contiguous float32 device tensors, into `out` [N,3] or a fresh tensor.
    Runs on the current stream; does not synchronise; carries no autograd history."""
    n = int(means.shape[0])
    dev = means.device
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_splat_normals(C.byref(uniforms), means.data_ptr(), log_scales.data_ptr(),
                                                  quats.data_ptr(), n, out.data_ptr(), _lib.current_stream(dev)),
                   "brush_splat_normals")
    return out


def splat_normals_backward_into(uniforms, means, log_scales, quats, v_normals, v_quats) -> torch.Tensor:
    """The bare VJP: brush_splat_normals_backward ADDS the gradient at `quats` into v_quats [N,4] (contiguous float32,
    the convention of the render backward's v_quats).  Runs on the current stream; does not synchronise."""
    n = int(means.shape[0])
    dev = means.device
    if tuple(v_normals.shape) != (n, 3) or tuple(v_quats.shape) != (n, 4) or not v_normals.is_contiguous() \
            or not v_quats.is_contiguous() or v_normals.dtype != torch.float32 or v_quats.dtype != torch.float32:
        raise ValueError(f"v_normals must be contiguous float32 [{n},3] and v_quats contiguous float32 [{n},4]")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_splat_normals_backward(C.byref(uniforms), means.data_ptr(), log_scales.data_ptr(),
                                                           quats.data_ptr(), n, v_normals.data_ptr(),
                                                           v_quats.data_ptr(), _lib.current_stream(dev)),
                   "brush_splat_normals_backward")
    return v_quats


class _SplatNormalsFn(torch.autograd.Function):
    """normals = brush_splat_normals(quats); backward: its VJP into a zeroed [N,4]."""

    @staticmethod
    def forward(ctx, quats, means, log_scales, uniforms):
        q = quats.detach().contiguous()
        ctx.uniforms = uniforms
        ctx.save_for_backward(means, log_scales, q)
        return splat_normals_from(uniforms, means, log_scales, q)

    @staticmethod
    def backward(ctx, v_normals):
        means, log_scales, q = ctx.saved_tensors
        v_quats = torch.zeros_like(q)
        splat_normals_backward_into(ctx.uniforms, means, log_scales, q, v_normals.to(torch.float32).contiguous(),
                                    v_quats)
        return v_quats, None, None, None


def splat_normals(camera_or_uniforms, means, log_scales, quats) -> torch.Tensor:
    """float32 [N,3]: per splat its shortest axis (the lowest index among equal log-scales) in camera space, turned
    towards the camera; every row is written, for splats no view would show too.  `camera_or_uniforms`: the
    BrushUniforms of a forward (render._forward_impl's third result), or a Camera (only its world-to-camera matrix is
    read).  `quats` must be the unit quaternions the forward is fed.
    Differentiable with respect to `quats` ONLY: the choice of the axis and of the sign are piecewise constant, so
    nothing reaches the log-scales or the means (as in 2DGS)."""
    n = _check_splat_rows(means, log_scales, quats)
    u = _uniforms(camera_or_uniforms, (1, 1))  # (the frame is not read)
    if n == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=means.device)
    return _SplatNormalsFn.apply(quats, means.detach().contiguous(), log_scales.detach().contiguous(), u)


def _check_frame(uniforms, pred, depth, normals_img):
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or pred.shape[2] != 4 or pred.dtype != torch.float32:
        got = f"{pred.dtype} {tuple(pred.shape)}" if isinstance(pred, torch.Tensor) else repr(pred)
        raise ValueError(f"pred must be a float32 [h,w,4] tensor, got {got}")
    h, w = int(pred.shape[0]), int(pred.shape[1])
    if (int(uniforms.img_size[0]), int(uniforms.img_size[1])) != (w, h):
        raise ValueError(f"pred is {w}x{h} but the uniforms describe a {int(uniforms.img_size[0])}x"
                         f"{int(uniforms.img_size[1])} frame")
    assert pred.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    dev = pred.device
    if not isinstance(depth, torch.Tensor) or tuple(depth.shape) != (h, w) or depth.dtype != torch.float32 \
            or depth.device != dev:
        raise ValueError(f"depth must be a float32 [h,w] = {(h, w)} tensor on pred's device")
    if normals_img is not None and (not isinstance(normals_img, torch.Tensor) or tuple(normals_img.shape) != (h, w, 3)
                                    or normals_img.dtype != torch.float32 or normals_img.device != dev):
        raise ValueError(f"normals_img must be a float32 [h,w,3] = {(h, w, 3)} tensor on pred's device")
    return h, w, dev


def _check_alpha_min(alpha_min):
    if not float(alpha_min) > 0.0:  # (a NaN fails too)
        raise ValueError(f"alpha_min must be > 0, got {alpha_min}")
    return float(alpha_min)


def _workspace(workspace, w, h, dev):
    nbytes = workspace_bytes(w, h)
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if workspace.numel() * workspace.element_size() < nbytes or workspace.device != dev:
        raise ValueError(f"workspace must hold {nbytes} bytes on pred's device")
    return workspace


def normal_loss_into(uniforms, pred: torch.Tensor, depth: torch.Tensor, normals_img: torch.Tensor,
                     v_pred: Optional[torch.Tensor], *, weight: float = 1.0, alpha_min: float = DEFAULT_ALPHA_MIN,
                     loss_accum: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                     v_depth_accum: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """brush_normal_loss on one render: returns (v_depth [h,w], v_normals_img [h,w,3], stats [2] = {loss, valid
    fraction}), all float32 on the device.  The twin of depth_loss_into: no graph, no upload, no read-back, no
    synchronisation.

    uniforms: the BrushUniforms of the forward (focal, pixel centre and frame size are read).  pred: [h,w,4] float32,
    the raw render; depth: [h,w] float32, its accumulated depth; normals_img: [h,w,3] float32, the replay of the
    per-splat normals on the same forward.  v_pred: None, or the contiguous [h,w,4] float32 gradient image the colour
    loss has written: the term's alpha gradient is added into its alpha channel in place (pixels that receive none
    keep their bits).  loss_accum: optional float32 [1] device tensor that receives `+= loss`.  v_depth_accum: optional
    contiguous float32 [h,w] tensor (another term's depth gradient): this term's is added into it and it is what comes
    back as v_depth, so a step has one depth gradient.  workspace: optional uint8 device tensor of
    workspace_bytes(w, h) bytes."""
    h, w, dev = _check_frame(uniforms, pred, depth, normals_img)
    if normals_img is None:
        raise ValueError("normal_loss_into needs normals_img (depth_normals is the normals-only form)")
    if v_pred is not None and (tuple(v_pred.shape) != (h, w, 4) or v_pred.dtype != torch.float32
                               or not v_pred.is_contiguous() or v_pred.device != dev):
        raise ValueError("v_pred must be a contiguous float32 [h,w,4] tensor on pred's device (it is updated in place)")
    if loss_accum is not None and (loss_accum.numel() != 1 or loss_accum.dtype != torch.float32
                                   or loss_accum.device != dev):
        raise ValueError("loss_accum must be one float32 word on pred's device")
    if v_depth_accum is not None and (tuple(v_depth_accum.shape) != (h, w) or v_depth_accum.dtype != torch.float32
                                      or not v_depth_accum.is_contiguous() or v_depth_accum.device != dev):
        raise ValueError("v_depth_accum must be a contiguous float32 [h,w] tensor on pred's device")
    cfg = _lib.BrushNormalLoss(float(weight), _check_alpha_min(alpha_min))
    pred, depth, normals_img = pred.contiguous(), depth.contiguous(), normals_img.contiguous()
    workspace = _workspace(workspace, w, h, dev)
    v_depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    v_normals_img = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    stats = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_normal_loss(
            C.byref(uniforms), pred.data_ptr(), depth.data_ptr(), normals_img.data_ptr(), C.byref(cfg),
            None, v_depth.data_ptr(), v_normals_img.data_ptr(), None if v_pred is None else v_pred.data_ptr(), stats.data_ptr(),
            None if loss_accum is None else loss_accum.data_ptr(), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), _lib.current_stream(dev)), "brush_normal_loss")
    if v_depth_accum is not None:
        v_depth = v_depth_accum.add_(v_depth)
    return v_depth, v_normals_img, stats


def depth_normals(camera, img_size, img: torch.Tensor, depth: torch.Tensor, *,
                  alpha_min: float = DEFAULT_ALPHA_MIN) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normals [h,w,3] float32, valid fraction, a 0-dim float32 device tensor): the camera-space normals of the surface
    a render's depth map implies (the normals-only form of brush_normal_loss), zeros where a pixel is not valid (the
    module's docstring).  img, depth: the two outputs of render_splats_depth.  `camera`: a Camera with
    img_size = (w, h), or the BrushUniforms of the forward.  No autograd."""
    u = _uniforms(camera, img_size)
    with torch.no_grad():
        img, depth = img.detach(), depth.detach()
        h, w, dev = _check_frame(u, img, depth, None)
        cfg = _lib.BrushNormalLoss(0.0, _check_alpha_min(alpha_min))
        img, depth = img.contiguous(), depth.contiguous()
        workspace = _workspace(None, w, h, dev)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().brush_normal_loss(
                C.byref(u), img.data_ptr(), depth.data_ptr(), None, C.byref(cfg), out.data_ptr(), None, None, None,
                stats.data_ptr(), None, workspace.data_ptr(), workspace.numel(), _lib.current_stream(dev)),
                "brush_normal_loss")
    return out, stats[1]


class _NormalLoss(torch.autograd.Function):
    """The kernel's three gradients are formed in the forward pass (the loss is linear in the incoming scalar) and
    scaled by it in the backward pass, as _DepthLoss does."""

    @staticmethod
    def forward(ctx, img, depth, normals_img, uniforms, weight, alpha_min):
        img_c = img.detach()
        v_img = torch.zeros_like(img_c, memory_format=torch.contiguous_format)
        v_depth, v_normals, stats = normal_loss_into(uniforms, img_c, depth.detach(), normals_img.detach(), v_img,
                                                     weight=weight, alpha_min=alpha_min)
        ctx.save_for_backward(v_img, v_depth, v_normals)
        return stats[0]

    @staticmethod
    def backward(ctx, v_loss):
        v_img, v_depth, v_normals = ctx.saved_tensors
        return v_img * v_loss, v_depth * v_loss, v_normals * v_loss, None, None, None


def normal_consistency_loss(camera, img_size, img: torch.Tensor, depth: torch.Tensor, normals_img: torch.Tensor, *,
                            weight: float = 1.0, alpha_min: float = DEFAULT_ALPHA_MIN) -> torch.Tensor:
    """The depth-normal consistency loss of a render as a differentiable scalar (a 0-dim float32 device tensor).

    img, depth, normals_img: the first three results of render_normals ([h,w,4], [h,w], [h,w,3] float32).  `camera`: a
    Camera with img_size = (w, h), or the BrushUniforms of the forward.  Gradients flow to img's alpha channel, to depth
    and to normals_img."""
    u = _uniforms(camera, img_size)
    return _NormalLoss.apply(img, depth, normals_img, u, float(weight), float(alpha_min))


def render_normals(camera, img_size, means, log_scales, quats, sh_coeffs, raw_opacity, *, antialiased: bool = False,
                   max_intersects: Optional[int] = None):
    """One render_splats_depth WITH autograd, plus splat_normals, plus the feature replay on THAT forward's aux and
    uniforms: (img [h,w,4], depth [h,w], normals_img [h,w,3], aux).  img and depth are bitwise render_splats_depth's and
    differentiable as there.

    THE BLENDING WEIGHTS ARE FROZEN in normals_img, as loudly as render_features says it: normals_img is differentiable
    with respect to `quats` through the per-splat normals ONLY; NO gradient reaches means, log_scales, sh_coeffs or
    raw_opacity through it (they receive theirs through img and depth).  Its backward is the replay's float transpose:
    order dependent in its last bits.  normals_img is not normalised: its length is the alpha-weighted agreement of
    the splats' normals; divide by it where alpha is large for a unit map.  `quats` must be unit quaternions, as for
    render_splats."""
    from . import render as R
    from .features import _FeatureImageFn

    R._check_inputs(means, None, log_scales, quats, sh_coeffs, raw_opacity)
    (img, depth), holder = R._render_op(camera, img_size, means, None, log_scales, quats, sh_coeffs, raw_opacity,
                                        max_intersects=max_intersects, antialiased=antialiased, depth=True)
    aux, u = holder["aux"], holder["uniforms"]
    normals = splat_normals(u, means, log_scales, quats)
    if means.shape[0] == 0:
        h, w = int(u.img_size[1]), int(u.img_size[0])
        return img, depth, torch.zeros((h, w, 3), dtype=torch.float32, device=means.device), aux
    normals_img = _FeatureImageFn.apply(normals, (u, aux))
    return img, depth, normals_img, aux
