"""Per-splat feature vectors through the compositing walk, both ways (build extension; gsplat's N-channel rasterisation
is the model, LangSplat, Feature-3DGS, Gaussian Grouping and FlashSplat are the uses).

A finished forward leaves its tile lists in the aux; three replays of its compositing walk (include/brush_hip.h,
csrc/features.hip) use them:

    brush_render_features           out[p,c]  = sum over the splats g the forward added to pixel p of fac f[g,c]
    brush_render_features_backward  v_f[g,c] += sum over those pixels of fac v[p,c]          (float atomics)
    brush_render_feature_sums       sums[g,c] += sum over those pixels of rint(fac m[p,c] 2^24)   (exact integers)

with fac = alpha T the blending weight the forward added the splat with.  THE GEOMETRY IS FROZEN: nothing here produces
a gradient for means, scales, rotations, opacities or colours; a feature image is differentiable with respect to the
features alone.

    img, feat, aux = splats.render_features(camera, (w, h), features)       # feat [h,w,C], d feat / d features
    sums = splat_feature_sums(splats, scene.views, maps)                    # launches only
    labels, sums = lift_labels(splats, scene.views, label_maps, num_classes=K)
    obj = splats.select(labels == 3)

The float transpose is order dependent in its last bits (atomics); the integer sums are order independent, so the same
views give the same bits on every run, in both aux modes.  Also `python -m brush_amd.lift`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .render import check_tensor

Q24 = float(1 << 24)  # the fixed point of a sum (brush_render_feature_sums)
MAX_CHANNELS = 64     # BRUSH_FEATURE_MAX_CHANNELS
MAP_F32, MAP_LABEL_U8 = 0, 1  # BRUSH_FEATURE_MAP_*
IGNORE_LABEL = 255


def _frame(uniforms):
    return int(uniforms.img_size[1]), int(uniforms.img_size[0])


def _check_channels(c) -> int:
    if not (1 <= int(c) <= MAX_CHANNELS):
        raise ValueError(f"the channel count must be in [1, {MAX_CHANNELS}], got {int(c)}")
    return int(c)


def _check_rows(t, dtype, what: str, dev=None) -> int:
    """`t` as a contiguous [N,C] device tensor of `dtype`; returns C."""
    if (not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != dtype or not t.is_contiguous()
            or t.device.type != "cuda" or (dev is not None and t.device != dev)):
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f"{what} must be a contiguous {dtype} [N,C] tensor on the GPU, got {got}")
    return _check_channels(t.shape[1])


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def features_from_aux(uniforms, aux, features: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bare forward replay: composites `features` (contiguous float32 [N,C], rows indexed by global splat id,
    1 <= C <= 64) over the finished forward (`uniforms`, `aux`: what render._forward_impl returned) into a float32
    [h,w,C] tensor (`out`, or a fresh one).  Every pixel and channel is written, zeros where nothing was added.  Bitwise
    repeatable.  Runs on the current stream; does not synchronise; carries no autograd history."""
    c = _check_rows(features, torch.float32, "features")
    dev = features.device
    h, w = _frame(uniforms)
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.float32, device=dev)
    else:
        check_tensor(out, torch.float32, (h, w, c), "out", dev)
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_features(C.byref(uniforms), C.byref(s), _ptr(features), c, out.data_ptr(),
                                                    int(features.shape[0]), _lib.current_stream(dev)),
                   "brush_render_features")
    return out


def feature_grads_from_aux(uniforms, aux, v_out: torch.Tensor, v_features: torch.Tensor) -> torch.Tensor:
    """The bare transpose: v_features[g,c] += sum over the pixels the forward added g to of fac v_out[p,c].  v_out:
    contiguous float32 [h,w,C]; v_features: contiguous float32 [N,C], ACCUMULATED into (zero it for a gradient).  Float
    atomics: the last bits depend on the order the waves arrive in.  Runs on the current stream; does not
    synchronise."""
    c = _check_rows(v_features, torch.float32, "v_features")
    dev = v_features.device
    h, w = _frame(uniforms)
    check_tensor(v_out, torch.float32, (h, w, c), "v_out", dev)
    if v_features.shape[0] == 0:
        return v_features
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_features_backward(C.byref(uniforms), C.byref(s), v_out.data_ptr(), c,
                                                             v_features.data_ptr(), int(v_features.shape[0]),
                                                             _lib.current_stream(dev)),
                   "brush_render_features_backward")
    return v_features


def feature_sums_from_aux(uniforms, aux, maps_or_labels: torch.Tensor, sums: torch.Tensor) -> torch.Tensor:
    """The bare exact transpose: sums[g,c] += sum over the pixels the forward added g to of rint(fac m[p,c] 2^24).
    sums: contiguous int64 [N,C], ACCUMULATED into.  maps_or_labels: a contiguous float32 [h,w,C] map (values are clamped
    to [0, 1], a NaN counts as 0) or a contiguous uint8 [h,w] label image, whose channel c is `label == c` (a label >= C
    belongs to no class).  Order independent: bitwise repeatable.  Runs on the current stream; does not synchronise."""
    c = _check_rows(sums, torch.int64, "sums")
    dev = sums.device
    h, w = _frame(uniforms)
    m = maps_or_labels
    if isinstance(m, torch.Tensor) and m.dtype == torch.uint8:
        check_tensor(m, torch.uint8, (h, w), "a label image", dev)
        kind = MAP_LABEL_U8
    else:
        check_tensor(m, torch.float32, (h, w, c), "maps", dev)
        kind = MAP_F32
    if sums.shape[0] == 0:
        return sums
    s = aux._as_struct()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_render_feature_sums(C.byref(uniforms), C.byref(s), m.data_ptr(), kind, c,
                                                        sums.data_ptr(), int(sums.shape[0]), _lib.current_stream(dev)),
                   "brush_render_feature_sums")
    return sums


class _FeatureImageFn(torch.autograd.Function):
    """feat = features_from_aux(features); backward: the float transpose into a zeroed tensor."""

    @staticmethod
    def forward(ctx, features, holder):
        u, aux = holder
        ctx.holder = holder
        ctx.shape = tuple(features.shape)
        return features_from_aux(u, aux, features.detach().contiguous())

    @staticmethod
    def backward(ctx, v_feat):
        u, aux = ctx.holder
        v_features = torch.zeros(ctx.shape, dtype=torch.float32, device=v_feat.device)
        feature_grads_from_aux(u, aux, v_feat.contiguous(), v_features)
        return v_features, None


def render_features(camera, img_size, means, log_scales, quats, sh_coeffs, raw_opacity, features, *,
                    antialiased: bool = False, max_intersects: Optional[int] = None):
    """One forward WITHOUT autograd plus the replay: (img [h,w,4], feat [h,w,C], aux).  `features`: float32 [N,C],
    1 <= C <= 64.  The geometry is frozen: feat is differentiable with respect to `features` ONLY (its backward is the
    float transpose, order dependent in its last bits); no gradient reaches means, log_scales, quats, sh_coeffs or
    raw_opacity, and img comes back detached.  `quats` must be unit quaternions, as for render_splats."""
    from . import render as R

    n = R._check_inputs(means, None, log_scales, quats, sh_coeffs, raw_opacity)
    if (not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != n
            or features.dtype != torch.float32 or features.device != means.device):
        got = f"{features.dtype} {tuple(features.shape)}" if isinstance(features, torch.Tensor) else repr(features)
        raise ValueError(f"features must be a float32 [{n},C] tensor on the splats' device, got {got}")
    _check_channels(features.shape[1])
    with torch.no_grad():
        img, aux, u = R._forward_impl(camera, img_size, means.detach(), log_scales.detach(), quats.detach(),
                                      sh_coeffs.detach(), raw_opacity.detach(), False, max_intersects,
                                      expect_backward=False, antialiased=antialiased)
    feat = _FeatureImageFn.apply(features, (u, aux))
    return img, feat, aux


# ---- lifting 2D maps onto the splats ------------------------------------------------------------------------------------
@dataclass
class FeatureSums:
    """Per-splat sums of maps over views, exact integers in units of 2^-24 "pixels of full weight".
    sum: int64 [N,C], the summed fac m per channel; weight: int64 [N], the summed fac (of the pixels no mask ruled
    out).  Device tensors as splat_feature_sums returns them; read() gives the CPU copy."""
    sum: torch.Tensor
    weight: torch.Tensor
    views: int = 0

    def mean(self) -> torch.Tensor:
        """float32 [N,C] = sum / weight, 0 where weight == 0; stays on the tensors' device, nothing is read back."""
        w = self.weight.to(torch.float64).unsqueeze(1)
        m = self.sum.to(torch.float64) / torch.where(w == 0, torch.ones_like(w), w)
        return torch.where(w == 0, torch.zeros_like(m), m).to(torch.float32)

    def read(self) -> "FeatureSums":
        """The one read-back (synchronises): the same sums as CPU tensors."""
        return FeatureSums(self.sum.cpu(), self.weight.cpu(), self.views)


def labels_from_sums(sums: torch.Tensor, min_weight: float = 0.0) -> torch.Tensor:
    """int32 [N]: per row of the int64 [N,C] class sums the class with the largest sum, the LOWEST class among equals,
    and -1 where no class received weight above `min_weight` (in pixels of full weight; the sums are in units of
    2^-24).  Pure torch on the sums' device; works on CPU tensors."""
    mw = float(min_weight)
    if not (mw >= 0.0):  # (a NaN fails too)
        raise ValueError(f"min_weight must be >= 0, got {min_weight!r}")
    if sums.dim() != 2 or sums.dtype != torch.int64:
        raise ValueError(f"sums must be int64 [N,C], got {sums.dtype} {tuple(sums.shape)}")
    n, c = sums.shape
    if c == 0 or n == 0:
        return torch.full((n,), -1, dtype=torch.int32, device=sums.device)
    best = sums.max(dim=1, keepdim=True).values
    classes = torch.arange(c, dtype=torch.int64, device=sums.device).expand(n, c)
    first = torch.where(sums == best, classes, torch.full_like(classes, c)).min(dim=1).values
    none = best.squeeze(1).to(torch.float64) <= mw * Q24
    return torch.where(none, torch.full_like(first, -1), first).to(torch.int32)


def _device_map(m, dev, num_classes):
    """One view's map on the device: (float32 [h,w,C], None) or (None, uint8 [h,w] labels)."""
    import numpy as np

    if not isinstance(m, torch.Tensor):
        m = torch.from_numpy(np.array(m, copy=True, order="C"))
    m = m.to(dev)
    if m.dtype == torch.uint8 and m.dim() == 2:
        if num_classes is None:
            raise ValueError("a uint8 [h,w] label map needs num_classes=")
        return None, m.contiguous()
    if num_classes is not None:
        raise ValueError(f"num_classes= goes with uint8 [h,w] label maps, got {m.dtype} {tuple(m.shape)}")
    if m.dim() != 3 or m.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"a map must be float32 [h,w,C], uint8 [h,w,C] or uint8 [h,w] labels, got {m.dtype} "
                         f"{tuple(m.shape)}")
    if m.dtype == torch.uint8:
        m = m.to(torch.float32) / 255.0
    return m.contiguous(), None


def splat_feature_sums(splats, views, maps, *, antialiased: bool = False, use_masks: bool = True,
                       num_classes: Optional[int] = None) -> FeatureSums:
    """The exact per-splat sums of `maps` over `views`, with the geometry frozen.  views: dataset.SceneViews or
    (Camera, gt, mask or None) triples of device tensors, as splat_error_scores takes them (gt is not read); maps: one
    per view, at the size the view is rendered at: a float32 [h,w,C] tensor in [0, 1], a uint8 [h,w,C] tensor read as
    b / 255, or, with num_classes = C, a uint8 [h,w] label tensor whose channel c is `label == c` (labels >= C, 255 among
    them, belong to no class).  1 <= C <= 64.  Per view: one forward, one replay of the map and one of a one-channel
    all-ones map for the weight; pixels a mask rules out count nowhere (map 0, label 255, weight 0).  The splats are
    synchronised once; with device-resident views and maps nothing else synchronises.  Returns the FeatureSums on the
    device (mean() stays there, read() reads back)."""
    from . import render as R

    views, maps = list(views), list(maps)
    if len(views) != len(maps):
        raise ValueError(f"one map per view: {len(views)} views, {len(maps)} maps")
    if num_classes is not None:
        if int(num_classes) > MAX_CHANNELS:
            raise ValueError(f"at most {MAX_CHANNELS} classes per pass, got {int(num_classes)}: remap the labels "
                             f"into [0, {MAX_CHANNELS}) (or lift them in groups)")
        num_classes = _check_channels(num_classes)
    parts = splats.frozen()  # one sync, as Splats.render does per call
    dev = parts[0].device
    n = splats.num_splats()
    sums = weight = None
    with torch.no_grad():
        for view, m in zip(views, maps):
            cam, _, _, mask = R.view_parts(view, dev, mask=use_masks)
            fmap, labels = _device_map(m, dev, num_classes)
            h, w = (int(x) for x in (labels if fmap is None else fmap).shape[:2])
            c = num_classes if fmap is None else _check_channels(fmap.shape[2])
            if sums is None:
                sums = torch.zeros((n, c), dtype=torch.int64, device=dev)
                weight = torch.zeros((n, 1), dtype=torch.int64, device=dev)
            elif sums.shape[1] != c:
                raise ValueError(f"every map must have {sums.shape[1]} channels, got {c}")
            ones = torch.ones((h, w, 1), dtype=torch.float32, device=dev)
            if mask is not None:
                if (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (h, w)
                        or mask.device != dev):
                    raise ValueError(f"a view's mask must be a uint8 {(h, w)} tensor on the splats' device")
                on = mask != 0
                ones = on.to(torch.float32).unsqueeze(2).contiguous()
                if fmap is None:
                    labels = torch.where(on, labels, torch.full_like(labels, IGNORE_LABEL))
                else:
                    fmap = torch.where(on.unsqueeze(2), fmap, torch.zeros_like(fmap))
            _, aux, u = R.forward_frozen(parts, cam, (w, h), antialiased)
            feature_sums_from_aux(u, aux, labels if fmap is None else fmap, sums)
            feature_sums_from_aux(u, aux, ones, weight)
    if sums is None:
        raise ValueError("no views")
    return FeatureSums(sums, weight.squeeze(1), len(views))


def lift_labels(splats, views, label_maps, num_classes: int, *, min_weight: float = 0.0, antialiased: bool = False,
                use_masks: bool = True):
    """Closed-form label transfer (FlashSplat is the model): every splat takes the class whose pixels it contributed the
    most blending weight to over `views`.  label_maps: one uint8 [h,w] image per view, class ids in [0, num_classes),
    anything else (255) unlabelled; num_classes <= 64.  Returns (labels int32 [N] on the device, FeatureSums): the
    lowest class wins a tie; -1 where no class received weight above `min_weight` (in pixels of full weight).  Cut an
    object out with splats.select(labels == k)."""
    if int(num_classes) > MAX_CHANNELS:
        raise ValueError(f"at most {MAX_CHANNELS} classes, got {int(num_classes)}: remap the labels into "
                         f"[0, {MAX_CHANNELS}) (or lift them in groups)")
    sums = splat_feature_sums(splats, views, label_maps, antialiased=antialiased, use_masks=use_masks,
                              num_classes=num_classes)
    return labels_from_sums(sums.sum, min_weight), sums
