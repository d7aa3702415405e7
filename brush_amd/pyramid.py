"""Device image pyramids: smaller copies of the resident training images, made where the images live.

Coarse-to-fine training (nerfstudio's `num_downscales` / `resolution_schedule`) and multi-scale evaluation
(Mip-Splatting's protocol: score at 1, 1/2, 1/4, 1/8) both need a view's image at a fraction of its stored size.
Everything above the images takes its size from the target it is handed, so the one piece needed is the resize itself,
on the device (a host resize and a second upload would undo the resident loader):

    area_resize     uint8 [h,w,3|4] images: an exact area (box) filter, defined in integers with one rounding
                    (include/brush_hip.h: brush_area_resize_u8; brush_amd/csrc/resize.hip)
    nearest_resize  uint16 / float32 [h,w] depth maps: dataset.resize_nearest bit for bit (brush_nearest_resize), so
                    a "no measurement" zero never blends into its neighbours

Both return a new tensor, on the current stream, without a read-back or a synchronisation.  `downscaled_size` is the
size of a level: (w + factor // 2) // factor per side, at least 1.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

MAX_FACTOR = 16
MAX_SIDE = 16384


def check_factor(factor) -> int:
    """`factor` as an int in 1..MAX_FACTOR, or a ValueError."""
    if isinstance(factor, bool) or int(factor) != factor or not 1 <= int(factor) <= MAX_FACTOR:
        raise ValueError(f"a downscale factor must be an integer from 1 to {MAX_FACTOR}, got {factor!r}")
    return int(factor)


def downscaled_size(w: int, h: int, factor: int) -> Tuple[int, int]:
    """(ow, oh) of a [h,w] image at 1 / factor: each side divided by the factor and rounded half up, at least 1."""
    f = check_factor(factor)
    if int(w) < 1 or int(h) < 1:
        raise ValueError(f"the size must be positive, got {(w, h)}")
    return max(1, (int(w) + f // 2) // f), max(1, (int(h) + f // 2) // f)


def _target_size(w: int, h: int, size, factor) -> Tuple[int, int]:
    if (size is None) == (factor is None):
        raise ValueError("give exactly one of `size` (ow, oh) and `factor`")
    if w < 1 or h < 1 or w > MAX_SIDE or h > MAX_SIDE:
        raise ValueError(f"the source must be 1..{MAX_SIDE} pixels on each side, got {(w, h)}")
    if factor is not None:
        return downscaled_size(w, h, factor)
    ow, oh = int(size[0]), int(size[1])
    if not (1 <= ow <= w and 1 <= oh <= h):
        raise ValueError(f"the output size (ow, oh) = {(ow, oh)} must be within 1..(w, h) = {(w, h)}: these resizes "
                         "only shrink")
    return ow, oh


def area_resize(image: torch.Tensor, size: Optional[Tuple[int, int]] = None, *,
                factor: Optional[int] = None) -> torch.Tensor:
    """`image`, a uint8 [h,w,3|4] device tensor, area-filtered to `size` = (ow, oh) or to
    downscaled_size(w, h, factor): a new contiguous uint8 [oh,ow,c] tensor (brush_area_resize_u8: every channel on its
    own, exact integer weights, one rounding).  Runs on the current stream; does not synchronise."""
    assert image.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if image.dim() != 3 or image.dtype != torch.uint8 or image.shape[2] not in (3, 4):
        raise ValueError(f"image must be a uint8 [h,w,3|4] tensor, got {image.dtype} {tuple(image.shape)}")
    h, w, c = (int(x) for x in image.shape)
    ow, oh = _target_size(w, h, size, factor)
    image = image.contiguous()
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=image.device)
    with torch.cuda.device(image.device):
        _lib.check(_lib.lib().brush_area_resize_u8(image.data_ptr(), w, h, c, out.data_ptr(), ow, oh,
                                                   _lib.current_stream(image.device)),
                   "brush_area_resize_u8")
    return out


def nearest_resize(t: torch.Tensor, size: Optional[Tuple[int, int]] = None, *,
                   factor: Optional[int] = None) -> torch.Tensor:
    """`t`, a uint16 or float32 [h,w] device tensor (a depth map), to `size` = (ow, oh) or to
    downscaled_size(w, h, factor) by taking the element under each output pixel's centre: dataset.resize_nearest bit for
    bit (brush_nearest_resize).  Runs on the current stream; does not synchronise."""
    assert t.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if t.dim() != 2 or t.dtype not in (torch.uint16, torch.float32):
        raise ValueError(f"t must be a uint16 or float32 [h,w] tensor, got {t.dtype} {tuple(t.shape)}")
    h, w = int(t.shape[0]), int(t.shape[1])
    ow, oh = _target_size(w, h, size, factor)
    t = t.contiguous()
    out = torch.empty((oh, ow), dtype=t.dtype, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().brush_nearest_resize(t.data_ptr(), t.element_size(), w, h, out.data_ptr(), ow, oh,
                                                   _lib.current_stream(t.device)),
                   "brush_nearest_resize")
    return out
