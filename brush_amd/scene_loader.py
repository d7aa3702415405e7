"""SceneLoader — crates/brush-dataset/src/scene_loader.rs, reshaped for a dataset that lives on the device.

The reference spawns a task that picks `rng.gen_range(0..len)` views, turns each view's u8 image into f32 on the host
(`image_to_tensor`) and uploads it, five batches ahead of the trainer.  Here every training image is uploaded once, at
construction, as the u8 it was decoded as (alpha kept when present, as image_to_tensor keeps it); the loss kernels read
u8 directly (brush_l1_ssim_loss_gt).  `next_batch` then only draws an index: no host<->device traffic, no
synchronisation and nothing left for a prefetch thread to do.  Batch size is 1, as the reference asserts
(train.rs:216-219).  A view's depth map (build extension, SceneView.depth) is uploaded the same way, once and in the
dtype it is stored in; brush_depth_loss reads uint16 and float32 directly.  `set_downscale` (build extension) makes the
loader hand out every view at 1 / factor, resized on the device from the resident copies (brush_amd/pyramid.py).
A view's loss mask (build extension, SceneView.mask) is uploaded once as u8; where such a view also has a depth map, the
resident depth copy is zeroed under the mask at load: a raw 0 already means "no measurement" to brush_depth_loss, so the
depth term skips masked pixels with no kernel of its own.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch


def scene_extent(scene) -> float:
    """`scene.bounds(0.0, 0.0).extent.max_element()` (scene_loader.rs:22): the largest half-size of the box around the
    training cameras (BoundingBox::extent is the half-size, bounding_box.rs:11)."""
    lo, hi = scene.bounds(0.0, 0.0)
    return float(np.max((np.asarray(hi, dtype=np.float32) - np.asarray(lo, dtype=np.float32)) / np.float32(2.0)))


class SceneLoader:
    """Uniform random training views of `scene` (a dataset.Scene) with their images resident on `device`.

    `seed` seeds a numpy Generator; view i of the sequence is `rng.integers(0, len(views))` (the reference's
    `rng.gen_range(0..len)` on a StdRng, whose bits numpy does not reproduce)."""

    def __init__(self, scene, seed: int = 42, device=None, batch_size: int = 1, use_masks: bool = True):
        if batch_size != 1:
            raise ValueError("only a batch size of 1 is supported (as the reference, train.rs:216-219)")
        if not scene.views:
            raise ValueError("the scene has no views to train on")
        self.scene = scene
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.scene_extent = scene_extent(scene)
        self.rng = np.random.default_rng(seed)
        self.images = []
        self.depths = []  # parallel to images: the view's depth map as stored (uint16 / float32 [h,w]), or None
        self.masks = []   # parallel to images: the view's loss mask (uint8 [h,w], nonzero = keep), or None
        for v in scene.views:
            img = np.require(v.image, requirements=["C"])
            if img.ndim != 3 or img.dtype != np.uint8 or img.shape[2] not in (3, 4):
                raise ValueError(f"{v.name}: the view's image must be uint8 [h,w,3|4], got {img.dtype} {img.shape}")
            self.images.append(torch.from_numpy(np.array(img, copy=True)).to(self.device))  # the one upload
            mask = getattr(v, "mask", None) if use_masks else None
            if mask is not None and (mask.dtype != np.uint8 or tuple(mask.shape) != tuple(img.shape[:2])):
                raise ValueError(f"{v.name}: the view's mask must be uint8 [h,w] = {tuple(img.shape[:2])}, got "
                                 f"{mask.dtype} {mask.shape}")
            depth = getattr(v, "depth", None)
            if depth is not None:
                if depth.dtype not in (np.uint16, np.float32) or tuple(depth.shape) != tuple(img.shape[:2]):
                    raise ValueError(f"{v.name}: the view's depth map must be uint16 or float32 [h,w] = "
                                     f"{tuple(img.shape[:2])}, got {depth.dtype} {depth.shape}")
                depth = np.array(depth, copy=True, order="C")
                if mask is not None:  # 0 = no measurement: the depth term leaves the masked pixels out
                    depth[mask == 0] = 0
                depth = torch.from_numpy(depth).to(self.device)  # as stored, once
            if mask is not None:
                mask = torch.from_numpy(np.array(mask, copy=True, order="C")).to(self.device)  # once
            self.depths.append(depth)
            self.masks.append(mask)
        self.total_bytes = int(sum(t.numel() * t.element_size() for t in self.images + self.depths + self.masks
                                   if t is not None))
        # the level next_batch / next_indexed / depth hand out: at factor 1 the uploaded tensors themselves
        self.downscale = 1
        self.level_bytes = 0
        self._images, self._depths, self._masks = self.images, self.depths, self.masks

    def __len__(self) -> int:
        return len(self.images)

    def set_downscale(self, factor: int) -> None:
        """Hands out every view at 1 / factor from now on (coarse-to-fine training): the image through
        pyramid.area_resize and the depth map and the mask, where the view has one, through pyramid.nearest_resize, each
        to pyramid.downscaled_size of that view's own size.  The previous level is dropped first; factor 1 goes back to the
        uploaded tensors and holds nothing.  Launches on the current stream and nothing else: no read-back, no
        synchronisation.  `level_bytes` is what the level holds beside `total_bytes`.  The random draw does not depend
        on the factor."""
        from .pyramid import area_resize, check_factor, nearest_resize

        factor = check_factor(factor)
        self._images, self._depths, self._masks = self.images, self.depths, self.masks  # drops the previous level
        self.downscale, self.level_bytes = 1, 0
        if factor == 1:
            return
        self._images = [area_resize(t, factor=factor) for t in self.images]
        self._depths = [None if t is None else nearest_resize(t, factor=factor) for t in self.depths]
        # a mask is resized like a depth map (never blended); nearest_resize moves 2- and 4-byte elements
        self._masks = [None if t is None else nearest_resize(t.to(torch.int16).view(torch.uint16),
                                                             factor=factor).view(torch.int16).to(torch.uint8)
                       for t in self.masks]
        self.downscale = factor
        self.level_bytes = int(sum(t.numel() * t.element_size() for t in self._images + self._depths + self._masks
                                   if t is not None))

    def next_index(self) -> int:
        return int(self.rng.integers(0, len(self.images)))

    def depth(self, i: int) -> Optional[torch.Tensor]:
        """View i's depth map on the device (uint16 or float32 [h,w], as stored; the view's depth_scale / depth_offset
        turn it into scene units), or None when the view has none.  At the current level's size."""
        return self._depths[i]

    def mask(self, i: int) -> Optional[torch.Tensor]:
        """View i's loss mask on the device (uint8 [h,w], nonzero = keep), or None when the view has none (or the
        loader was built with use_masks=False).  At the current level's size."""
        return self._masks[i]

    def view_at(self, i: int) -> Tuple[object, torch.Tensor, Optional[torch.Tensor]]:
        """(view i's Camera, its image, its loss mask or None) as resident on the device at the current level, without a
        draw: the rng is not touched."""
        return self.scene.views[i].camera, self._images[i], self._masks[i]

    def next_batch(self) -> Tuple[object, torch.Tensor]:
        """(SceneView, its image as a uint8 [h,w,3|4] device tensor)."""
        _, view, image = self.next_indexed()
        return view, image

    def next_indexed(self) -> Tuple[int, object, torch.Tensor]:
        """next_batch with the drawn view's index in scene.views in front (the same draw from the same rng)."""
        i = self.next_index()
        return i, self.scene.views[i], self._images[i]
