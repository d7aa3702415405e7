"""SceneLoader — crates/brush-dataset/src/scene_loader.rs, reshaped for a dataset that lives on the device.

The reference spawns a task that picks `rng.gen_range(0..len)` views, turns each view's u8 image into f32 on the host
(`image_to_tensor`) and uploads it, five batches ahead of the trainer.  Here every training image is uploaded once, at
construction, as the u8 it was decoded as (alpha kept when present, as image_to_tensor keeps it); the loss kernels read
u8 directly (brush_l1_ssim_loss_gt).  `next_batch` then only draws an index: no host<->device traffic, no
synchronisation and nothing left for a prefetch thread to do.  Batch size is 1, as the reference asserts
(train.rs:216-219).
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

    def __init__(self, scene, seed: int = 42, device=None, batch_size: int = 1):
        if batch_size != 1:
            raise ValueError("only a batch size of 1 is supported (as the reference, train.rs:216-219)")
        if not scene.views:
            raise ValueError("the scene has no views to train on")
        self.scene = scene
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.scene_extent = scene_extent(scene)
        self.rng = np.random.default_rng(seed)
        self.images = []
        for v in scene.views:
            img = np.require(v.image, requirements=["C"])
            if img.ndim != 3 or img.dtype != np.uint8 or img.shape[2] not in (3, 4):
                raise ValueError(f"{v.name}: the view's image must be uint8 [h,w,3|4], got {img.dtype} {img.shape}")
            self.images.append(torch.from_numpy(np.array(img, copy=True)).to(self.device))  # the one upload
        self.total_bytes = int(sum(t.numel() * t.element_size() for t in self.images))

    def __len__(self) -> int:
        return len(self.images)

    def next_index(self) -> int:
        return int(self.rng.integers(0, len(self.images)))

    def next_batch(self) -> Tuple[object, torch.Tensor]:
        """(SceneView, its image as a uint8 [h,w,3|4] device tensor)."""
        _, view, image = self.next_indexed()
        return view, image

    def next_indexed(self) -> Tuple[int, object, torch.Tensor]:
        """next_batch with the drawn view's index in scene.views in front (the same draw from the same rng)."""
        i = self.next_index()
        return i, self.scene.views[i], self.images[i]
