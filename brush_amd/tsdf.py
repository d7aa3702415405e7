"""Volumetric fusion of rendered depth: a dense truncated signed distance volume on the device, and the triangle mesh
cut out of it (KinectFusion's fusion; the TSDF mesh exports of 2DGS, GOF and nerfstudio are the models).

    vol = TsdfVolume(origin, voxel_size, (nx, ny, nz))
    vol.integrate_splats(splats, dataset.train.views)      # render_splats_depth per view, fused K views per launch
    mesh = vol.extract_mesh(min_views=2)                   # brush_amd.mesh.Mesh: vertices, colors, faces (host arrays)

Every voxel holds integers (the views that saw it, the sum of their quantised truncated distances, 8-bit colour sums),
and one lane owns a voxel, so a volume's bits depend on neither the order of the views nor on how many go into one
launch, and the mesh arrays are the same on every run.  The kernels are brush_tsdf_integrate / brush_tsdf_mesh_count /
brush_tsdf_mesh_emit (include/brush_hip.h states the arithmetic and the orders; brush_amd/csrc/tsdf.hip).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_SIDE = 2048          # BRUSH_TSDF_MAX_SIDE
MAX_VOXELS = 1 << 28     # BRUSH_TSDF_MAX_VOXELS
PLANES = 6               # BRUSH_TSDF_PLANES: count, sdf_sum, r, g, b, rgb_count
MAX_VIEWS = 16           # BRUSH_TSDF_MAX_VIEWS: views of one launch
SDF_ONE = 32767          # the quantised distance of one truncation length
# Views fused per launch by integrate_splats.  The volume is read and written once per launch, so K views share its
# 48 B per voxel; but the launch is bound by the image gathers, and K images compete for the caches: at 256^3 with 1080p
# views the time per view is lowest at K = 2 (DESIGN.md §8 row 19 holds the measurement).
DEFAULT_VIEWS_PER_LAUNCH = 2


def check_grid(voxel_size, dims):
    """(voxel_size, (nx, ny, nz)) as the kernels take them, or a ValueError that names the limit."""
    voxel_size = float(voxel_size)
    if not (math.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size!r}")
    if len(dims) != 3:
        raise ValueError(f"dims must be (nx, ny, nz), got {dims!r}")
    dims = tuple(int(d) for d in dims)
    if min(dims) < 1 or max(dims) > MAX_SIDE:
        raise ValueError(f"every side of the grid must be in [1, {MAX_SIDE}] voxels, got {dims}")
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"the grid {dims[0]} x {dims[1]} x {dims[2]} has {dims[0] * dims[1] * dims[2]} voxels, over "
                         f"the limit of 2^28 = {MAX_VOXELS}: use a larger voxel or tighter bounds")
    return voxel_size, dims


def _depth_kind_flags(depth_kind) -> int:
    """The flags of brush_tsdf_integrate_ex for TsdfVolume.integrate's `depth_kind`, or a ValueError."""
    if depth_kind == "accumulated":
        return 0
    if depth_kind == "metric":
        return _lib.TSDF_DEPTH_METRIC
    raise ValueError(f"depth_kind must be 'accumulated' or 'metric', got {depth_kind!r}")


@dataclass
class TsdfArrays:
    """TsdfVolume.read(): host arrays indexed [k, j, i] (x fastest).  `sdf`: the mean distance in units of the
    truncation length, in [-1, 1], NaN where no view observed the voxel; `rgb`: the mean colour, 0 where no view gave
    one."""
    count: np.ndarray      # uint32 [nz, ny, nx]
    sdf_sum: np.ndarray    # int32 [nz, ny, nx]
    sdf: np.ndarray        # float32 [nz, ny, nx]
    rgb: np.ndarray        # uint8 [nz, ny, nx, 3]
    rgb_sum: np.ndarray    # uint32 [nz, ny, nx, 3]
    rgb_count: np.ndarray  # uint32 [nz, ny, nx]


class TsdfVolume:
    """A dense grid of nx ny nz voxels, voxel (i, j, k) centred at origin + (idx + 0.5) voxel_size, resident on the
    device as six planes of 32-bit integers (24 bytes per voxel)."""

    def __init__(self, origin, voxel_size, dims, *, trunc: Optional[float] = None, device=None):
        self.voxel_size, self.dims = check_grid(voxel_size, dims)
        origin = tuple(float(x) for x in origin)
        if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        self.origin = origin
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        # the longest edge of the extraction is a cell's body diagonal: a sign change across it must be a crossing of
        # the surface, not the step from "in front" to the unobserved band behind it
        if not (math.isfinite(self.trunc) and self.trunc >= math.sqrt(3.0) * self.voxel_size):
            raise ValueError(f"trunc must be at least sqrt(3) voxels ({math.sqrt(3.0) * self.voxel_size:g}), "
                             f"got {self.trunc!r}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        assert self.device.type == "cuda", "brush_amd has no CPU path: the volume lives on the GPU"
        self.state = torch.zeros((PLANES, self.num_voxels), dtype=torch.int32, device=self.device)
        self.views = 0

    @property
    def num_voxels(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def nbytes(self) -> int:
        return PLANES * 4 * self.num_voxels

    def _grid(self) -> _lib.BrushTsdfGrid:
        g = _lib.BrushTsdfGrid()
        g.origin[:] = self.origin
        g.voxel, g.trunc = self.voxel_size, self.trunc
        g.nx, g.ny, g.nz = self.dims
        return g

    @classmethod
    def from_arrays(cls, origin, voxel_size, count, sdf_sum, rgb_sum=None, rgb_count=None, *,
                    trunc: Optional[float] = None, device=None) -> "TsdfVolume":
        """A volume with the given state: `count` and `sdf_sum` [nz, ny, nx] (x fastest), optionally `rgb_sum`
        [nz, ny, nx, 3] and `rgb_count` [nz, ny, nx] (both or neither; absent: no voxel has a colour)."""
        count = np.asarray(count)
        if count.ndim != 3:
            raise ValueError(f"count must be [nz, ny, nx], got {count.shape}")
        sdf_sum = np.asarray(sdf_sum)
        if sdf_sum.shape != count.shape:
            raise ValueError(f"sdf_sum must have count's shape {count.shape}, got {sdf_sum.shape}")
        if (rgb_sum is None) != (rgb_count is None):
            raise ValueError("rgb_sum and rgb_count go together")
        vol = cls(origin, voxel_size, count.shape[::-1], trunc=trunc, device=device)
        host = np.zeros((PLANES, vol.num_voxels), dtype=np.int32)
        host[0] = count.astype(np.uint32).reshape(-1).view(np.int32)
        host[1] = sdf_sum.astype(np.int32).reshape(-1)
        if rgb_sum is not None:
            rgb_sum, rgb_count = np.asarray(rgb_sum), np.asarray(rgb_count)
            if rgb_sum.shape != count.shape + (3,) or rgb_count.shape != count.shape:
                raise ValueError(f"rgb_sum must be {count.shape + (3,)} and rgb_count {count.shape}, got "
                                 f"{rgb_sum.shape} / {rgb_count.shape}")
            host[2:5] = rgb_sum.astype(np.uint32).reshape(-1, 3).T.view(np.int32)
            host[5] = rgb_count.astype(np.uint32).reshape(-1).view(np.int32)
        vol.state.copy_(torch.from_numpy(host))
        return vol

    def read(self) -> TsdfArrays:
        """The volume on the host (one copy, one synchronisation)."""
        nx, ny, nz = self.dims
        host = self.state.cpu().numpy()
        count = host[0].view(np.uint32).reshape(nz, ny, nx)
        sdf_sum = host[1].reshape(nz, ny, nx)
        rgb_sum = np.ascontiguousarray(host[2:5].view(np.uint32).T).reshape(nz, ny, nx, 3)
        rgb_count = host[5].view(np.uint32).reshape(nz, ny, nx)
        with np.errstate(invalid="ignore", divide="ignore"):
            sdf = np.where(count > 0, sdf_sum / (count.astype(np.float64) * SDF_ONE), np.nan).astype(np.float32)
            rgb = np.where(rgb_count[..., None] > 0, np.rint(rgb_sum / rgb_count[..., None].astype(np.float64)), 0)
        return TsdfArrays(count, sdf_sum, sdf, rgb.astype(np.uint8), rgb_sum, rgb_count)

    def integrate(self, views, imgs: Sequence[torch.Tensor], depths: Sequence[torch.Tensor], *,
                  masks: Optional[Sequence[Optional[torch.Tensor]]] = None, alpha_min: float = 0.5,
                  max_depth: Optional[float] = None, near: float = 0.2, depth_kind: str = "accumulated") -> None:
        """Fuses views into the volume (brush_tsdf_integrate_ex), up to MAX_VIEWS per launch: launches and the upload of the
        view records (96 bytes a view), no read-back, no synchronisation.  `views`:
        SceneViews or (Camera, (w, h)) pairs, or their filter3d.view_records as a float32 [V, 24] HOST array; `imgs[v]`:
        the view's raw render, float32 [h, w, 4] on the volume's device (premultiplied colour and alpha, as
        render_splats_depth returns it); `depths[v]`: its accumulated depth, float32 [h, w]; `masks[v]`: uint8 [h, w]
        or None, 0 = ignore the pixel.  A pixel is used where alpha >= alpha_min and 0 < depth / alpha <= max_depth
        (None: no limit); a voxel is seen by a view where its camera-space z exceeds `near`.  `depth_kind`:
        "accumulated" (the default): depths[v] is D = sum T alpha z and the distance is D / alpha; "metric": depths[v]
        already is a distance (a median depth map) and is used as it is, alpha still gating the pixel."""
        from .filter3d import VIEW_WORDS, view_records

        flags = _depth_kind_flags(depth_kind)
        rec = views if isinstance(views, np.ndarray) else view_records(views)
        if rec.ndim != 2 or rec.shape[1] != VIEW_WORDS or rec.dtype != np.float32:
            raise ValueError(f"view records must be a float32 [V,{VIEW_WORDS}] host array, got {rec.dtype} {rec.shape}")
        nv = int(rec.shape[0])
        if len(imgs) != nv or len(depths) != nv or (masks is not None and len(masks) != nv):
            raise ValueError(f"{nv} views need {nv} images, depth maps and (if any) masks")
        if not (math.isfinite(alpha_min) and alpha_min > 0):
            raise ValueError(f"alpha_min must be finite and > 0, got {alpha_min!r}")
        if not (math.isfinite(near) and near >= 0):
            raise ValueError(f"near must be finite and >= 0, got {near!r}")
        max_depth = math.inf if max_depth is None else float(max_depth)
        if not max_depth > 0:
            raise ValueError(f"max_depth must be > 0, got {max_depth!r}")
        sizes = rec.view(np.uint32)[:, 20:22]
        keep = []  # what the launches read: alive until they are enqueued (the stream orders the rest)
        data = (_lib.BrushTsdfViewData * max(nv, 1))()
        for v in range(nv):
            w, h = int(sizes[v, 0]), int(sizes[v, 1])
            img = self._checked(imgs[v], (h, w, 4), torch.float32, f"imgs[{v}]")
            dep = self._checked(depths[v], (h, w), torch.float32, f"depths[{v}]")
            msk = None if masks is None or masks[v] is None else self._checked(masks[v], (h, w), torch.uint8,
                                                                                f"masks[{v}]")
            keep.append((img, dep, msk))
            data[v].img, data[v].depth = img.data_ptr(), dep.data_ptr()
            data[v].mask = None if msk is None else msk.data_ptr()
        if nv == 0:
            return
        rec_dev = torch.from_numpy(np.ascontiguousarray(rec)).to(self.device)
        grid = self._grid()
        with torch.cuda.device(self.device):
            stream = _lib.current_stream()
            for base in range(0, nv, MAX_VIEWS):
                k = min(MAX_VIEWS, nv - base)
                chunk = C.cast(C.addressof(data) + base * C.sizeof(_lib.BrushTsdfViewData),
                               C.POINTER(_lib.BrushTsdfViewData))
                _lib.check(_lib.lib().brush_tsdf_integrate_ex(C.byref(grid), self.state.data_ptr(),
                                                              rec_dev.data_ptr() + base * VIEW_WORDS * 4, chunk, k,
                                                              float(alpha_min), max_depth, float(near), flags, stream),
                           "brush_tsdf_integrate_ex")
        self.views += nv

    def _checked(self, t, shape, dtype, what):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype \
                or t.device != self.device:
            got = (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)
            raise ValueError(f"{what} must be a {dtype} {tuple(shape)} tensor on {self.device}, got {got}")
        return t.detach().contiguous()

    def integrate_splats(self, splats, views, *, antialiased: bool = False, use_masks: bool = True,
                         views_per_launch: Optional[int] = None, alpha_min: float = 0.5,
                         max_depth: Optional[float] = None, near: float = 0.2, depth: str = "expected",
                         level: float = 0.5) -> None:
        """Renders `splats` from every view (Splats.render_depth at the view's own size) and fuses the renders,
        `views_per_launch` at a time (default DEFAULT_VIEWS_PER_LAUNCH, at most MAX_VIEWS): that many renders are alive
        at once.  `views`: SceneViews, whose loss masks are honoured unless `use_masks` is False, or (Camera, (w, h))
        pairs.  The volume's bits do not depend on `views_per_launch` or on the order of the views.
        `depth`: "expected" (the default) fuses D / alpha; "median" fuses the median depth at `level`
        (Splats.render_median_depth: the z of the splat at which the accumulated opacity first reaches `level`), which
        does not blend a silhouette's foreground with what lies behind it."""
        from .render import view_parts
        from .median_depth import check_level

        if depth not in ("expected", "median"):
            raise ValueError(f"depth must be 'expected' or 'median', got {depth!r}")
        level = check_level(level)
        k = DEFAULT_VIEWS_PER_LAUNCH if views_per_launch is None else int(views_per_launch)
        if not 1 <= k <= MAX_VIEWS:
            raise ValueError(f"views_per_launch must be in [1, {MAX_VIEWS}], got {views_per_launch!r}")
        views = list(views)
        with torch.no_grad():
            for base in range(0, len(views), k):
                chunk = views[base:base + k]
                imgs, depths, masks = [], [], []
                for v in chunk:
                    cam, size = view_parts(v)[:2]
                    if depth == "median":
                        img, _, dmap, _, _ = splats.render_median_depth(cam, size, level=level, antialiased=antialiased)
                    else:
                        img, dmap, _ = splats.render_depth(cam, size, antialiased=antialiased)
                    imgs.append(img)
                    depths.append(dmap)
                    m = getattr(v, "mask", None) if use_masks else None
                    masks.append(None if m is None else torch.from_numpy(np.ascontiguousarray(m)).to(self.device))
                self.integrate(chunk, imgs, depths, masks=masks, alpha_min=alpha_min, max_depth=max_depth, near=near,
                               depth_kind="metric" if depth == "median" else "accumulated")

    def extract_mesh(self, min_views: int = 2):
        """The surface sdf = 0 as an indexed triangle mesh (brush_amd.mesh.Mesh, host arrays): marching tetrahedra over
        the lattice of voxel centres, using only voxels at least `min_views` views observed.  Vertices are in lattice
        order, faces in cell order, normals point towards positive distance (at the cameras); a volume without a
        surface gives an empty mesh.  One read-back (the two totals) between counting and emitting."""
        from .mesh import Mesh

        min_views = int(min_views)
        if min_views < 1:
            raise ValueError(f"min_views must be at least 1, got {min_views}")
        l = _lib.lib()
        nbytes = _lib.size_query("brush_tsdf_mesh_workspace_size", *self.dims)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        totals = torch.zeros(2, dtype=torch.int32, device=self.device)
        grid = self._grid()
        with torch.cuda.device(self.device):
            stream = _lib.current_stream()
            _lib.check(l.brush_tsdf_mesh_count(C.byref(grid), self.state.data_ptr(), min_views, totals.data_ptr(),
                                               ws.data_ptr(), nbytes, stream), "brush_tsdf_mesh_count")
            nvert, nface = (int(x) & 0xFFFFFFFF for x in totals.cpu().tolist())
            vertices = torch.empty((nvert, 3), dtype=torch.float32, device=self.device)
            colors = torch.empty((nvert, 3), dtype=torch.uint8, device=self.device)
            faces = torch.empty((nface, 3), dtype=torch.int32, device=self.device)
            _lib.check(l.brush_tsdf_mesh_emit(C.byref(grid), self.state.data_ptr(), min_views, nvert, nface,
                                              vertices.data_ptr() if nvert else None,
                                              colors.data_ptr() if nvert else None,
                                              faces.data_ptr() if nface else None, ws.data_ptr(), nbytes, stream),
                       "brush_tsdf_mesh_emit")
        return Mesh(vertices.cpu().numpy(), colors.cpu().numpy(), faces.cpu().numpy())
