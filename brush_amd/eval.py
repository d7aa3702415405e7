"""Evaluation on held-out views — mirror of crates/brush-train/src/eval.rs.

`eval_stats` renders each eval view of a Scene and scores it against the view's image with PSNR and SSIM
(eval.rs:27-77); the metrics come from one fused HIP pass per view (include/brush_hip.h: brush_eval_metrics) and
are read back once, after the last view (the reference syncs twice per view).

Command line (prints one line per view, then the means):

    python -m brush_amd.eval SPLATS DATASET [--format auto|nerf|colmap] [--eval-split-every K]
                             [--max-resolution R] [--num-frames K] [--seed S] [--window 11] [--json OUT]
                             [--depth-metrics] [--depth-mode depth|disparity] [--downscale 1,2,4,8]
                             [--depth-dir DIR [--depth-median]] [--normal-dir DIR] [--distortion-dir DIR]
                             [--background white|black|R,G,B] [--no-masks]

--background white scores over a white background (the protocol of the NeRF-synthetic numbers in the literature): the
render and the image's straight RGBA are composed over the colour first (brush_amd/compose.py).  A view's loss mask
(nerfstudio's mask_path, COLMAP's masks/<image name>.png) leaves its zero pixels out of the PSNR unless --no-masks.

--normal-dir DIR writes two camera-space normal maps per eval view (brush_amd/normal_loss.py): <stem>_normal.npy, the
rendered map of the splats' normals divided by its length where alpha >= 0.5 (0 elsewhere), and <stem>_normal_depth.npy,
the normals of the surface the rendered depth map implies (0 where a pixel or a neighbour is not covered); both f32
[h,w,3], facing the camera (z < 0).

--distortion-dir DIR writes the depth-distortion map of every eval view (brush_amd/distortion.py):
<stem>_distortion.npy, sum over the pairs of a pixel's splats of w_i w_j (z_i - z_j)^2, f32 [h,w]: large where a ray
crosses a thick or doubled surface.

--downscale 1,2,4,8 is Mip-Splatting's multi-scale protocol: the views are scored once per scale, rendered at 1 / scale
of their size against the image area-filtered to that size on the device (brush_amd/pyramid.py); one block of lines per
scale, and a `scales` list in --json.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _lib, cli
from .dataset import detect_format  # noqa: F401  (its home is dataset.py; importable from here as before)


def eval_metrics(pred: torch.Tensor, gt: torch.Tensor, window: int = 11,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """{mse, psnr, ssim} of pred's RGB against gt's RGB as a float32 [3] device tensor (brush_eval_metrics); does not
    synchronise.  pred: [h,w,4] float32 (the op's output); gt: [h,w,3|4] uint8 (read as b / 255) or float32; the
    alpha of both is ignored (eval.rs:50-57).  `window`: SSIM window, odd 3..15 (the reference's eval uses 11).
    `out`: optional contiguous float32 [3] device tensor to write into (e.g. a row of a [V,3] tensor)."""
    assert pred.is_cuda and gt.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if pred.dim() != 3 or gt.dim() != 3:
        raise ValueError(f"pred must be [h,w,4] and gt [h,w,3|4], got {tuple(pred.shape)} / {tuple(gt.shape)}")
    h, w = int(pred.shape[0]), int(pred.shape[1])
    if tuple(pred.shape) != (h, w, 4) or tuple(gt.shape[:2]) != (h, w) or gt.shape[2] not in (3, 4):
        raise ValueError(f"pred must be [h,w,4] and gt [h,w,3|4], got {tuple(pred.shape)} / {tuple(gt.shape)}")
    if pred.dtype != torch.float32:
        raise ValueError(f"pred must be float32, got {pred.dtype}")
    dtypes = {torch.uint8: _lib.EVAL_GT_U8, torch.float32: _lib.EVAL_GT_F32}
    if gt.dtype not in dtypes:
        raise ValueError(f"gt must be uint8 or float32, got {gt.dtype}")
    if int(window) not in (3, 5, 7, 9, 11, 13, 15):
        raise ValueError(f"window must be an odd size 3..15, got {window}")
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=pred.device)
    elif tuple(out.shape) != (3,) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != pred.device:
        raise ValueError("out must be a contiguous float32 [3] tensor on pred's device")
    pred, gt = pred.contiguous(), gt.contiguous()
    l = _lib.lib()
    nbytes = _lib.size_query("brush_eval_workspace_size", w, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(l.brush_eval_metrics(pred.data_ptr(), gt.data_ptr(), dtypes[gt.dtype], w, h, int(gt.shape[2]),
                                        int(window), out.data_ptr(), ws.data_ptr(), nbytes,
                                        _lib.current_stream()),
                   "brush_eval_metrics")
    return out


@dataclass
class EvalView:
    """eval.rs:11-20.  `rendered`: RGB [h,w,3] device tensor.  `aux`: the view's RenderAux, kept only when
    eval_stats is called with keep_aux=True (None otherwise)."""
    view: object  # dataset.SceneView
    rendered: torch.Tensor
    psnr: float
    ssim: float
    aux: object = None
    # Build extension (loss masks): kept pixels / all pixels of the view's mask at the evaluated level; 1.0 without one.
    valid_fraction: float = 1.0


@dataclass
class EvalStats:
    """eval.rs:22-25"""
    samples: List[EvalView] = field(default_factory=list)

    def mean_psnr(self) -> float:
        """Mean PSNR over the samples (what the viewer logs, rerun.rs:163-185); nan without samples."""
        return float(np.mean([s.psnr for s in self.samples])) if self.samples else float("nan")

    def mean_ssim(self) -> float:
        """Mean SSIM over the samples (rerun.rs:163-185); nan without samples."""
        return float(np.mean([s.ssim for s in self.samples])) if self.samples else float("nan")


def select_views(num_views: int, num_frames: Optional[int] = None,
                 rng: Optional[np.random.Generator] = None) -> List[int]:
    """Indices of the views eval_stats scores (eval.rs:34-38): every view in order when num_frames is None or at least
    num_views, else num_frames distinct views sampled with `rng` (a numpy Generator; a fresh one when None), in
    ascending order."""
    if num_frames is None or num_frames >= num_views:
        return list(range(num_views))
    if num_frames < 0:
        raise ValueError(f"num_frames must be >= 0, got {num_frames}")
    rng = np.random.default_rng() if rng is None else rng
    return sorted(int(i) for i in rng.choice(num_views, size=int(num_frames), replace=False))


def eval_stats(splats, scene, num_frames: Optional[int] = None, rng: Optional[np.random.Generator] = None,
               window: int = 11, keep_aux: bool = False, antialiased: bool = False, downscale: int = 1,
               background=None, use_masks: bool = True) -> EvalStats:
    """eval.rs:27-77: render each selected view of `scene` (a dataset.Scene, e.g. Dataset.eval) at its image's size
    through Splats.render under no_grad and score it against the image's RGB, uploaded as uint8, with eval_metrics.
    The metrics of all views go into one [V,3] device tensor that is read back once, after the last view.
    `antialiased`: render in the antialiased mode (render.render_splats), e.g. splats trained in it.
    `downscale` = f > 1 scores at 1 / f: the uploaded image goes through pyramid.area_resize and the view is rendered at
    pyramid.downscaled_size of its size (the camera is a field of view: it holds at any size); 1 is the call without it.

    One deviation from the reference: `aux` is kept only with keep_aux=True, because a RenderAux holds the
    intersection lists of its view (hundreds of MB for a large scene).

    Trainer state: rendering goes through Splats.render, which applies the SH optimizer steps a SplatTrainer has
    deferred (Splats.sync), exactly as any render or trainer.sync() does; nothing else of the trainer changes.  Call it
    from the trainer's thread and stream, between step() calls.

    `background` (None, "white", "black", an (r, g, b) tuple or a float32 [3] device tensor) and the views' loss masks
    (SceneView.mask, honoured when `use_masks`): with a background or a masked view among the selected ones, each view
    goes through compose.compose_forward first (render and straight-alpha image composed over the colour, both zeroed
    where the mask is 0; a mask follows `downscale` through pyramid.nearest_resize) and eval_metrics scores the float32
    result.  A masked view's `valid_fraction` f is an exact count of the mask's nonzero pixels at the evaluated level,
    read back with the metrics (at most one more read-back, after the last view), and its psnr is 10 log10(f / mse),
    computed on the host in float64 from the read-back mse, the PSNR over the kept pixels (nan when f == 0).  Its ssim
    is the mean SSIM of the masked images as they are, zeroed pixels included: the blur mixes pixels across the mask's
    edge, so there is no exact per-pixel restriction of it.  With neither option in play the call is the one without
    them, launch for launch."""
    import math

    from .compose import as_background, compose_forward
    from .pyramid import check_factor
    from .render import view_parts

    downscale = check_factor(downscale)
    views = scene.views
    idx = select_views(len(views), num_frames, rng)
    dev = splats.means.device
    if isinstance(background, str) and background == "random":
        raise ValueError("an eval has no 'random' background: score over a fixed colour")
    bg = as_background(background, dev)
    metrics = torch.empty((len(idx), 3), dtype=torch.float32, device=dev)
    masked = use_masks and any(getattr(views[i], "mask", None) is not None for i in idx)
    kept = torch.zeros(len(idx), dtype=torch.int64, device=dev) if masked else None  # nonzero mask pixels per view
    pixels = [0] * len(idx)                                                          # mask pixels per view; 0: no mask
    rendered = []
    with torch.no_grad():
        for row, i in enumerate(idx):
            # the image as u8, as the reference uploads to_rgb8() (the kernel divides by 255)
            camera, _, gt, mask = view_parts(views[i], dev, downscale=downscale, gt=True, mask=use_masks)
            h, w = int(gt.shape[0]), int(gt.shape[1])
            pred, aux = splats.render(camera, (w, h), False, antialiased=antialiased)
            if bg is None and mask is None:  # a plain view, possibly among masked ones
                eval_metrics(pred, gt, window, out=metrics[row])
                shown = pred
            else:
                shown, target = compose_forward(pred, gt, background=bg, mask=mask)
                eval_metrics(shown, target, window, out=metrics[row])
            if mask is not None:
                kept[row] = torch.count_nonzero(mask)
                pixels[row] = h * w
            rendered.append((shown[..., :3], aux if keep_aux else None))
    host = metrics.cpu().numpy()  # the one read-back without masks
    host_kept = kept.cpu().numpy() if masked else None  # the one further read-back
    samples = []
    for k, (i, (r, a)) in enumerate(zip(idx, rendered)):
        psnr, f = float(host[k, 1]), 1.0
        if pixels[k] > 0:
            f = float(host_kept[k]) / float(pixels[k])
            mse = float(host[k, 0])
            if f == 0.0:
                psnr = float("nan")
            else:
                psnr = 10.0 * math.log10(f / mse) if mse > 0.0 else float("inf")
        samples.append(EvalView(views[i], r, psnr, float(host[k, 2]), a, f))
    return EvalStats(samples)


@dataclass
class DepthEvalView:
    """One view of eval_depth.  `mean_abs_error`: mean |r| over the view's valid pixels (nan when none is valid), r as
    brush_depth_loss defines it for the mode; `valid_fraction`: valid pixels / all pixels."""
    view: object  # dataset.SceneView
    mean_abs_error: float
    valid_fraction: float


def eval_depth(splats, scene, *, mode: str = "depth", alpha_min: float = 0.5,
               antialiased: bool = False) -> List[DepthEvalView]:
    """The depth error of `splats` on every view of `scene` (a dataset.Scene) that has a depth map: the view is
    rendered with its depth output at the map's size (Splats.render_depth under no_grad) and scored by
    brush_depth_loss, metrics only, with weight 1 against the map as stored (uint16 or float32, with the view's
    depth_scale / depth_offset).  The kernel's mean runs over all pixels and its second word is the valid fraction, so
    the mean over the valid pixels is stats[0] / stats[1].  The statistics of all views are read back once, after the
    last view.  Views without a depth map are skipped; the result is empty when no view has one."""
    from .depth_loss import depth_loss_into

    views = [v for v in scene.views if getattr(v, "depth", None) is not None]
    dev = splats.means.device
    stats = torch.empty((len(views), 2), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for row, v in enumerate(views):
            d = np.require(v.depth, requirements=["C", "W"])
            if d.ndim != 2 or d.dtype not in (np.uint16, np.float32):
                raise ValueError(f"{v.name}: the view's depth map must be uint16 or float32 [h,w], got {d.dtype} {d.shape}")
            h, w = int(d.shape[0]), int(d.shape[1])
            img, depth, _ = splats.render_depth(v.camera, (w, h), antialiased=antialiased)
            _, st = depth_loss_into(img, depth, torch.from_numpy(d).to(dev), None, weight=1.0,
                                    scale=float(v.depth_scale), offset=float(v.depth_offset), alpha_min=alpha_min,
                                    mode=mode, want_v_depth=False)
            stats[row].copy_(st)
    host = stats.cpu().numpy().astype(np.float64)  # the one readback
    return [DepthEvalView(v, float(host[k, 0] / host[k, 1]) if host[k, 1] > 0 else float("nan"), float(host[k, 1]))
            for k, v in enumerate(views)]


def _write_maps(views, out_dir: str, render, save=None):
    """The loop of the writers below: under no_grad, for each view, `render(camera, (w, h))` at the size of the view's
    image gives pairs (suffix, device tensor), and each tensor is written to out_dir/<stem of the view's name><suffix>
    by `save(path, tensor)` (None: np.save as float32).  Returns the written paths."""
    import os

    if save is None:
        save = lambda path, t: np.save(path, t.cpu().numpy().astype(np.float32))
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    with torch.no_grad():
        for v in views:
            h, w = int(v.image.shape[0]), int(v.image.shape[1])
            stem = os.path.splitext(os.path.basename(v.name))[0]
            for suffix, t in render(v.camera, (w, h)):
                paths.append(os.path.join(out_dir, stem + suffix))
                save(paths[-1], t)
    return paths


def write_depth_maps(splats, views, out_dir: str, median: bool = False):
    """For each view: <stem>_depth.npy, the accumulated depth D = sum T alpha z (Splats.render_depth), and
    <stem>_depth_norm.npy, D / max(alpha, 1e-6) with 0 where alpha is 0; both f32 [h,w].  `median`: also
    <stem>_depth_median.npy, the median depth at level 0.5 (Splats.render_median_depth; 0 where alpha < 0.5).  Returns
    the written paths."""
    def render(camera, size):
        if median:
            img, depth, med, _, _ = splats.render_median_depth(camera, size)
        else:
            img, depth, _ = splats.render_depth(camera, size)
        alpha = img[..., 3]
        norm = torch.where(alpha > 0, depth / torch.clamp(alpha, min=1e-6), torch.zeros_like(depth))
        return (("_depth.npy", depth), ("_depth_norm.npy", norm)) + ((("_depth_median.npy", med),) if median else ())

    return _write_maps(views, out_dir, render)


def write_normal_maps(splats, views, out_dir: str, antialiased: bool = False):
    """For each view: <stem>_normal.npy, the rendered normal map (Splats.render_normals) divided by its length where
    alpha >= 0.5, 0 elsewhere, and <stem>_normal_depth.npy, the normals the rendered depth map implies
    (normal_loss.depth_normals, alpha_min 0.5; 0 where invalid); both f32 [h,w,3], camera space.  Returns the written
    paths."""
    from .normal_loss import depth_normals

    def render(camera, size):
        img, depth, nimg, _ = splats.render_normals(camera, size, antialiased=antialiased)
        length = torch.sqrt((nimg * nimg).sum(dim=2, keepdim=True))
        keep = (img[..., 3:4] >= 0.5) & (length > 0)
        unit = torch.where(keep, nimg / torch.where(keep, length, torch.ones_like(length)), torch.zeros_like(nimg))
        from_depth, _ = depth_normals(camera, size, img, depth, alpha_min=0.5)
        return ("_normal.npy", unit), ("_normal_depth.npy", from_depth)

    return _write_maps(views, out_dir, render)


def write_distortion_maps(splats, views, out_dir: str, antialiased: bool = False):
    """For each view: <stem>_distortion.npy, the depth-distortion map sum w_i w_j (z_i - z_j)^2 of the view
    (Splats.render_distortion, mode "depth"), f32 [h,w].  Returns the written paths."""
    def render(camera, size):
        return (("_distortion.npy", splats.render_distortion(camera, size, antialiased=antialiased)[2]),)

    return _write_maps(views, out_dir, render)


def zoomed_camera(camera, img_size, zoom: float):
    """`camera` with `zoom` times its focal lengths on an image of the same size and the same principal point: the
    central 1 / zoom of the view, magnified (a zoom-in no training view sampled, which is what the 3D smoothing filter
    of brush_amd/filter3d.py is for)."""
    from .camera import Camera, focal_to_fov

    w, h = int(img_size[0]), int(img_size[1])
    fx, fy = camera.focal((w, h))
    return Camera(camera.position, camera.rotation, focal_to_fov(float(fx) * zoom, w), focal_to_fov(float(fy) * zoom, h),
                  camera.center_uv)


def write_zoomed_renders(splats, views, zoom: float, out_dir: str, antialiased: bool = False, background=None):
    """For each view: <stem>_zoom<zoom>.png, the view rendered through zoomed_camera at its own size, composed over
    `background` (an (r, g, b) tuple, "white" or "black"; None: black) and written as 8-bit RGB.  There is no ground
    truth for a zoom-in, so nothing is scored: the images are for inspection.  Returns the written paths."""
    from PIL import Image

    from .compose import check_background

    bg = check_background(background)
    rgb = {None: (0.0, 0.0, 0.0), "black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0)}.get(bg, bg)

    def render(camera, size):
        img, _ = splats.render(zoomed_camera(camera, size, zoom), size, antialiased=antialiased)
        colour = torch.tensor(rgb, dtype=torch.float32, device=img.device)
        out = img[..., :3] + (1.0 - img[..., 3:4]) * colour
        return ((f"_zoom{zoom:g}.png", torch.clamp(torch.round(out * 255.0), 0, 255).to(torch.uint8)),)

    return _write_maps(views, out_dir, render, save=lambda path, u8: Image.fromarray(u8.cpu().numpy()).save(path))


# ---------------------------------------------------------------------------- command line
def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.eval",
                                description="PSNR / SSIM of a splat file on a dataset's eval views")
    p.add_argument("splats", help=".ply or .safetensors splat file")
    p.add_argument("dataset", help="dataset directory or .zip (NeRF-synthetic or COLMAP)")
    cli.add_dataset_options(p)
    p.add_argument("--num-frames", type=int, default=None)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--window", type=int, default=11)
    cli.add_json_option(p)
    p.add_argument("--depth-dir", default=None,
                   help="also write every eval view's accumulated depth D (<view stem>_depth.npy, f32 [h,w]) and "
                        "D / alpha (<view stem>_depth_norm.npy, 0 where alpha is 0) to this directory")
    p.add_argument("--depth-median", action="store_true",
                   help="--depth-dir: also write every eval view's median depth (<view stem>_depth_median.npy: the z "
                        "of the splat at which the accumulated opacity first reaches one half, 0 where it never does)")
    p.add_argument("--distortion-dir", default=None,
                   help="also write every eval view's depth-distortion map (<view stem>_distortion.npy, f32 [h,w]) to "
                        "this directory")
    p.add_argument("--normal-dir", default=None,
                   help="also write every eval view's rendered normal map (<view stem>_normal.npy, unit where alpha >= "
                        "0.5, else 0) and the normals its depth map implies (<view stem>_normal_depth.npy) to this "
                        "directory, f32 [h,w,3] in camera space")
    cli.add_antialiased_option(p)
    p.add_argument("--depth-metrics", action="store_true",
                   help="also score the rendered depth of every eval view that has a depth map: mean absolute error "
                        "over the valid pixels and the valid fraction (eval_depth)")
    p.add_argument("--depth-mode", choices=("depth", "disparity"), default="depth",
                   help="--depth-metrics: compare depth / alpha, or alpha / depth (maps of inverse depths)")
    p.add_argument("--downscale", default=None, metavar="F,...",
                   help="multi-scale eval: score once per factor (1..16, e.g. 1,2,4,8), rendering at 1 / F of each "
                        "view's size against the area-filtered image")
    p.add_argument("--background", default=None, metavar="white|black|R,G,B",
                   help="score over this background colour: the render and the image's straight RGBA are composed "
                        "over it first (white: the protocol of the NeRF-synthetic numbers in the literature)")
    p.add_argument("--no-masks", action="store_true",
                   help="ignore the dataset's loss masks (nerfstudio's mask_path, COLMAP's masks/<image name>.png)")
    p.add_argument("--zoom", type=float, default=None, metavar="Z",
                   help="with --image-dir: also render every scored view at Z times its focal length (same size and "
                        "principal point) and write the images for inspection; a zoom-in has no ground truth, so "
                        "nothing is scored (metrics across scales: --downscale)")
    p.add_argument("--image-dir", default=None, metavar="DIR", help="--zoom: where the zoomed renders go")
    return p


def parse_scales(text: str) -> List[int]:
    """'1,2,4,8' -> [1, 2, 4, 8]; ValueError for anything that is not a list of factors 1..16."""
    from .pyramid import check_factor

    try:
        return [check_factor(int(x)) for x in text.split(",")]
    except ValueError:
        raise ValueError(f"--downscale takes factors from 1 to 16 separated by commas, got {text!r}") from None


def main(argv=None) -> int:
    import os
    import sys

    p = parser()
    args = p.parse_args(argv)
    scales = None
    if args.downscale is not None:
        try:
            scales = parse_scales(args.downscale)
        except ValueError as e:
            p.error(str(e))
    background = None
    if args.background is not None:
        from .compose import parse_background

        try:
            background = parse_background(args.background)
            if background == "random":
                raise ValueError("--background random is a training option: an eval scores over a fixed colour")
        except ValueError as e:
            p.error(str(e))
    compose_args = {"background": background, "use_masks": not args.no_masks}
    if (args.zoom is None) != (args.image_dir is None):
        p.error("--zoom and --image-dir go together")
    if args.depth_median and args.depth_dir is None:
        p.error("--depth-median needs --depth-dir")
    if args.zoom is not None and not (args.zoom > 0 and args.zoom < float("inf")):
        p.error("--zoom must be a positive factor")

    data = cli.read_args_dataset(args)  # before any GPU work
    if not cli.chosen_views(data, "eval"):
        print(f"{args.dataset}: the dataset has no eval views (try --eval-split-every K)", file=sys.stderr)
        return 2
    from .undistort import undistort_for_cli

    dev = cli.cuda_device()
    data = undistort_for_cli(data, not args.no_undistort, dev)
    splats = cli.load_splats(args.splats, dev)
    rng = np.random.default_rng(args.seed)
    scale_rows = None
    if scales is None:
        stats = eval_stats(splats, data.eval, args.num_frames, rng, args.window, antialiased=args.antialiased,
                           **compose_args)
        for s in stats.samples:
            print(f"{s.view.name}\tpsnr {s.psnr:.4f}\tssim {s.ssim:.6f}")
        print(f"mean ({len(stats.samples)} views)\tpsnr {stats.mean_psnr():.4f}\tssim {stats.mean_ssim():.6f}")
    else:
        # the same views at every scale: chosen once, then scored as a scene of their own
        from .dataset import Scene

        chosen = Scene([data.eval.views[i] for i in select_views(len(data.eval.views), args.num_frames, rng)])
        scale_rows, stats = [], None
        for f in scales:
            st = eval_stats(splats, chosen, None, None, args.window, antialiased=args.antialiased, downscale=f,
                            **compose_args)
            stats = st if stats is None or f == 1 else stats  # the top-level rows: scale 1 when asked for, else the first
            for s in st.samples:
                print(f"scale 1/{f}\t{s.view.name}\tpsnr {s.psnr:.4f}\tssim {s.ssim:.6f}")
            print(f"scale 1/{f}\tmean ({len(st.samples)} views)\tpsnr {st.mean_psnr():.4f}\tssim {st.mean_ssim():.6f}")
            scale_rows.append({"downscale": f,
                               "views": [{"name": s.view.name, "psnr": s.psnr, "ssim": s.ssim} for s in st.samples],
                               "mean_psnr": st.mean_psnr(), "mean_ssim": st.mean_ssim()})
    if args.depth_dir:
        write_depth_maps(splats, [s.view for s in stats.samples], args.depth_dir, median=args.depth_median)
    if args.normal_dir:
        write_normal_maps(splats, [s.view for s in stats.samples], args.normal_dir, antialiased=args.antialiased)
    if args.distortion_dir:
        write_distortion_maps(splats, [s.view for s in stats.samples], args.distortion_dir,
                              antialiased=args.antialiased)
    if args.zoom is not None:
        for path in write_zoomed_renders(splats, [s.view for s in stats.samples], args.zoom, args.image_dir,
                                         antialiased=args.antialiased, background=background):
            print(f"zoom {args.zoom:g}\t{path}")
    depth_rows = None
    if args.depth_metrics:
        depth_rows = eval_depth(splats, data.eval, mode=args.depth_mode, antialiased=args.antialiased)
        for r in depth_rows:
            print(f"{r.view.name}\tdepth_mae {r.mean_abs_error:.6f}\tvalid {r.valid_fraction:.4f}")
        mae = float(np.mean([r.mean_abs_error for r in depth_rows])) if depth_rows else float("nan")
        print(f"mean ({len(depth_rows)} views with depth)\tdepth_mae {mae:.6f}")
    if args.json:
        res = {"splats": os.path.abspath(args.splats), "dataset": os.path.abspath(args.dataset), "window": args.window,
               "antialiased": bool(args.antialiased),
               "background": list(background) if isinstance(background, tuple) else background,
               "use_masks": not args.no_masks,
               "views": [{"name": s.view.name, "psnr": s.psnr, "ssim": s.ssim} for s in stats.samples],
               "mean_psnr": stats.mean_psnr(), "mean_ssim": stats.mean_ssim()}
        if scale_rows is not None:
            res["scales"] = scale_rows
        if depth_rows is not None:
            res["depth_mode"] = args.depth_mode
            res["depth_views"] = [{"name": r.view.name, "mean_abs_error": r.mean_abs_error,
                                   "valid_fraction": r.valid_fraction} for r in depth_rows]
            res["mean_depth_abs_error"] = (float(np.mean([r.mean_abs_error for r in depth_rows])) if depth_rows
                                           else float("nan"))
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
