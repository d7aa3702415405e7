"""Training a scene end to end — mirror of crates/brush-viewer/src/train_loop.rs without the viewer's messages.

    dataset -> initial splats -> (random training view, SplatTrainer.step) x steps -> eval on request -> splats

Initial splats (train_loop.rs:57-90): a caller's splats (e.g. a .ply) win; else the COLMAP SfM points
(colmap_initial_points + Splats.from_point_cloud); else `Splats.from_random_config` inside
`train.bounds(0.25 |e|, |e|)`, |e| the length of `train.bounds(0, 0)`'s extent.  The training images are uploaded
once, as u8, by scene_loader.SceneLoader, and the loss kernels read them as they are (brush_l1_ssim_loss_gt).  Each
step's loss goes into a preallocated device log; between refinements a step neither uploads, reads back nor
synchronises, and the log is read back at eval points and at the end.

Command line (one line per eval and a last line; --json also writes the eval rows and the loss curve):

    python -m brush_amd.train_loop DATASET [--steps 30000] [--format auto|nerf|colmap] [--max-resolution R]
        [--eval-split-every K] [--eval-every N] [--eval-views V] [--init PLY] [--init-count 10000] [--sh-degree 3]
        [--seed 42] [--export OUT.ply] [--json LOG] [--antialiased] [--pose-opt] [--export-cameras CAMS.json]
        [--strategy default|mcmc] [--cap-max 1000000] [--exposure-opt] [--export-exposures EXP.json]
        [--bilagrid-opt] [--bilagrid-shape 16,16,8] [--bilagrid-tv W] [--export-bilagrids GRIDS.npz]
        [--depth-weight W] [--depth-weight-final W] [--depth-mode depth|disparity]
        [--normal-weight W] [--normal-from-step S]
        [--distortion-weight W] [--distortion-from-step S] [--distortion-mode depth|ndc] [--distortion-far Z]
        [--downscale-schedule STEP:FACTOR,...] [--num-downscales K] [--resolution-schedule S]
        [--contribution-prune-at STEP,...] [--contribution-prune-min 0.01]
        [--background white|black|random|R,G,B] [--no-masks] [--filter3d] [--filter3d-every 100]
        [--densify-by grad|error] [--densify-error-thresh 1.0] [--densify-error-views 32] [--densify-growth 0.05]
        [--max-splats N] [--revised-opacity]

--densify-by error replaces the refinement's gradient rule (TrainConfig.densify_by, brush_amd/error_score.py): in front
of every refining step the loop renders --densify-error-views training views (0: all), distributes each view's per-pixel
L1 error to the splats by their blending weights and densifies the splats whose largest share reaches
--densify-error-thresh, at most --densify-growth of the count per refinement and never beyond --max-splats.
--revised-opacity gives the two splats a clone or split leaves the opacity 1 - sqrt(1 - o) (under either rule).  The
log's `error_passes` holds (step, views).

--filter3d trains under Mip-Splatting's 3D smoothing filter (TrainConfig.filter3d, brush_amd/filter3d.py): every splat
is low-passed at the highest rate any training view sampled it, recomputed every --filter3d-every steps and whenever the
splat count changed.  Evals, contribution prunes and --export then work on the baked splats (Splats.bake_filter3d), which
any viewer shows correctly; the JSON log records the mode.

--background composes the render and the (straight-alpha) target over a colour in front of the loss and in the evals
(TrainConfig.background, brush_amd/compose.py); random draws a colour per step on the device and evaluates over black.
Loss masks (nerfstudio's mask_path; COLMAP's masks/<image name>.png) are honoured unless --no-masks is given: masked
pixels are left out of the loss, the depth term and the eval's PSNR.

--contribution-prune-at 16000,24000 drops, after each listed step, the splats whose largest blending weight over all
training views stays below --contribution-prune-min (TrainConfig.contribution_prune_at, brush_amd/contribution.py); the
log's `prunes` holds (step, splats before, after).

--downscale-schedule 0:4,3000:2,6000:1 trains coarse to fine (TrainConfig.downscale_schedule, brush_amd/pyramid.py): from
each STEP on, the training targets are the resident images at 1 / FACTOR of their stored size, area-filtered on the device
(depth maps: nearest neighbour).  --num-downscales K --resolution-schedule S is nerfstudio's spelling of the same thing:
the pairs (i S, 2^(K - i)) for i = 0..K.  Evals render at the eval views' full size whatever the schedule says.

--depth-weight W > 0 supervises the rendered depth with the dataset's depth maps (nerfstudio's depth_file_path; COLMAP's
depths/<image stem>.png|.npy): W times the mean absolute difference of depth / alpha (--depth-mode disparity: alpha /
depth, for maps that hold inverse depths) is added to the loss of every view that has a map (TrainConfig.depth_weight,
brush_amd/depth_loss.py).  --depth-weight-final W2 moves the weight exponentially from W to W2 over the run.

--normal-weight W > 0 adds the depth-normal consistency loss of the surface-oriented trainers from step
--normal-from-step on (TrainConfig.normal_weight, brush_amd/normal_loss.py): W times the mean over all pixels of
alpha - Nr . Nd, Nr the rendered map of the splats' normals, Nd the normal the rendered depth map implies.  It needs no
extra data; a run with it is not bitwise reproducible (float atomics in the gradient of Nr).

--distortion-weight W > 0 adds the depth-distortion term of the same trainers from step --distortion-from-step on
(TrainConfig.distortion_weight, brush_amd/distortion.py): W times the mean over all pixels of
sum over pairs of w_i w_j (m_i - m_j)^2, w the blending weights of a pixel's splats and m their depths
(--distortion-mode depth) or 2DGS's NDC mapping of them (ndc, with --distortion-far).  Its gradient goes through the
blending weights into the geometry.  No extra data; not with --pose-opt, not in deterministic mode, not bitwise
reproducible (float atomics).

--strategy mcmc trains with a fixed splat budget of --cap-max (TrainConfig.strategy, brush_amd/mcmc.py) instead of the
clone / split / prune refinement.

--pose-opt refines every training view's camera pose beside the splats (TrainConfig.pose_opt, brush_amd/pose.py);
--export-cameras writes the training views' names and 4x4 world-to-camera matrices as the run leaves them.  Eval views
carry no correction and are rendered as given.

--exposure-opt fits a 3x4 affine colour map per training view beside the splats (TrainConfig.exposure_opt,
brush_amd/exposure.py); --export-exposures writes the training views' names and maps as the run leaves them.  Eval views
are rendered as given.

--bilagrid-opt fits a bilateral grid (a GW x GH x GL lattice of affine colour maps read at pixel position and luminance,
--bilagrid-shape) per training view beside the splats (TrainConfig.bilagrid_opt, brush_amd/bilagrid.py), smoothed by a
total-variation prior of weight --bilagrid-tv; --export-bilagrids writes the training views' names and grids
[V, GL, GH, GW, 12] as the run leaves them (.npz).  Not with --exposure-opt.  Eval views are rendered as given.

BRUSH_DETERMINISTIC=1 makes the renders (and so a run with a fixed seed) bitwise repeatable.
"""
from __future__ import annotations

import dataclasses
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from . import cli
from .dataset import Dataset
from .gaussian_splats import Splats
from .scene_loader import SceneLoader
from .train import SplatTrainer, TrainConfig


@dataclass
class EvalRow:
    step: int           # training steps done when the eval ran
    psnr: float         # mean over the eval views
    ssim: float
    splats: int
    seconds: float      # wall time since the loop started, evals included
    loss: float         # loss of the last step (nan at step 0)
    iters_per_s: float  # training steps per second since the previous eval row, evals excluded


@dataclass
class TrainLog:
    steps: int
    losses: np.ndarray                            # [steps] f32, the loss of every step
    evals: List[EvalRow] = field(default_factory=list)
    seconds: float = 0.0                          # wall time of the whole loop
    train_seconds: float = 0.0                    # the same without the evals
    image_bytes: int = 0                          # training images resident on the device
    num_splats: int = 0
    pose_opt: bool = False
    pose_deltas: Optional[List[List[float]]] = None  # pose_opt: the twist (omega, tau) of every training view
    exposure_opt: bool = False
    exposures: Optional[List[List[float]]] = None    # exposure_opt: the 3x4 map (12 floats, row-major) of every view
    bilagrid_opt: bool = False                    # TrainConfig.bilagrid_opt: trained with per-view bilateral grids
    bilagrid_shape: Optional[Tuple[int, int, int]] = None  # bilagrid_opt: (GW, GH, GL)
    downscales: List[Tuple[int, int]] = field(default_factory=list)  # (step, factor): the level switches that happened
    prunes: List[Tuple[int, int, int]] = field(default_factory=list)  # (step, splats before, after): contribution prunes
    background: object = None                     # TrainConfig.background as configured
    masked_views: int = 0                         # training views whose loss mask the run used
    filter3d: bool = False                        # TrainConfig.filter3d: trained under the 3D smoothing filter
    filter3d_refreshes: List[int] = field(default_factory=list)  # the steps in front of which the filter was recomputed
    densify_by: str = "grad"                      # TrainConfig.densify_by as configured
    error_passes: List[Tuple[int, int]] = field(default_factory=list)  # (step, views): the score passes that ran
    normal_weight: float = 0.0                    # TrainConfig.normal_weight as configured (0: the term was off)
    distortion_weight: float = 0.0                # TrainConfig.distortion_weight as configured (0: the term was off)

    def to_json(self) -> dict:
        return {"steps": self.steps, "seconds": self.seconds, "train_seconds": self.train_seconds,
                "image_bytes": self.image_bytes, "num_splats": self.num_splats, "pose_opt": self.pose_opt,
                "pose_deltas": self.pose_deltas, "exposure_opt": self.exposure_opt, "exposures": self.exposures,
                "bilagrid_opt": bool(self.bilagrid_opt),
                "bilagrid_shape": None if self.bilagrid_shape is None else [int(x) for x in self.bilagrid_shape],
                "downscales": [[int(s), int(f)] for s, f in self.downscales],
                "prunes": [[int(s), int(b), int(a)] for s, b, a in self.prunes],
                "background": list(self.background) if isinstance(self.background, tuple) else self.background,
                "masked_views": int(self.masked_views), "filter3d": bool(self.filter3d),
                "filter3d_refreshes": [int(s) for s in self.filter3d_refreshes],
                "densify_by": self.densify_by, "error_passes": [[int(s), int(v)] for s, v in self.error_passes],
                "normal_weight": float(self.normal_weight), "distortion_weight": float(self.distortion_weight),
                "evals": [dataclasses.asdict(r) for r in self.evals], "losses": [float(x) for x in self.losses]}


def _colmap_points(root: str) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """The SfM points of a COLMAP dataset (colmap_initial_points), or None when it has no non-empty points3D file."""
    from . import dataset as D

    files = D.DatasetFiles(root)
    _, _, ext = D._colmap_paths(files)
    if files.find_base_path(f"sparse/0/points3D.{ext}") is None:
        return None
    pos, col = D.colmap_initial_points(root)
    return (pos, col) if pos.shape[0] > 0 else None


def load_dataset(root: str, fmt: str = "auto", max_resolution: Optional[int] = None,
                 eval_split_every: Optional[int] = None):
    """(Dataset, COLMAP SfM points or None) of a dataset directory or zip; host only (no device work)."""
    from .dataset import detect_format, read_dataset

    fmt = detect_format(root) if fmt == "auto" else fmt
    data = read_dataset(root, fmt, max_resolution=max_resolution, eval_split_every=eval_split_every)
    return data, (_colmap_points(root) if fmt == "colmap" else None)


def random_init_bounds(scene) -> Tuple[np.ndarray, np.ndarray]:
    """train_loop.rs:80-90: |e| = length of bounds(0, 0).extent (the half-size), box = bounds(0.25 |e|, |e|)."""
    lo, hi = scene.bounds(0.0, 0.0)
    e = float(np.linalg.norm((hi.astype(np.float32) - lo.astype(np.float32)) / np.float32(2.0)))
    return scene.bounds(e * 0.25, e)


class TrainLoop:
    """The state of one run: splats, trainer, resident views and the device loss log.  `train_scene` drives it; tests
    and tools may call step() / evaluate() themselves (from one thread, on the current stream)."""

    def __init__(self, dataset: Dataset, config: Optional[TrainConfig] = None, *, steps: int, init=None,
                 init_count: int = 10000, sh_degree: int = 3, seed: int = 42, device=None, exchange=None):
        """exchange: the dist.ViewExchange of a data-parallel driver, looked at only to refuse what a run of more than
        one rank cannot do (TrainConfig.check's multi_rank); the loop itself trains single-view."""
        if steps < 0:
            raise ValueError(f"steps must be >= 0, got {steps}")
        # the mean learning rate decays over the run; the refinement RNG takes the run's seed (train_loop.rs:44-46)
        self.config = dataclasses.replace(config or TrainConfig(), total_steps=max(int(steps), 1), seed=int(seed))
        self.config.check(multi_rank=exchange is not None and int(getattr(exchange, "world", 1)) > 1)
        self._prune_at = frozenset(self.config.check_contribution_prune())
        self.dataset = dataset
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.steps = int(steps)
        self.rng = np.random.default_rng(seed)  # random init and eval view choice, as the reference's one StdRng
        if isinstance(init, Splats):
            self.splats = init
        elif init is not None:
            positions, colors = init
            self.splats = Splats.from_point_cloud(positions, colors, sh_degree, self.device)
        else:
            self.splats = Splats.from_random_config(init_count, sh_degree, random_init_bounds(dataset.train), self.rng,
                                                    self.device)
        self.loader = SceneLoader(dataset.train, seed, self.device, use_masks=self.config.use_masks)
        self.trainer = SplatTrainer(self.splats, self.config)
        self.poses = None
        if self.config.pose_opt:
            from .pose import PoseTable

            self.poses = PoseTable(len(self.loader), self.config.lr_pose_rot, self.config.lr_pose_trans,
                                   self.config.pose_reg)
        self.exposures = None
        if self.config.exposure_opt:
            from .exposure import ExposureTable

            self.exposures = ExposureTable(len(self.loader), self.device, self.config.lr_exposure,
                                           self.config.exposure_reg)
        self.bilagrids = None
        if self.config.bilagrid_opt:
            from .bilagrid import BilagridTable

            self.bilagrids = BilagridTable(len(self.loader), self.device, self.config.lr_bilagrid,
                                           self.config.bilagrid_shape, self.config.bilagrid_tv)
        # 3D smoothing filter: the training views' records go to the device once, so that a refresh is launches only.
        # Full-size intrinsics and the dataset's poses, whatever level the downscale schedule trains at and whatever
        # pose_opt has moved: the filter bounds what the stored images can resolve.
        self._filter_views = None
        self._filter_stale, self._filter_at = True, -1  # (the step index the filter was last computed in front of)
        if self.config.filter3d:
            from .filter3d import view_records

            self._filter_views = torch.from_numpy(view_records(dataset.train.views)).to(self.device)
        self.losses = torch.zeros(self.steps, dtype=torch.float32, device=self.device)
        self.done = 0
        self.log = TrainLog(self.steps, np.zeros(0, np.float32), image_bytes=self.loader.total_bytes,
                            background=self.config.background,
                            masked_views=sum(m is not None for m in self.loader.masks),
                            filter3d=bool(self.config.filter3d), densify_by=self.config.densify_by,
                            normal_weight=float(self.config.normal_weight),
                            distortion_weight=float(self.config.distortion_weight))
        # error-driven densification: a host generator of its own picks the views of a score pass (the loader's draw
        # order does not change), and a fixed background colour goes to the device here, once
        self._score_rng, self._score_bg = None, None
        if self.config.densify_by == "error":
            from .compose import as_background

            self._score_rng = np.random.default_rng([int(seed), 0x65727273])
            bg = "black" if self.config.background == "random" else self.config.background
            self._score_bg = as_background(bg, self.device)
        self._t0 = time.perf_counter()
        self._eval_seconds = 0.0
        self._last = (0, 0.0)  # (step, training seconds) of the previous eval row

    def refresh_filter3d(self):
        """Recomputes the 3D filter lengths of the current splats from the dataset's training views (full-size
        intrinsics, the dataset's poses: neither the downscale level nor pose_opt's corrections enter) and hands them to
        the trainer.  Launches only: no upload, no read-back, no synchronisation."""
        from .filter3d import filter3d_rates

        self.trainer.set_filter3d(filter3d_rates(self.splats.means.detach(), self._filter_views,
                                                 variance=self.config.filter3d_variance))
        self._filter_stale, self._filter_at = False, self.done
        self.log.filter3d_refreshes.append(self.done)

    def baked_splats(self) -> Splats:
        """What a renderer should be given: with TrainConfig.filter3d the splats with the current filter baked in
        (Splats.bake_filter3d, a copy; the filter is refreshed first when the count changed since), else the splats
        themselves."""
        if not self.config.filter3d:
            return self.splats
        if self._filter_stale or self.trainer.filter3d is None \
                or int(self.trainer.filter3d.shape[0]) != self.splats.num_splats():
            self.refresh_filter3d()
        return self.splats.bake_filter3d(self.trainer.filter3d)

    def score_errors(self) -> int:
        """One score pass of error-driven densification: densify_error_views distinct training views (0: all of them),
        chosen with a generator of the loop's own, at the loader's current level; each is rendered (the baked splats
        under TrainConfig.filter3d: their rows are the raw splats' rows) in the config's antialiased mode and over its
        background ("random" scores over black, as the evals do), its L1 error map under its loss mask is distributed
        to the splats (error_score.splat_error_scores) and the trainer receives every splat's largest share
        (SplatTrainer.set_densify_scores).  Appends (step, views) to the log's `error_passes` and returns the number of
        views.  Launches only: no upload, no read-back, no synchronisation."""
        from .error_score import splat_error_scores

        total, k = len(self.loader), self.config.densify_error_views
        k = total if k == 0 else min(k, total)
        chosen = sorted(int(i) for i in self._score_rng.choice(total, size=k, replace=False))
        views = [self.loader.view_at(i) for i in chosen]
        self.trainer.sync(self.splats)
        bufs = splat_error_scores(self.baked_splats(), views, antialiased=self.config.antialiased,
                                  background=self._score_bg, use_masks=self.config.use_masks)
        self.trainer.set_densify_scores(bufs.scores("max"))
        self.log.error_passes.append((self.done, k))
        return k

    def step(self):
        """One training iteration on a random view, at the level TrainConfig.downscale_at gives for this step; its loss
        lands in the device log.  With TrainConfig.densify_by = "error" a refining step (SplatTrainer.will_refine) is
        preceded by score_errors().  With TrainConfig.filter3d the 3D filter is recomputed in front of the step (from the
        training views at full size and at the dataset's poses, refresh_filter3d) before the first step, after any step
        that changed the splat count (refinement, contribution prune) and otherwise when the step index is a multiple
        of filter3d_every; no step synchronises because of the filter."""
        if self.done >= self.steps:
            raise RuntimeError(f"the run has {self.steps} steps, all done")
        if self.config.filter3d and (self._filter_stale or (self.done % self.config.filter3d_every == 0
                                                            and self._filter_at != self.done)):
            self.refresh_filter3d()
        factor = self.config.downscale_at(self.done)
        if factor != self.loader.downscale:  # a level switch: launches only (SceneLoader.set_downscale)
            self.loader.set_downscale(factor)
            self.log.downscales.append((self.done, factor))
        if self.config.densify_by == "error" and self.trainer.will_refine():
            self.score_errors()
        # every option that is off hands the step None (or a neutral value): that is the step without the option.  The
        # drawn view's resident depth map (with depth supervision on) and loss mask go with the step where the view has
        # them; views without one train as before.
        i, view, gt = self.loader.next_indexed()
        self.trainer.step(self.splats, view.camera, gt, self.loader.scene_extent,
                          loss_out=self.losses[self.done:self.done + 1],
                          view_index=i if (self.poses is not None or self.exposures is not None
                                           or self.bilagrids is not None) else None,
                          poses=self.poses, exposures=self.exposures, bilagrids=self.bilagrids,
                          gt_depth=self.loader.depth(i) if self.config.depth_weight > 0.0 else None,
                          depth_scale=getattr(view, "depth_scale", 1.0),
                          depth_offset=getattr(view, "depth_offset", 0.0),
                          background=self.config.background, gt_mask=self.loader.mask(i))
        if self.trainer.last_refine is not None:
            self._filter_stale = True  # refinement rebuilt the splats: the filter belongs to the old rows
        if self.done in self._prune_at:
            self.prune_by_contribution()
        self.done += 1

    def prune_by_contribution(self) -> Tuple[int, int]:
        """Measures every splat's contribution over all training views, at the current downscale factor and in the
        config's antialiased mode, keeps the splats prune_mask(min_max=contribution_prune_min) leaves, rebuilds the
        parameters and resets the optimizer state and refinement statistics (SplatTrainer.keep_splats).  Appends
        (step, before, after) to the log's `prunes` and returns (before, after).  Synchronises (one read-back).  With
        TrainConfig.filter3d the contributions are those of the baked splats (what the renderer draws); the rows kept
        are taken from the raw ones."""
        from .contribution import prune_mask, splat_contributions

        self.trainer.sync(self.splats)
        before = self.splats.num_splats()
        c = splat_contributions(self.baked_splats(), self.dataset.train.views, antialiased=self.config.antialiased,
                                downscale=self.loader.downscale)
        keep = torch.nonzero(~prune_mask(c, min_max=self.config.contribution_prune_min)).squeeze(1)
        after = self.trainer.keep_splats(self.splats, keep) if int(keep.numel()) < before else before
        self._filter_stale = self._filter_stale or after != before
        self.log.prunes.append((self.done, before, after))
        return before, after

    def train_viewmats(self) -> List[Tuple[str, np.ndarray]]:
        """(name, row-major 4x4 float32 world-to-camera matrix) of every training view as the run holds it now: the
        dataset's matrix, under its refined twist with pose_opt (updates still pending are not in)."""
        out = []
        for i, v in enumerate(self.dataset.train.views):
            m = np.asarray(v.camera.world_to_local(), dtype=np.float32) if self.poses is None \
                else self.poses.viewmat(i, v.camera).numpy()
            out.append((v.name, m))
        return out

    def evaluate(self, eval_views: Optional[int] = None) -> Tuple[EvalRow, object]:
        """eval_stats on the dataset's eval views, between steps, on this thread and stream (its docstring's rule);
        appends and returns the EvalRow (and the EvalStats).  Always at the eval views' full size, whatever level the
        downscale schedule has the training at: the rows of one run stay comparable.  With TrainConfig.filter3d the
        baked splats are evaluated."""
        from .eval import eval_stats

        if self.dataset.eval is None or not self.dataset.eval.views:
            raise ValueError("the dataset has no eval views")
        torch.cuda.synchronize(self.device)  # the training time up to here is done
        t = time.perf_counter()
        train_s = t - self._t0 - self._eval_seconds
        # evaluated in the mode the splats are trained in; a random training background evaluates over black
        # (with no background and no masked eval view eval_stats is the call without the options)
        bg = "black" if self.config.background == "random" else self.config.background
        stats = eval_stats(self.baked_splats(), self.dataset.eval, eval_views, self.rng,
                           antialiased=self.config.antialiased, background=bg, use_masks=self.config.use_masks)
        loss = float(self.losses[self.done - 1].item()) if self.done > 0 else float("nan")
        dstep, dt = self.done - self._last[0], train_s - self._last[1]
        row = EvalRow(self.done, stats.mean_psnr(), stats.mean_ssim(), self.splats.num_splats(),
                      time.perf_counter() - self._t0, loss, dstep / dt if dstep > 0 and dt > 0 else float("nan"))
        self._last = (self.done, train_s)
        self._eval_seconds += time.perf_counter() - t
        self.log.evals.append(row)
        return row, stats

    def finish(self) -> Tuple[Splats, TrainLog]:
        """Applies the trainer's pending SH steps (the returned splats are current) and the pending pose updates, and
        reads the loss log back.  With TrainConfig.filter3d the returned splats are the baked ones (Splats.bake_filter3d
        under the current filter: what the evals rendered and what a viewer shows correctly); the raw parameters stay at
        `loop.splats` and the filter at `loop.trainer.filter3d`."""
        self.trainer.sync(self.splats)
        self.log.pose_opt = self.poses is not None
        if self.poses is not None:
            self.poses.apply_all()
            self.log.pose_deltas = self.poses.deltas()
        self.log.exposure_opt = self.exposures is not None
        if self.exposures is not None:
            self.log.exposures = self.exposures.exposures()
        self.log.bilagrid_opt = self.bilagrids is not None
        if self.bilagrids is not None:
            self.log.bilagrid_shape = tuple(self.bilagrids.shape)
        self.log.losses = self.losses.cpu().numpy()  # synchronises
        self.log.seconds = time.perf_counter() - self._t0
        self.log.train_seconds = self.log.seconds - self._eval_seconds
        self.log.num_splats = self.splats.num_splats()
        return self.baked_splats(), self.log


def train_scene(dataset: Dataset, config: Optional[TrainConfig] = None, *, steps: int, init=None,
                init_count: int = 10000, sh_degree: int = 3, seed: int = 42, eval_every: int = 0,
                eval_views: Optional[int] = None, on_eval: Optional[Callable] = None,
                device=None, on_finish: Optional[Callable] = None) -> Tuple[Splats, TrainLog]:
    """Trains `dataset.train` for `steps` iterations (train_loop.rs) and returns (current splats, TrainLog).

    `config` is copied with total_steps = steps and seed = seed.  `init`: Splats to start from, or (positions,
    colours) of a point cloud (e.g. load_dataset's COLMAP points), or None for from_random_config(init_count,
    sh_degree) in random_init_bounds(dataset.train).  `eval_every` > 0: eval_stats at step 0, every `eval_every` steps
    and after the last step, on `eval_views` views (all when None) chosen with the run's rng; `on_eval(row, stats)` is
    called after each; `on_finish(loop)` after the run's finish(), with the TrainLoop (its poses, its views)."""
    if eval_every > 0 and (dataset.eval is None or not dataset.eval.views):
        raise ValueError("eval_every > 0 needs a dataset with eval views")
    loop = TrainLoop(dataset, config, steps=steps, init=init, init_count=init_count, sh_degree=sh_degree, seed=seed,
                     device=device)

    def ev():
        row, stats = loop.evaluate(eval_views)
        if on_eval is not None:
            on_eval(row, stats)

    if eval_every > 0:
        ev()
    for i in range(steps):
        loop.step()
        if eval_every > 0 and (loop.done % eval_every == 0 or loop.done == steps):
            ev()
    res = loop.finish()
    if on_finish is not None:
        on_finish(loop)
    return res


# ---------------------------------------------------------------------------- command line
def parse_downscale_schedule(text: str) -> Tuple[Tuple[int, int], ...]:
    """'0:4,3000:2,6000:1' -> ((0, 4), (3000, 2), (6000, 1)); the pairs are validated by TrainConfig."""
    pairs = []
    for item in text.split(","):
        step, sep, factor = item.partition(":")
        try:
            if not sep:
                raise ValueError
            pairs.append((int(step), int(factor)))
        except ValueError:
            raise ValueError(f"--downscale-schedule takes STEP:FACTOR pairs separated by commas, got {item!r}") from None
    return tuple(pairs)


def downscale_schedule_from_args(args) -> Tuple[Tuple[int, int], ...]:
    """The (step, factor) pairs the command line asks for, from either spelling; () when it asks for none.  Raises
    ValueError when both spellings are given or one is malformed."""
    explicit = args.downscale_schedule is not None
    shorthand = args.num_downscales is not None
    if explicit and (shorthand or args.resolution_schedule is not None):
        raise ValueError("--downscale-schedule and --num-downscales / --resolution-schedule are two spellings of one "
                         "option: give one of them")
    if explicit:
        pairs = parse_downscale_schedule(args.downscale_schedule)
    elif shorthand:
        k = args.num_downscales
        every = 3000 if args.resolution_schedule is None else args.resolution_schedule  # splatfacto's default
        if not 0 <= k <= 4 or every < 1:
            raise ValueError("--num-downscales must be 0..4 (factors up to 16) and --resolution-schedule >= 1")
        pairs = tuple((i * every, 2 ** (k - i)) for i in range(k + 1))
    elif args.resolution_schedule is not None:
        raise ValueError("--resolution-schedule needs --num-downscales")
    else:
        return ()
    return TrainConfig(downscale_schedule=pairs).check_downscale_schedule()


def parse_prune_steps(text: str) -> Tuple[int, ...]:
    """'16000,24000' -> (16000, 24000); the steps are validated by TrainConfig."""
    try:
        return tuple(int(x) for x in text.split(","))
    except ValueError:
        raise ValueError(f"--contribution-prune-at takes steps separated by commas, got {text!r}") from None


def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.train_loop",
                                description="train splats on a dataset (NeRF-synthetic or COLMAP)")
    p.add_argument("dataset", help="dataset directory or .zip")
    p.add_argument("--steps", type=int, default=30000)
    cli.add_dataset_options(p)
    p.add_argument("--eval-every", type=int, default=0, help="eval every N steps (0: never)")
    p.add_argument("--eval-views", type=int, default=None, help="eval views per eval (default: all)")
    p.add_argument("--init", default=None, help="start from this .ply instead of the dataset's points / random splats")
    p.add_argument("--init-count", type=int, default=10000, help="random initial splats when there are no points")
    p.add_argument("--sh-degree", type=int, default=3)
    p.add_argument("--seed", type=int, default=42)
    cli.add_export_option(p, "the trained splats")
    cli.add_json_option(p, help="write the eval rows and the loss curve to this file")
    cli.add_antialiased_option(p, "train (and evaluate) in the antialiased mode: opacity compensation of the 2D blur")
    p.add_argument("--pose-opt", action="store_true",
                   help="refine the training views' camera poses beside the splats (eval views are rendered as given)")
    p.add_argument("--export-cameras", default=None, metavar="FILE.json",
                   help="write name and 4x4 world-to-camera matrix of every training view after the run")
    p.add_argument("--exposure-opt", action="store_true",
                   help="fit a per-view affine colour map (exposure / white balance) beside the splats")
    p.add_argument("--export-exposures", default=None, metavar="FILE.json",
                   help="write name and 3x4 exposure map of every training view after the run")
    p.add_argument("--bilagrid-opt", action="store_true",
                   help="fit a per-view bilateral grid (colour maps by pixel position and luminance) beside the splats")
    p.add_argument("--bilagrid-shape", default=None, metavar="GW,GH,GL",
                   help="--bilagrid-opt: the lattice of every view (default 16,16,8)")
    p.add_argument("--bilagrid-tv", type=float, default=TrainConfig.bilagrid_tv, metavar="W",
                   help="--bilagrid-opt: weight of the total-variation prior on the grids")
    p.add_argument("--export-bilagrids", default=None, metavar="FILE.npz",
                   help="write names and grids [V,GL,GH,GW,12] of the training views after the run")
    p.add_argument("--strategy", choices=("default", "mcmc"), default="default",
                   help="how the splat count evolves: clone / split / prune, or MCMC relocation with a fixed budget")
    p.add_argument("--cap-max", type=int, default=TrainConfig.mcmc_cap_max, metavar="N",
                   help="--strategy mcmc: the splat budget")
    p.add_argument("--depth-weight", type=float, default=0.0, metavar="W",
                   help="supervise the rendered depth with the dataset's depth maps, with this weight (0: off)")
    p.add_argument("--depth-weight-final", type=float, default=None, metavar="W",
                   help="move the depth weight exponentially from --depth-weight to this value over the run")
    p.add_argument("--normal-weight", type=float, default=0.0, metavar="W",
                   help="add the depth-normal consistency loss with this weight (0: off)")
    p.add_argument("--normal-from-step", type=int, default=TrainConfig.normal_from_step, metavar="S",
                   help="--normal-weight: the first step that carries the term")
    p.add_argument("--distortion-weight", type=float, default=0.0, metavar="W",
                   help="add the depth-distortion term with this weight (0: off)")
    p.add_argument("--distortion-from-step", type=int, default=TrainConfig.distortion_from_step, metavar="S",
                   help="--distortion-weight: the first step that carries the term")
    p.add_argument("--distortion-mode", choices=("depth", "ndc"), default="depth",
                   help="--distortion-weight: compare camera-space depths, or 2DGS's NDC mapping of them")
    p.add_argument("--distortion-near", type=float, default=TrainConfig.distortion_near, metavar="Z",
                   help="--distortion-mode ndc: the near plane of the mapping")
    p.add_argument("--distortion-far", type=float, default=None, metavar="Z",
                   help="--distortion-mode ndc: the far plane of the mapping (required there)")
    p.add_argument("--depth-mode", choices=("depth", "disparity"), default="depth",
                   help="compare depth / alpha, or alpha / depth (the maps then hold inverse depths)")
    p.add_argument("--downscale-schedule", default=None, metavar="STEP:FACTOR,...",
                   help="coarse-to-fine training: from STEP on, train on the images at 1 / FACTOR (e.g. 0:4,3000:2,6000:1)")
    p.add_argument("--num-downscales", type=int, default=None, metavar="K",
                   help="nerfstudio's spelling: start at 1 / 2^K and double the resolution every --resolution-schedule steps")
    p.add_argument("--resolution-schedule", type=int, default=None, metavar="S",
                   help="--num-downscales: steps between two doublings (default 3000)")
    p.add_argument("--contribution-prune-at", default=None, metavar="STEP,...",
                   help="after each of these steps, drop the splats whose largest blending weight over all training "
                        "views stays below --contribution-prune-min (e.g. 16000,24000)")
    p.add_argument("--contribution-prune-min", type=float, default=TrainConfig.contribution_prune_min, metavar="T",
                   help="--contribution-prune-at: the threshold on the largest blending weight (0: only splats that "
                        "are never composited and never stop a pixel)")
    p.add_argument("--background", default=None, metavar="white|black|random|R,G,B",
                   help="compose the render and the target over this colour in front of the loss and in the evals; "
                        "random draws a colour per step (and evaluates over black)")
    p.add_argument("--no-masks", action="store_true",
                   help="ignore the dataset's loss masks (nerfstudio's mask_path, COLMAP's masks/<image name>.png)")
    p.add_argument("--filter3d", action="store_true",
                   help="train under Mip-Splatting's 3D smoothing filter; evals and --export use the baked splats")
    p.add_argument("--filter3d-every", type=int, default=TrainConfig.filter3d_every, metavar="K",
                   help="--filter3d: recompute the filter every K steps (and whenever the splat count changed)")
    p.add_argument("--densify-by", choices=("grad", "error"), default="grad",
                   help="what refinement clones and splits on: the screen-space gradient statistic, or each splat's "
                        "share of the per-pixel image error over a set of training views")
    p.add_argument("--densify-error-thresh", type=float, default=TrainConfig.densify_error_thresh, metavar="T",
                   help="--densify-by error: densify at this many pixels of full error in a splat's worst view")
    p.add_argument("--densify-error-views", type=int, default=TrainConfig.densify_error_views, metavar="V",
                   help="--densify-by error: training views per score pass (0: all)")
    p.add_argument("--densify-growth", type=float, default=TrainConfig.densify_growth, metavar="G",
                   help="--densify-by error: densify at most this fraction of the splats per refinement")
    p.add_argument("--max-splats", type=int, default=None, metavar="N",
                   help="--densify-by error: never grow beyond this many splats")
    p.add_argument("--revised-opacity", action="store_true",
                   help="give the two splats a clone or split leaves the opacity 1 - sqrt(1 - o) of their source")
    return p


def main(argv=None) -> int:
    import os
    import sys

    p = parser()
    args = p.parse_args(argv)
    try:
        schedule = downscale_schedule_from_args(args)
        prune_at = () if args.contribution_prune_at is None else parse_prune_steps(args.contribution_prune_at)
        from .compose import parse_background
        background = None if args.background is None else parse_background(args.background)
        shape = TrainConfig.bilagrid_shape
        if args.bilagrid_shape is not None:
            try:
                shape = tuple(int(x) for x in args.bilagrid_shape.split(","))
            except ValueError:
                raise ValueError(f"--bilagrid-shape takes GW,GH,GL, got {args.bilagrid_shape!r}") from None
        config = TrainConfig(bilagrid_opt=args.bilagrid_opt, bilagrid_shape=shape, bilagrid_tv=args.bilagrid_tv,
                             antialiased=args.antialiased, pose_opt=args.pose_opt, strategy=args.strategy,
                             mcmc_cap_max=args.cap_max, exposure_opt=args.exposure_opt, depth_weight=args.depth_weight,
                             depth_weight_final=args.depth_weight_final, depth_mode=args.depth_mode,
                             downscale_schedule=schedule, contribution_prune_at=prune_at,
                             contribution_prune_min=args.contribution_prune_min, background=background,
                             use_masks=not args.no_masks, filter3d=args.filter3d, filter3d_every=args.filter3d_every,
                             densify_by=args.densify_by, densify_error_thresh=args.densify_error_thresh,
                             densify_error_views=args.densify_error_views, densify_growth=args.densify_growth,
                             densify_max_splats=args.max_splats, revised_opacity=args.revised_opacity,
                             normal_weight=args.normal_weight, normal_from_step=args.normal_from_step,
                             distortion_weight=args.distortion_weight, distortion_from_step=args.distortion_from_step,
                             distortion_mode=args.distortion_mode, distortion_near=args.distortion_near,
                             distortion_far=args.distortion_far)
        config.check()  # the configuration the run trains with, before the dataset is loaded
    except ValueError as e:
        p.error(str(e))
    if not os.path.exists(args.dataset):
        p.error(f"dataset not found: {args.dataset}")
    if args.steps < 0 or args.eval_every < 0:
        p.error("--steps and --eval-every must be >= 0")
    if args.cap_max < 1:
        p.error("--cap-max must be >= 1")
    if args.init is not None and not os.path.isfile(args.init):
        p.error(f"--init file not found: {args.init}")

    data, points = load_dataset(args.dataset, args.format, args.max_resolution, args.eval_split_every)  # host only
    if not data.train.views:
        print(f"{args.dataset}: the dataset has no training views", file=sys.stderr)
        return 2
    if args.depth_weight > 0 and not any(v.depth is not None for v in data.train.views):
        print(f"{args.dataset}: --depth-weight needs training views with depth maps", file=sys.stderr)
        return 2
    if args.eval_every > 0 and not cli.chosen_views(data, "eval"):
        print(f"{args.dataset}: --eval-every needs eval views (try --eval-split-every K)", file=sys.stderr)
        return 2

    dev = cli.cuda_device()
    from .undistort import undistort_for_cli

    data = undistort_for_cli(data, not args.no_undistort, dev)  # distorted views become pinhole views, once
    init = Splats.from_ply(args.init, dev) if args.init else points

    def on_eval(row, stats):
        print(f"step {row.step}\tpsnr {row.psnr:.4f}\tssim {row.ssim:.6f}\tsplats {row.splats}\t"
              f"{row.iters_per_s:.1f} it/s", flush=True)

    cameras = []

    exposures = []

    grids = []

    def on_finish(loop):
        if loop.bilagrids is not None:
            grids.append(loop.bilagrids.grids())
        if loop.exposures is not None:
            exposures.extend({"name": v.name, "exposure": [[float(x) for x in row] for row in m]}
                             for v, m in zip(loop.dataset.train.views, loop.exposures.matrices()))
        cameras.extend({"name": name, "world_to_camera": [[float(x) for x in row] for row in m]}
                       for name, m in loop.train_viewmats())

    splats, log = train_scene(data, config, steps=args.steps,
                              init=init, init_count=args.init_count,
                              sh_degree=args.sh_degree, seed=args.seed, eval_every=args.eval_every,
                              eval_views=args.eval_views, on_eval=on_eval, device=dev, on_finish=on_finish)
    final = float(log.losses[-1]) if log.steps else float("nan")
    rate = log.steps / log.train_seconds if log.train_seconds > 0 else float("nan")
    print(f"done: {log.steps} steps in {log.seconds:.1f} s ({rate:.1f} it/s), {log.num_splats} splats, "
          f"final loss {final:.6f}, {log.image_bytes / 1e6:.1f} MB of images on the device")
    if args.export:
        cli.export_splats(args.export, splats)
    if args.export_cameras:
        cli.write_json(args.export_cameras, {"pose_opt": bool(args.pose_opt), "cameras": cameras})
    if args.export_exposures:
        if not args.exposure_opt:
            exposures.extend({"name": v.name, "exposure": [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0],
                                                           [0.0, 0.0, 1.0, 0.0]]} for v in data.train.views)
        cli.write_json(args.export_exposures, {"exposure_opt": bool(args.exposure_opt), "views": exposures})
    if args.export_bilagrids:
        from .bilagrid import bilagrid_identity

        names = np.asarray([v.name for v in data.train.views])
        g = grids[0] if grids else bilagrid_identity(config.bilagrid_shape).numpy()[None].repeat(len(names), axis=0)
        with open(args.export_bilagrids, "wb") as f:
            np.savez(f, names=names, grids=g)
    if args.json:
        res = {"dataset": os.path.abspath(args.dataset), "seed": args.seed, "sh_degree": args.sh_degree,
               "antialiased": bool(args.antialiased), "strategy": args.strategy,
               "cap_max": int(args.cap_max) if args.strategy == "mcmc" else None,
               "densify_error_thresh": float(args.densify_error_thresh),
               "densify_error_views": int(args.densify_error_views), "densify_growth": float(args.densify_growth),
               "max_splats": args.max_splats, "revised_opacity": bool(args.revised_opacity)}
        res.update(log.to_json())
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
