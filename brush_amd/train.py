"""Training iteration around the op — what the metric's train iters/s measures.

Mirror of the reference's `SplatTrainer::step` (crates/brush-train/src/train.rs:211-393) and
`refine_splats` (train.rs:395-579; periodic, plain torch tensor ops): render, loss = L1*(1-w) - SSIM*w (train.rs:243-268, ssim.rs:42-101),
backward, screen-space gradient statistics (train.rs:284-316), Adam with eps 1e-15 on the five
parameter groups and the higher-order-SH learning-rate lerp (train.rs:318-359).

The reference builds the loss and the optimizer from Burn tensor ops; here they are the fused HIP
entry points of include/brush_hip.h (brush_l1_ssim_loss, brush_adam_step, brush_refine_stats) called
straight on the op's forward/backward, so one iteration is ≈40 kernel launches and no autograd graph;
with a single view the optimizer step runs inside the backward's last kernel (brush_render_backward_adam).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

from . import _lib
from . import filter3d as F3
from . import mcmc
from . import render as R
from .camera import Camera
from .dist import allreduce_densification_stats
from .gaussian_splats import Splats


@dataclass
class TrainConfig:
    """Defaults of train.rs:19-87 and the UI's learning-rate schedule (panels/load_data.rs:41-71)."""
    warmup_steps: int = 500
    ssim_weight: float = 0.2
    ssim_window_size: int = 11
    lr_mean: float = 1.6e-4
    lr_mean_decay: float = 0.01   # total decay factor over `total_steps`
    total_steps: int = 30000
    lr_coeffs_dc: float = 0.004
    lr_coeffs_sh_scale: float = 20.0
    lr_opac: float = 0.05
    lr_scale: float = 0.01
    lr_rotation: float = 0.002
    # refinement (train.rs:25-53)
    refine_every: int = 100
    max_refine_step: int = 15000
    reset_alpha_value: float = 0.004
    cull_alpha_thresh: float = 0.005
    cull_scale_thresh: float = 5.0
    reset_alpha_every_refine: int = 30
    densify_grad_thresh: float = 0.0002
    densify_size_thresh: float = 0.005
    seed: int = 42
    # The build extensions below are not in the reference.  Which of them train on a single view only, and which make a
    # step take the separate-call optimizer path, is said once, in SplatTrainer.step's docstring.
    # Build extension: deferred Adam of the SH block (include/brush_hip.h: BrushLazySh).  Same parameter values as the
    # eager optimizer, bit for bit; SplatTrainer.sync() brings `splats.sh_coeffs` up to date for readers that do not go
    # through the trainer (Splats.render / to_ply call it themselves).
    deferred_sh_adam: bool = True
    # Build extension: render and backpropagate in the antialiased mode (BRUSH_AUX_ANTIALIASED: opacity compensation of
    # the 2D blur).  There is no antialiased record path (brush_render_backward_records), so a step given an `exchange`
    # raises.  Refinement still prunes on sigmoid(raw_opacity), as gsplat does.
    antialiased: bool = False
    # Build extension: per-view camera-pose refinement (brush_amd/pose.py; gsplat's pose_opt is the model).  Each
    # training view carries a camera-frame twist, stepped by Adam from the view-matrix gradient of the render backward.
    # Learning rates in radians / world units per step; pose_reg pulls the twists back to the dataset's poses (and
    # pins the gauge the scene shares with its cameras).  DESIGN §8 row 9 has the runs these defaults come from.
    pose_opt: bool = False
    lr_pose_rot: float = 1e-3
    lr_pose_trans: float = 5e-4
    pose_reg: float = 1e-6
    # Build extension: per-view exposure compensation (brush_amd/exposure.py; the 3DGS trainer's exposure compensation
    # is the model, gsplat's app_opt covers the same ground).  Each training view carries a 3x4 affine colour map,
    # applied to the render before the loss and stepped by Adam on the device.  lr_exposure decays by the total factor
    # lr_exposure_decay over `total_steps` (formed like the mean rate); exposure_reg pulls the maps back to the identity
    # (and pins the gain the scene shares with its exposures).  Eval views are rendered as given.  DESIGN §8 row 11.
    exposure_opt: bool = False
    lr_exposure: float = 1e-2
    lr_exposure_decay: float = 0.1
    exposure_reg: float = 1e-6
    # Build extension: per-view bilateral grids (brush_amd/bilagrid.py; gsplat's use_bilateral_grid and Wang et al.,
    # "Bilateral Guided Radiance Field Processing", are the models).  Each training view carries a lattice of
    # bilagrid_shape = (GW, GH, GL) affine colour maps, read at (x, y, the pixel's luminance), sliced through the render
    # before the loss and stepped by Adam on the device: what an exposure map cannot express (vignetting, local tone
    # mapping, brightness-dependent colour).  lr_bilagrid decays by the total factor lr_bilagrid_decay over
    # `total_steps` (formed like the exposure rate); bilagrid_tv weighs the total-variation prior that keeps a grid
    # smooth (added to the grid's gradient, not to the reported loss).  2e-3, 0.01 and 10.0 are gsplat's values:
    # hyper-parameter defaults, not measured here.  Not with exposure_opt (a constant grid is the affine map: one colour
    # model per view), densify_by="error" or a multi-rank exchange.  Eval views are rendered as given.  DESIGN §8 row 24.
    bilagrid_opt: bool = False
    bilagrid_shape: Tuple[int, int, int] = (16, 16, 8)
    lr_bilagrid: float = 2e-3
    lr_bilagrid_decay: float = 0.01
    bilagrid_tv: float = 10.0
    # Build extension: how the splat count evolves.  "default": refine_splats (clone / split / prune / opacity reset, the
    # reference's train.rs:395-579).  "mcmc": a fixed budget (brush_amd/mcmc.py; Kheradmand et al. 2024, gsplat's
    # MCMCStrategy): dead splats (opacity <= mcmc_min_opacity) are relocated onto live ones, the count grows by
    # mcmc_growth per refinement up to mcmc_cap_max, every step adds noise of mcmc_noise_lr * lr_mean to the means and
    # the opacity / scale regularisers to the gradients; the optimizer state is kept and opacities are never reset.
    # Same schedule (warmup_steps, refine_every, max_refine_step).
    strategy: str = "default"
    mcmc_cap_max: int = 1_000_000
    mcmc_noise_lr: float = 5e5
    mcmc_min_opacity: float = 0.005
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01
    mcmc_growth: float = 1.05
    # Build extension: depth supervision (brush_amd/depth_loss.py; the 3DGS trainer's depth regulariser and gsplat's
    # depth_loss are the models).  A step given a view's depth map adds depth_weight * mean over all pixels of
    # |rendered - target| to the loss, on depth / alpha ("depth") or alpha / depth ("disparity": the map then holds
    # inverse depths), over the pixels with a measurement and alpha >= depth_alpha_min ("mostly covered": a
    # hyper-parameter default, not a measured number).  The weight goes from depth_weight to depth_weight_final (None:
    # constant) exponentially over `total_steps`, formed like the exposure rate.  0 (the default) is the step without the
    # option, bit for bit.  DESIGN §8 row 12.
    depth_weight: float = 0.0
    depth_weight_final: Optional[float] = None
    depth_mode: str = "depth"
    depth_alpha_min: float = 0.5
    # Build extension: coarse-to-fine training (brush_amd/pyramid.py; nerfstudio's num_downscales / resolution_schedule
    # is the model).  (step, factor) pairs, steps non-negative and strictly increasing, factors 1..16: from `step` on the
    # training loop draws its targets at 1 / factor of their stored size (SceneLoader.set_downscale).  The trainer's step
    # takes its size from the target, so nothing else changes; () (the default) is the run without the option, bit for
    # bit.  DESIGN §8 row 13.
    downscale_schedule: Tuple[Tuple[int, int], ...] = ()
    # Build extension: pruning by rendered contribution (brush_amd/contribution.py; RadSplat is the model).  Steps,
    # non-negative and strictly increasing: after the optimizer update of a listed step the training loop measures every
    # splat's contribution over all training views and drops the splats whose largest blending weight stays below
    # contribution_prune_min (0.01 is RadSplat's value: a hyper-parameter default, not a measured number; 0.0 is the
    # exact rule, "never added and never stopped a pixel", which changes no bit of any training view).  The optimizer
    # state and the refinement statistics are reset as after a refinement.  Driven by train_loop.TrainLoop, not by
    # SplatTrainer.step; not with strategy "mcmc" (a fixed budget relocates instead) nor with a multi-rank exchange.
    # () (the default) is the run without the option, bit for bit.  DESIGN §8 row 15.
    contribution_prune_at: Tuple[int, ...] = ()
    contribution_prune_min: float = 0.01
    # Build extension: background colour and loss masks (brush_amd/compose.py; gsplat's backgrounds / masks and
    # nerfstudio's mask_path are the models).  background: None (the render is compared as it is, premultiplied, against
    # the image's straight RGB(A)), "white", "black", an (r, g, b) tuple, or "random": the render and the target are
    # composed over that colour in front of the loss, the target then being opaque RGB; "random" draws torch.rand(3) per
    # step from a device generator seeded from `seed` (no upload, no synchronisation; evaluates over black), the usual
    # way to keep splats of an RGBA object capture from hiding behind a black background.  use_masks: the training loop
    # hands a view's mask (SceneView.mask, nonzero = keep) to the step, which zeroes the other pixels of both images and
    # of the gradient; the resident depth maps are zeroed under the masks at load, so the depth term skips them too.
    # None with no masked view is the run without the option, launch for launch and bit for bit.  Works on every
    # optimizer path.  DESIGN §8 row 16.
    background: object = None
    use_masks: bool = True
    # Build extension: the 3D smoothing filter of Mip-Splatting (brush_amd/filter3d.py), the world-space half of what
    # `antialiased` is the screen-space half of.  Every splat carries a filter length (SplatTrainer.set_filter3d; the
    # training loop computes it from the training views, brush_filter3d_rates, before the first step, after every step
    # that changed the splat count and every filter3d_every steps); a step renders and backpropagates through the
    # effective log-scales and opacities (brush_filter3d_apply / _backward around the existing forward and backward) and
    # steps the raw parameters.  filter3d_variance: the filter's variance in squared sampling intervals (0.2 is
    # Mip-Splatting's value: a hyper-parameter default, not a measured number).  Refinement, the opacity reset and the
    # prune thresholds keep reading the RAW parameters, as Mip-Splatting's densification does.  Combines with
    # antialiased, background / masks, exposure, pose and depth; not with strategy "mcmc".  False (the default) is the
    # step without the option, launch for launch.  DESIGN §8 row 17.
    filter3d: bool = False
    filter3d_every: int = 100
    filter3d_variance: float = 0.2
    # Build extension: error-driven densification (brush_amd/error_score.py; Rota Bulo et al., "Revising Densification
    # in Gaussian Splatting", ECCV 2024, is the model).  densify_by: "grad" is the reference's rule (mean screen-space
    # gradient norm >= densify_grad_thresh), launch for launch and bit for bit.  "error": refine_splats clones and splits
    # the splats whose score (SplatTrainer.set_densify_scores; the training loop hands it each splat's largest share,
    # over densify_error_views training views, of the per-pixel L1 error distributed by blending weight, in front of
    # every refining step) is >= densify_error_thresh, in units of pixels of full error in the splat's worst view (1.0:
    # a hyper-parameter default, not a measured number); at most ceil(densify_growth * N) of them per refinement, the
    # largest scores first (0.05 is the paper's cap), and never beyond densify_max_splats.  densify_error_views: views
    # per score pass, 0 = every training view (32: an unmeasured default).  Small / large -> clone / split, the prunes and
    # the opacity reset stay as they are; the step then skips the gradient statistics.  revised_opacity (the same
    # paper's correction, gsplat's revised_opacity; under either densify_by): every clone source and split source and
    # the rows appended for them get the opacity 1 - sqrt(1 - o) of the source's post-step opacity o, so that the pair
    # covers what the source covered.  "error" is single-GPU and not with strategy "mcmc", pose_opt or exposure_opt
    # (the score pass would have to render through the refined pose or map).  The defaults are the run without the
    # options, bit for bit.  DESIGN §8 row 18.
    densify_by: str = "grad"
    densify_error_thresh: float = 1.0
    densify_error_views: int = 32
    densify_growth: float = 0.05
    densify_max_splats: Optional[int] = None
    revised_opacity: bool = False
    # Build extension: the depth-normal consistency loss of the surface-oriented trainers (brush_amd/normal_loss.py; 2DGS,
    # GOF, RaDe-GS and PGSR are the models).  From step normal_from_step on (7000 is 2DGS's schedule: a hyper-parameter
    # default, not a measured number) a step adds normal_weight * mean over all pixels of (alpha - Nr . Nd) to the loss:
    # Nr the rendered map of the per-splat normals (their shortest axes, facing the camera), Nd the normal of the surface
    # the rendered depth map implies, over the pixels with alpha >= normal_alpha_min whose four neighbours have it too.
    # Needs no extra data.  The gradient reaches the rotations through the per-splat normals, and everything through the
    # depth map and the alpha channel; the blending weights of Nr are frozen (a replay of the finished forward), and
    # with `poses` the pose receives no gradient from this term's normals (the depth gradient reaches it as depth
    # supervision's does).  The replay's transpose uses float atomics: a trajectory with the term on is NOT bitwise
    # reproducible, in deterministic mode too.  Single-view.  Reads the RAW log-scales under the 3D filter (the shortest
    # axis of Sigma + f^2 I is that of Sigma).  0 (the default) or a step before normal_from_step is the step without the
    # option, same path, bit for bit.  DESIGN §8 row 22.
    normal_weight: float = 0.0
    normal_from_step: int = 7000
    normal_alpha_min: float = 0.5
    # Build extension: the depth-distortion term of the same trainers (brush_amd/distortion.py), the second of their two
    # self-supervised regularisers.  From step distortion_from_step on (3000 is 2DGS's schedule: a hyper-parameter
    # default, not a measured number) a step adds distortion_weight * mean over all pixels of
    # L(p) = sum over pairs of w_i w_j (m_i - m_j)^2 to the loss, w the blending weights of the pixel's entries and m
    # their depths (distortion_mode "depth") or 2DGS's NDC mapping of them ("ndc", with distortion_near and the required
    # distortion_far).  Needs no extra data; masked by gt_mask.  NOTHING IS FROZEN: the gradient reaches means, scales,
    # rotations and opacities through the blending weights and the depths (a replay adds the term's per-record VJP into
    # the render backward's compact rows, brush_render_backward_distortion).  Single-view, separate-call path; refused
    # with `poses` (the pose would get no gradient through the term) and in deterministic mode (no compact rows there);
    # float atomics: a trajectory with the term on is not bitwise reproducible.  0 (the default) or a step before
    # distortion_from_step is the step without the option, same path, bit for bit.  DESIGN §8 row 23.
    distortion_weight: float = 0.0
    distortion_from_step: int = 3000
    distortion_mode: str = "depth"
    distortion_near: float = 0.2
    distortion_far: Optional[float] = None

    def check(self, multi_rank: bool = False):
        """A ValueError naming the first thing wrong with the configuration, before anything touches a dataset or a
        device.  multi_rank: the run is driven with a dist.ViewExchange of more than one rank, which rules out what has
        to see every view on one GPU."""
        from .compose import check_background

        if self.strategy not in ("default", "mcmc"):
            raise ValueError(f"TrainConfig.strategy must be 'default' or 'mcmc', got {self.strategy!r}")
        if self.depth_mode not in ("depth", "disparity"):
            raise ValueError(f"TrainConfig.depth_mode must be 'depth' or 'disparity', got {self.depth_mode!r}")
        if self.depth_weight < 0 or (self.depth_weight_final or 0.0) < 0:
            raise ValueError("TrainConfig.depth_weight / depth_weight_final must be >= 0")
        self.check_normal()
        self.check_distortion()
        self.check_downscale_schedule()
        prune_at = self.check_contribution_prune()
        if prune_at and self.strategy == "mcmc":
            raise ValueError("TrainConfig.contribution_prune_at cannot be combined with strategy='mcmc': a fixed "
                             "budget relocates splats instead of pruning them")
        if prune_at and multi_rank:  # (every rank would have to measure every view)
            raise ValueError("TrainConfig.contribution_prune_at cannot be combined with a multi-rank exchange: pruning "
                             "by contribution is single-GPU")
        self.check_filter3d()
        if self.filter3d and multi_rank:  # (the filter's step is single-view)
            raise ValueError("TrainConfig.filter3d cannot be combined with a multi-rank exchange: the 3D filter is "
                             "single-GPU")
        check_background(self.background)
        self.check_bilagrid(multi_rank)
        self.check_densify()
        if self.densify_by == "error":
            # what the score pass cannot serve, in the order it is refused in
            for on, what in ((self.strategy == "mcmc", "strategy='mcmc': a fixed budget relocates splats instead of "
                                                       "densifying them"),
                             (multi_rank, "a multi-rank exchange: the score pass is single-GPU"),
                             (self.pose_opt, "pose_opt: the score pass would have to render through the refined poses"),
                             (self.exposure_opt, "exposure_opt: the score pass would have to render through the "
                                                 "refined exposure maps"),
                             (self.bilagrid_opt, "bilagrid_opt: the score pass would have to render through the "
                                                 "refined bilateral grids")):
                if on:
                    raise ValueError(f"TrainConfig.densify_by='error' cannot be combined with {what}")

    def check_bilagrid(self, multi_rank: bool = False):
        """A ValueError naming what is wrong with the bilateral-grid fields."""
        from .bilagrid import check_shape

        try:
            check_shape(self.bilagrid_shape)
        except ValueError as e:
            raise ValueError(f"TrainConfig.bilagrid_shape: {e}") from None
        for name in ("lr_bilagrid", "lr_bilagrid_decay", "bilagrid_tv"):
            x = getattr(self, name)
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not (math.isfinite(x) and x >= 0.0):
                raise ValueError(f"TrainConfig.{name} must be finite and >= 0, got {x!r}")
        if self.bilagrid_opt and self.exposure_opt:
            raise ValueError("TrainConfig.bilagrid_opt cannot be combined with exposure_opt: a constant grid is the "
                             "affine map, so one colour model per view")
        if self.bilagrid_opt and multi_rank:
            raise ValueError("TrainConfig.bilagrid_opt cannot be combined with a multi-rank exchange: the grids are "
                             "single-GPU")

    def check_normal(self):
        """A ValueError naming what is wrong with the normal-consistency fields."""
        w, s, a = self.normal_weight, self.normal_from_step, self.normal_alpha_min
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"TrainConfig.normal_weight must be finite and >= 0, got {w!r}")
        if isinstance(s, bool) or not isinstance(s, int) or s < 0:
            raise ValueError(f"TrainConfig.normal_from_step must be an integer >= 0, got {s!r}")
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not (math.isfinite(a) and a > 0.0):
            raise ValueError(f"TrainConfig.normal_alpha_min must be finite and > 0, got {a!r}")

    def check_distortion(self):
        """A ValueError naming what is wrong with the depth-distortion fields."""
        from .distortion import distortion_config

        w, s = self.distortion_weight, self.distortion_from_step
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"TrainConfig.distortion_weight must be finite and >= 0, got {w!r}")
        if isinstance(s, bool) or not isinstance(s, int) or s < 0:
            raise ValueError(f"TrainConfig.distortion_from_step must be an integer >= 0, got {s!r}")
        if w > 0.0 and self.pose_opt:
            raise ValueError("TrainConfig.distortion_weight cannot be combined with pose_opt: the pose would get no "
                             "gradient through the term")
        try:
            distortion_config(self.distortion_mode, self.distortion_near, self.distortion_far)
        except ValueError as e:
            raise ValueError(f"TrainConfig.distortion_mode / distortion_near / distortion_far: {e}") from None

    def check_densify(self):
        """A ValueError naming what is wrong with the densification fields."""
        def number(x):
            return not isinstance(x, bool) and isinstance(x, (int, float))

        if self.densify_by not in ("grad", "error"):
            raise ValueError(f"TrainConfig.densify_by must be 'grad' or 'error', got {self.densify_by!r}")
        t, v, g, m = self.densify_error_thresh, self.densify_error_views, self.densify_growth, self.densify_max_splats
        if not number(t) or not (math.isfinite(t) and t >= 0.0):
            raise ValueError(f"TrainConfig.densify_error_thresh must be finite and >= 0, got {t!r}")
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"TrainConfig.densify_error_views must be an integer >= 0, got {v!r}")
        if not number(g) or not 0.0 < g <= 1.0:  # (a NaN fails too)
            raise ValueError(f"TrainConfig.densify_growth must be in (0, 1], got {g!r}")
        if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 0):
            raise ValueError(f"TrainConfig.densify_max_splats must be None or an integer >= 0, got {m!r}")

    def check_filter3d(self):
        """A ValueError naming what is wrong with the filter3d fields or their combination with the strategy."""
        e, v = self.filter3d_every, self.filter3d_variance
        if isinstance(e, bool) or not isinstance(e, int) or e < 1:
            raise ValueError(f"TrainConfig.filter3d_every must be an integer >= 1, got {e!r}")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"TrainConfig.filter3d_variance must be finite and >= 0, got {v!r}")
        if self.filter3d and self.strategy == "mcmc":
            raise ValueError("TrainConfig.filter3d cannot be combined with strategy='mcmc': relocation and the "
                             "regularisers act on the raw scales and opacities")

    def check_contribution_prune(self) -> Tuple[int, ...]:
        """contribution_prune_at as a tuple of ints, or a ValueError naming what is wrong with the two fields."""
        steps = []
        at = self.contribution_prune_at
        if not isinstance(at, (tuple, list)):
            raise ValueError(f"TrainConfig.contribution_prune_at holds a tuple of steps, got {at!r}")
        for x in at:
            if isinstance(x, bool) or not isinstance(x, (int, float)) or int(x) != x:
                raise ValueError(f"TrainConfig.contribution_prune_at holds integer steps, got {x!r}")
            if int(x) < 0:
                raise ValueError(f"TrainConfig.contribution_prune_at: steps must be >= 0, got {int(x)}")
            if steps and int(x) <= steps[-1]:
                raise ValueError(f"TrainConfig.contribution_prune_at: steps must be strictly increasing, got {int(x)} "
                                 f"after {steps[-1]}")
            steps.append(int(x))
        t = self.contribution_prune_min
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0.0 <= float(t) <= 1.0:
            raise ValueError(f"TrainConfig.contribution_prune_min must be in [0, 1], got {t!r}")
        return tuple(steps)

    def check_downscale_schedule(self) -> Tuple[Tuple[int, int], ...]:
        """The schedule as a tuple of (int step, int factor), or a ValueError naming what is wrong with it."""
        from .pyramid import MAX_FACTOR

        pairs = []
        for p in self.downscale_schedule:
            if not isinstance(p, (tuple, list)) or len(p) != 2 or any(isinstance(x, bool) or int(x) != x for x in p):
                raise ValueError(f"TrainConfig.downscale_schedule holds (step, factor) pairs of integers, got {p!r}")
            step, factor = int(p[0]), int(p[1])
            if step < 0:
                raise ValueError(f"TrainConfig.downscale_schedule: steps must be >= 0, got {step}")
            if not 1 <= factor <= MAX_FACTOR:
                raise ValueError(f"TrainConfig.downscale_schedule: factors must be 1..{MAX_FACTOR}, got {factor}")
            if pairs and step <= pairs[-1][0]:
                raise ValueError(f"TrainConfig.downscale_schedule: steps must be strictly increasing, got {step} after "
                                 f"{pairs[-1][0]}")
            pairs.append((step, factor))
        return tuple(pairs)

    def downscale_at(self, step: int) -> int:
        """The factor of the last pair of downscale_schedule with pair.step <= step; 1 when there is none."""
        factor = 1
        for s, f in self.downscale_schedule:
            if s > step:
                break
            factor = int(f)
        return factor


@dataclass
class RefineStats:
    """train.rs:95-101"""
    num_split: int
    num_cloned: int
    num_transparent_pruned: int
    num_scale_pruned: int


def quaternion_vec_multiply(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """train.rs:140-177, term by term (quaternions as (w, x, y, z))."""
    qw, qx, qy, qz = q[:, 0:1], q[:, 1:2], q[:, 2:3], q[:, 3:4]
    vx, vy, vz = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    t1 = qw * vx + qy * vz - qz * vy
    t2 = qw * vy - qx * vz + qz * vx
    t3 = qw * vz + qx * vy - qy * vx
    t4 = qx * vx + qy * vy + qz * vz
    rx = vx + (qw * t1 + qx * t4 - qy * t3 + qz * t2) * 2.0
    ry = vy + (qw * t2 - qx * t3 + qy * t4 + qz * t1) * 2.0
    rz = vz + (qw * t3 + qx * t2 - qy * t1 + qz * t4) * 2.0
    return torch.cat([rx, ry, rz], dim=1)


def densify_candidates(scores: torch.Tensor, n: int, thresh: float, growth: float,
                       max_splats: Optional[int] = None) -> torch.Tensor:
    """A boolean [N] tensor, True where a splat is densified under TrainConfig.densify_by = "error": score >= thresh (a
    NaN never passes), and when more than min(ceil(growth n), max_splats - n), clamped at 0, pass, the largest by score
    among them, ties broken by lower index.  `n`: the current splat count, N.  Pure torch; works on CPU tensors and
    never synchronises a device."""
    n = int(n)
    if scores.dim() != 1 or int(scores.shape[0]) != n:
        raise ValueError(f"scores must be a [N] = [{n}] tensor, got {tuple(scores.shape)}")
    budget = int(math.ceil(float(growth) * n))
    if max_splats is not None:
        budget = min(budget, int(max_splats) - n)
    budget = min(max(budget, 0), n)
    passed = scores >= thresh
    key = torch.where(passed, scores.to(torch.float64), torch.full_like(scores, -math.inf, dtype=torch.float64))
    order = torch.sort(key, descending=True, stable=True).indices  # stable: among equals the lower index comes first
    mask = torch.zeros(n, dtype=torch.bool, device=scores.device)
    mask[order[:budget]] = passed[order[:budget]]
    return mask


def revised_opacity(raw: torch.Tensor) -> torch.Tensor:
    """logit(1 - sqrt(1 - sigmoid(raw))): the raw opacity of each of the two splats a clone or a split leaves, such that
    the pair covers what the source covered, 1 - (1 - o')^2 = o ("Revising Densification in Gaussian Splatting";
    gsplat's revised_opacity).  Written without the cancellations: 1 - o = sigmoid(-raw), r = sqrt(1 - o),
    o' = o / (1 + r), logit(o') = log(o' / r)."""
    r = torch.sqrt(torch.sigmoid(-raw))
    return torch.log(torch.sigmoid(raw) / (1.0 + r) / r)


def l1_ssim_loss(pred: torch.Tensor, gt: torch.Tensor, ssim_weight: float, window: int = 11,
                 grad_scale: float = 1.0, out: Optional[torch.Tensor] = None):
    """(loss [1] device tensor, d loss / d pred [h,w,4]) through brush_l1_ssim_loss.  A torch.uint8 `gt` (a view's
    image as decoded, kept on the device) goes to brush_l1_ssim_loss_gt and is read as b / 255 in the kernels: the
    result is bitwise that of the float32 target u8 / 255.  Other dtypes are converted with .float().
    `out`: optional contiguous float32 [1] device tensor on pred's device to write the loss into (e.g. one element of a
    preallocated per-step log); it is also the returned loss tensor."""
    assert pred.is_cuda and gt.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    h, w = int(pred.shape[0]), int(pred.shape[1])
    if tuple(pred.shape) != (h, w, 4) or tuple(gt.shape[:2]) != (h, w) or gt.shape[2] not in (3, 4):
        raise ValueError(f"pred must be [h,w,4] and gt [h,w,3|4], got {tuple(pred.shape)} / {tuple(gt.shape)}")
    if out is not None and (tuple(out.shape) != (1,) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != pred.device):
        raise ValueError("out must be a contiguous float32 [1] tensor on pred's device")
    u8 = gt.dtype == torch.uint8
    pred, gt = pred.contiguous().float(), (gt.contiguous() if u8 else gt.contiguous().float())
    l = _lib.lib()
    nbytes = _lib.size_query("brush_loss_workspace_size", w, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device) if out is None else out
    v_pred = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        stream = _lib.current_stream()
        if u8:
            _lib.check(l.brush_l1_ssim_loss_gt(pred.data_ptr(), gt.data_ptr(), _lib.EVAL_GT_U8, w, h, int(gt.shape[2]),
                                               float(ssim_weight), int(window), float(grad_scale), loss.data_ptr(),
                                               v_pred.data_ptr(), ws.data_ptr(), nbytes, stream),
                       "brush_l1_ssim_loss_gt")
        else:
            _lib.check(l.brush_l1_ssim_loss(pred.data_ptr(), gt.data_ptr(), w, h, int(gt.shape[2]), float(ssim_weight),
                                            int(window), float(grad_scale), loss.data_ptr(), v_pred.data_ptr(),
                                            ws.data_ptr(), nbytes, stream),
                       "brush_l1_ssim_loss")
    return loss, v_pred


def optimizer_path(exchange: bool, grad_sync: bool, fused_backward: bool, mcmc: bool, depth: bool,
                   filter3d: bool) -> str:
    """Which way a step's gradients reach Adam, from what the step was given (depth: an active depth term or an active
    normal-consistency term, which hands the backward a depth gradient too; filter3d: a
    3D filter is set).  "records": the views' gradient records are exchanged and reduced into Adam (brush_amd.dist).
    "fused": Adam runs inside the backward's last kernel (brush_render_backward_adam[_pose]).  "separate": the dense
    backward, then brush_adam_step; what needs the dense gradients between the two (grad_sync, the mcmc regularisers,
    the 3D filter's VJP) or a backward the fused kernel does not have (the depth gradient) forces it.  The first two
    step only the SH blocks of the splats the view touches, so only they defer the rest (TrainConfig.deferred_sh_adam).
    """
    if exchange:
        return "records"
    if grad_sync or mcmc or depth or filter3d or not fused_backward:
        return "separate"
    return "fused"


class SplatTrainer:
    filter3d: Optional[torch.Tensor] = None  # the 3D filter lengths [N] of set_filter3d, or None
    densify_scores: Optional[torch.Tensor] = None  # the scores [N] of set_densify_scores, until a refinement takes them

    def __init__(self, splats: Splats, config: TrainConfig | None = None):
        self.config = config or TrainConfig()
        self.config.check()
        self.filter3d = None
        self.densify_scores = None
        self._bg_rng, self._bg_fixed = None, {}  # "random"'s device generator; the fixed colours' device tensors
        dev = splats.means.device
        assert dev.type == "cuda", "brush_amd has no CPU path: the splats must live on the GPU"
        self.iter = 0
        self._reset(splats.num_splats(), int(splats.sh_coeffs.shape[1]), dev)
        self.fused_backward = True  # single view: brush_render_backward_adam instead of backward + brush_adam_step
        # rotation/|rotation| left by the previous fused backward, valid only for the very Parameter object the
        # trainer updated (identity + storage + autograd version); see invalidate_cached_rotation().
        self.invalidate_cached_rotation()
        self.last_refine = None  # RefineStats, or mcmc.McmcRefineStats with strategy "mcmc"
        self.rng = torch.Generator(device=dev)
        self.rng.manual_seed(self.config.seed)
        splats.lazy_sh_owner = self

    def invalidate_cached_rotation(self):
        """Call after writing `splats.rotation` behind autograd's back (`.data.copy_(ckpt)`, an external
        kernel): such writes do not bump the tensor version the cache key watches.  In-place ops on the
        Parameter itself, replacing the Parameter and refine_splats are detected without it."""
        self._norm_rot, self._norm_rot_key, self._norm_rot_owner = None, None, None

    def _rotation_key(self, splats: Splats):
        return (splats.rotation.data_ptr(), splats.num_splats(), splats.rotation._version)

    def _take_rotation(self, splats: Splats, stream) -> torch.Tensor:
        """rotation / |rotation|, which Splats::render feeds the op (gaussian_splats.rs:174-175): what the previous
        update left (_store_rotation) when that was for this very rotation, else recomputed.  Empties the cache."""
        if self._norm_rot is not None and self._norm_rot_key == self._rotation_key(splats) \
                and self._norm_rot_owner is splats.rotation:
            norm_rot = self._norm_rot
        else:
            quats = splats.rotation.detach()
            norm_rot = torch.empty_like(quats)
            with torch.cuda.device(quats.device):
                _lib.check(_lib.lib().brush_normalize_quats(quats.data_ptr(), norm_rot.data_ptr(), quats.shape[0],
                                                            stream), "brush_normalize_quats")
        self.invalidate_cached_rotation()
        return norm_rot

    def _store_rotation(self, splats: Splats, norm_rot: torch.Tensor):
        """Keeps the rotation / |rotation| an update kernel wrote for the rotation it has just stepped in place."""
        self._norm_rot, self._norm_rot_key, self._norm_rot_owner = norm_rot, self._rotation_key(splats), splats.rotation

    def set_filter3d(self, filter: Optional[torch.Tensor]):
        """Sets (None: clears) the 3D smoothing filter the next steps train under: a contiguous float32 [N] device
        tensor of filter lengths, one per splat (filter3d.filter3d_rates), kept by reference.  With a filter set a step
        takes the separate-call path whatever `fused_backward` says.  The filter is not resized when refinement changes
        the count: the next step then refuses to run until a filter of the new length is set."""
        if filter is not None:
            if self.config.strategy == "mcmc":
                raise ValueError("the 3D filter cannot be combined with strategy='mcmc'")
            if not isinstance(filter, torch.Tensor) or filter.dim() != 1 or filter.dtype != torch.float32 \
                    or not filter.is_cuda or not filter.is_contiguous():
                raise ValueError("the 3D filter must be a contiguous float32 [N] tensor on the GPU")
            filter = filter.detach()
        self.filter3d = filter

    def set_densify_scores(self, scores: Optional[torch.Tensor]):
        """Hands the next refinement its scores under TrainConfig.densify_by = "error" (None: clears them): a float32
        [N] tensor on the splats' device, one score per splat (error_score.ErrorScoreBuffers.scores), kept by
        reference.  The refinement consumes and clears them; one that finds none, or scores of another length than the
        splat count, refuses to run."""
        if scores is not None:
            if not isinstance(scores, torch.Tensor) or scores.dim() != 1 or scores.dtype != torch.float32 \
                    or not scores.is_cuda:
                raise ValueError("the densification scores must be a float32 [N] tensor on the GPU")
            scores = scores.detach()
        self.densify_scores = scores

    def _check_densify_scores(self, n: int):
        if self.densify_scores is None:
            raise ValueError("TrainConfig.densify_by is 'error' but the trainer has no scores for this refinement: call "
                             "set_densify_scores first (train_loop.TrainLoop does)")
        if int(self.densify_scores.shape[0]) != n:
            raise ValueError(f"stale densification scores: {int(self.densify_scores.shape[0])} scores for {n} splats; "
                             "set them for the current splats (set_densify_scores)")

    def will_refine(self) -> bool:
        """Whether the coming step ends in a refinement (train.rs:361: past the warm-up, before max_refine_step, one
        step after every multiple of refine_every)."""
        c = self.config
        return self.iter < c.max_refine_step and self.iter >= c.warmup_steps and self.iter % c.refine_every == 1

    LAZY_TABLE_ROWS = 2048

    def _lazy_state(self, splats: Splats, n: int, ncoef: int) -> Optional[_lib.BrushLazySh]:
        """The BrushLazySh of this step (optimizer time self.opt_time), or None when the SH block is stepped eagerly:
        rows of whole 16-byte chunks only (SH degree 1 or 3), n a multiple of 4."""
        c = self.config
        if not c.deferred_sh_adam or (3 * ncoef) % 4 != 0 or n % 4 != 0 or n == 0:
            return None
        dev = splats.means.device
        if self._lazy is not None and self.opt_time + 1 > self._lazy.base + self._lazy.capacity:
            self.sync(splats)   # the table ends here: bring every block to opt_time, then start a new table
            self._lazy = None
        if self._lazy is None:
            import numpy as np
            rows = np.empty((self.LAZY_TABLE_ROWS, 4), dtype=np.float32)
            _lib.check(_lib.lib().brush_lazy_sh_fill_table(0.9, 0.999, c.lr_coeffs_dc, 1.0 / c.lr_coeffs_sh_scale,
                                                           self.opt_time, self.LAZY_TABLE_ROWS, rows.ctypes.data),
                       "brush_lazy_sh_fill_table")
            table = torch.from_numpy(rows).to(dev)
            sh_time = torch.full((n,), self.opt_time, dtype=torch.int32, device=dev)
            z = _lib.BrushLazySh()
            z.table, z.base, z.capacity = table.data_ptr(), self.opt_time, self.LAZY_TABLE_ROWS
            z.sh_time = sh_time.data_ptr()
            z.beta1, z.beta2, z.epsilon = 0.9, 0.999, 1e-15
            self._lazy, self._lazy_bufs = z, (sh_time, table)
        z = self._lazy
        z.now = self.opt_time
        z.sh_moment1 = self.moment1.data_ptr() + 4 * 11 * n
        z.sh_moment2 = self.moment2.data_ptr() + 4 * 11 * n
        return z

    @torch.no_grad()
    def sync(self, splats: Splats):
        """Applies every pending SH step (brush_lazy_sh_flush): afterwards splats.sh_coeffs and the moments are what the
        eager optimizer holds.  No-op when nothing is pending."""
        if self._lazy is None or not self._lazy_pending:
            return
        sh = splats.sh_coeffs.detach()
        n, ncoef = sh.shape[0], sh.shape[1]
        z = self._lazy
        z.now = self.opt_time
        with torch.cuda.device(sh.device):
            _lib.check(_lib.lib().brush_lazy_sh_flush(C.byref(z), sh.data_ptr(), n, R.sh_degree_from_coeffs(ncoef),
                                                      _lib.current_stream(sh.device)),
                       "brush_lazy_sh_flush")
        self._lazy_pending = False

    def _reset_stats(self, n: int, dev):
        """reset_stats (train.rs:201-204): the screen-space gradient statistics refinement decides on."""
        self.grad_2d_accum = torch.zeros(n, device=dev)
        self.xy_grad_counts = torch.zeros(n, device=dev)

    def _reset(self, n: int, ncoef: int, dev):
        """reset_stats + `self.optim = self.opt_config.init()` (train.rs:201-204,559-563): the state of a trainer of `n`
        splats that has not stepped yet, at construction and after every change of the count."""
        # deferred Adam of the SH block: per-splat optimizer time of the stored block, table of per-step constants
        self._lazy: Optional[_lib.BrushLazySh] = None
        self._lazy_bufs = None      # (sh_time, table) tensors the struct points into
        self._lazy_pending = False  # some block may be behind opt_time
        self._reset_stats(n, dev)
        # Adam moments of the five groups, [means|log_scales|quats|raw_opac|sh] (AdamConfig of train.rs:184)
        self.moment1 = torch.zeros(n * (11 + 3 * ncoef), device=dev)
        self.moment2 = torch.zeros(n * (11 + 3 * ncoef), device=dev)
        self.opt_time = 0  # Adam's per-parameter step count

    @torch.no_grad()
    def refine_splats(self, splats: Splats, pre_step: dict) -> RefineStats:
        """train.rs:395-579.  `splats` holds the post-step parameters and is rebuilt in place
        (clone / split / prune / opacity reset); `pre_step` holds the parameters before the optimizer
        step (clones and split positions are taken from those).  As in the reference, the shrunken
        scale and the re-sampled mean of a split *source* are computed on temporaries that are dropped
        (train.rs:402,500-526 vs 528): only the appended splats change."""
        c = self.config
        dev = splats.means.device
        post = {"means": splats.means.detach(), "rotation": splats.rotation.detach(), "sh": splats.sh_coeffs.detach(),
                "opac": splats.raw_opacity.detach(), "scales": splats.log_scales.detach()}
        if c.densify_by == "error":  # the scores of set_densify_scores take the gradient statistic's place
            n = int(post["means"].shape[0])
            self._check_densify_scores(n)
            big_grad = densify_candidates(self.densify_scores, n, c.densify_error_thresh, c.densify_growth,
                                          c.densify_max_splats)
            self.densify_scores = None
        else:
            grads = self.grad_2d_accum / self.xy_grad_counts.clamp_min(1.0)
            big_grad = grads >= c.densify_grad_thresh
        small = post["scales"].exp().max(dim=1).values < c.densify_size_thresh
        app = {k: [] for k in post}
        clone_inds = torch.nonzero(small & big_grad).squeeze(1)
        if clone_inds.numel() > 0:
            for k in post:
                app[k].append(pre_step[k][clone_inds])
        split_inds = torch.nonzero(~small & big_grad).squeeze(1)
        ns = int(split_inds.numel())
        if ns > 0:
            cur_rots = post["rotation"][split_inds]
            cur_scale = post["scales"][split_inds].exp()
            app["rotation"].append(cur_rots)
            app["sh"].append(post["sh"][split_inds])
            app["opac"].append(post["opac"][split_inds])
            app["scales"].append((cur_scale / 1.6).log())
            cur_means = pre_step["means"][split_inds]
            # first sample: the source's re-sampled mean, dropped by the reference (kept for the RNG stream)
            torch.randn((ns, 3), generator=self.rng, device=dev)
            samples_new = quaternion_vec_multiply(cur_rots, torch.randn((ns, 3), generator=self.rng, device=dev) * 0.5
                                                  * cur_scale)
            app["means"].append(cur_means + samples_new)
        new = {k: (torch.cat([post[k]] + app[k], 0) if app[k] else post[k]) for k in post}
        if c.revised_opacity and (clone_inds.numel() > 0 or ns > 0):
            # sources and the rows appended for them (clones, then splits: the order of `sources`), from the sources'
            # post-step opacities (`new` is a fresh tensor here: something was appended)
            sources = torch.cat([clone_inds, split_inds])
            revised = revised_opacity(post["opac"][sources])
            new["opac"][sources] = revised
            new["opac"][post["opac"].shape[0]:] = revised
        start = new["means"].shape[0]

        def prune(mask):
            keep = torch.nonzero(~mask).squeeze(1)
            if keep.numel() < mask.numel():
                for k in new:
                    new[k] = new[k][keep]

        prune(torch.sigmoid(new["opac"]) < c.cull_alpha_thresh)
        alpha_pruned = start - new["means"].shape[0]
        prune(new["scales"].exp().max(dim=1).values > c.cull_scale_thresh)
        scale_pruned = start - new["means"].shape[0]  # cumulative, as train.rs:551
        if (self.iter // c.refine_every) % c.reset_alpha_every_refine == 0:
            new["opac"] = torch.zeros_like(new["opac"]) + math.log(c.reset_alpha_value / (1.0 - c.reset_alpha_value))
        splats.replace_parameters(new["means"], new["sh"], new["rotation"], new["opac"], new["scales"])
        self._reset(splats.num_splats(), int(splats.sh_coeffs.shape[1]), dev)
        return RefineStats(ns, int(clone_inds.numel()), alpha_pruned, scale_pruned)

    @torch.no_grad()
    def keep_splats(self, splats: Splats, keep: torch.Tensor) -> int:
        """Rebuilds `splats` in place from its rows `keep` (a 1-D index tensor on the splats' device) and resets the
        optimizer state and the refinement statistics, exactly as refine_splats does after a count change.  Returns the
        new count.  Call between steps, after sync()."""
        self.sync(splats)
        dev = splats.means.device
        keep = keep.to(device=dev, dtype=torch.int64)
        splats.replace_parameters(**{name: getattr(splats, name).detach()[keep] for name in
                                     ("means", "rotation", "sh_coeffs", "raw_opacity", "log_scales")})
        self._reset(splats.num_splats(), int(splats.sh_coeffs.shape[1]), dev)
        self.invalidate_cached_rotation()
        return splats.num_splats()

    def _decayed(self, start: float, factor: float) -> float:
        """`start` on its way to start * factor, exponentially over config.total_steps, at this iteration."""
        return start * (factor ** (1.0 / self.config.total_steps)) ** self.iter

    def _lr_mean(self, scene_extent: float) -> float:
        return self._decayed(self.config.lr_mean, self.config.lr_mean_decay) * scene_extent

    def _background(self, background, dev) -> Optional[torch.Tensor]:
        """step's `background` as the float32 [3] device tensor brush_compose_* reads: a tensor is taken as it is, a
        fixed colour is uploaded once and kept, "random" is drawn on the device from a generator seeded from
        config.seed."""
        from .compose import as_background, check_background

        if background is None or isinstance(background, torch.Tensor):
            return as_background(background, dev)
        background = check_background(background)
        if background == "random":
            if self._bg_rng is None:
                self._bg_rng = torch.Generator(device=dev)
                self._bg_rng.manual_seed(self.config.seed)
            return as_background("random", dev, self._bg_rng)
        if background not in self._bg_fixed:
            self._bg_fixed[background] = as_background(background, dev)
        return self._bg_fixed[background]

    def _lr_exposure(self) -> float:
        return self._decayed(self.config.lr_exposure, self.config.lr_exposure_decay)

    def _lr_bilagrid(self) -> float:
        return self._decayed(self.config.lr_bilagrid, self.config.lr_bilagrid_decay)

    def _depth_weight(self) -> float:
        c = self.config
        if c.depth_weight_final is None or c.depth_weight <= 0.0 or c.depth_weight_final <= 0.0:
            return c.depth_weight  # (an exponential ramp needs two positive ends)
        return self._decayed(c.depth_weight, c.depth_weight_final / c.depth_weight)

    def _normal_active(self) -> bool:
        """Whether the coming step carries the normal-consistency term (TrainConfig.normal_weight / normal_from_step)."""
        return self.config.normal_weight > 0.0 and self.iter >= self.config.normal_from_step

    def _distortion_active(self) -> bool:
        """Whether the coming step carries the depth-distortion term (TrainConfig.distortion_weight /
        distortion_from_step)."""
        return self.config.distortion_weight > 0.0 and self.iter >= self.config.distortion_from_step

    def _check_step(self, grad_sync, exchange, view_index, poses, exposures, gt_depth, bilagrids=None):
        """Refuses the combinations of step's arguments and the configuration that no path serves, before anything is
        touched (neither the trainer's state nor the splats are looked at)."""
        c = self.config
        if c.filter3d and self.filter3d is None:
            raise ValueError("TrainConfig.filter3d is set but the trainer has no filter: call set_filter3d first "
                             "(train_loop.TrainLoop does)")
        if exchange is not None or grad_sync is not None:
            # what is single-view, in the order it is refused in; a new single-view option is one more row
            for on, what in ((self.filter3d is not None, "the 3D filter"),
                             (gt_depth is not None, "depth supervision"),
                             (self._normal_active(), "the normal-consistency term"),
                             (self._distortion_active(), "the distortion term (TrainConfig.distortion_weight)"),
                             (c.strategy == "mcmc", "the mcmc strategy"),
                             (poses is not None, "pose refinement"),
                             (exposures is not None, "exposure compensation"),
                             (bilagrids is not None, "the bilateral grids")):
                if on:
                    raise ValueError(f"{what} is single-view: it cannot be combined with exchange / grad_sync")
        if bilagrids is not None and exposures is not None:
            raise ValueError("bilagrids cannot be combined with exposures: a constant grid is the affine map, so one "
                             "colour model per view")
        if self._distortion_active():
            # what the term's gradient replay cannot serve
            for on, what in ((poses is not None, "pose refinement (`poses`): the pose would get no gradient through "
                                                 "the term"),
                             (R.deterministic_default(), "deterministic mode: it keeps one gradient row per "
                                                         "intersection, the term adds into per-splat rows")):
                if on:
                    raise ValueError(f"TrainConfig.distortion_weight cannot be combined with {what}")
        if c.densify_by == "error":
            # what the score pass cannot serve (TrainConfig.check refuses the configured forms of the same rows)
            for on, what in ((c.strategy == "mcmc", "the mcmc strategy"),
                             (exchange is not None or grad_sync is not None, "exchange / grad_sync"),
                             (poses is not None, "pose refinement"),
                             (exposures is not None, "exposure compensation"),
                             (bilagrids is not None, "the bilateral grids")):
                if on:
                    raise ValueError(f"densify_by='error' cannot be combined with {what}")
        for name, table in (("poses", poses), ("exposures", exposures), ("bilagrids", bilagrids)):
            if table is not None and view_index is None:
                raise ValueError(f"{name} needs view_index")
        if exchange is not None and grad_sync is not None:
            raise ValueError("exchange and grad_sync are two ways to sum the views' gradients: give one of them")
        if c.antialiased and exchange is not None:
            raise ValueError("antialiased training has no data-parallel record path (brush_render_backward_records)")

    def _loss(self, pred, gt_image, batch_views, loss_out, view_index, exposures, background, gt_mask, bilagrids=None):
        """(loss [1], d loss / d pred at the raw render `pred`): exposure map or bilateral grid, composition over the
        background and under the mask, L1 / SSIM, and the same stages backwards, each only with its option."""
        from .compose import compose_backward, compose_forward

        c = self.config
        bg = None if background is None else self._background(background, pred.device)
        compose = bg is not None or gt_mask is not None
        seen = pred if exposures is None else exposures.forward(view_index, pred)
        if bilagrids is not None:  # (never beside exposures: _check_step)
            seen = bilagrids.forward(view_index, pred)
        target = gt_image
        if compose:
            seen, target = compose_forward(seen, gt_image, background=bg, mask=gt_mask)
        loss, v_pred = l1_ssim_loss(seen, target, c.ssim_weight, c.ssim_window_size, 1.0 / batch_views, out=loss_out)
        if compose:
            compose_backward(v_pred, background=bg, mask=gt_mask, out=v_pred)
        if exposures is not None:  # the loss saw the compensated image; the render backward takes the gradient at pred
            v_pred = exposures.backward_step(view_index, pred, v_pred, lr=self._lr_exposure())
        if bilagrids is not None:
            v_pred = bilagrids.backward_step(view_index, pred, v_pred, lr=self._lr_bilagrid())
        return loss, v_pred

    def _update_records(self, splats, exchange, cfg, size, params, norm_rot, fwd, want_stats):
        """View-sharded data parallelism: records of this view -> all-gather -> per-splat sum -> Adam."""
        means, log_scales, quats, raw_opac, sh = params
        u, aux, pred, v_pred = fwd
        exchange.backward_records(u, aux, means, log_scales, norm_rot, raw_opac, pred, v_pred)
        exchange.gather()
        next_rot = torch.empty_like(quats)
        exchange.reduce_adam(cfg, size, means, log_scales, quats, raw_opac, sh, self.moment1, self.moment2, next_rot,
                             self.grad_2d_accum if want_stats else None, self.xy_grad_counts if want_stats else None)
        self._store_rotation(splats, next_rot)

    def _update_fused(self, splats, cfg, size, params, norm_rot, fwd, want_stats, pose, stream):
        """Single view: the gradients go straight through the optimizer inside the backward's last kernel."""
        means, log_scales, quats, raw_opac, sh = params
        u, aux, pred, v_pred = fwd
        n, l = means.shape[0], _lib.lib()
        nbytes = _lib.size_query("brush_bwd_workspace_size_flags", n, size[0], size[1], int(u.sh_degree),
                                 int(aux.max_intersects), aux.workspace_flags)
        ws, s_aux = aux.backward_workspace(nbytes, means.device)
        v_xy = torch.empty((max(n, 1), 2), dtype=torch.float32, device=means.device)
        next_rot = torch.empty_like(quats)
        args = (C.byref(u), C.byref(s_aux), C.byref(cfg), means.data_ptr(), log_scales.data_ptr(),
                norm_rot.data_ptr(), quats.data_ptr(), raw_opac.data_ptr(), sh.data_ptr(), n, pred.data_ptr(),
                v_pred.data_ptr(), v_xy.data_ptr(), self.moment1.data_ptr(), self.moment2.data_ptr(),
                next_rot.data_ptr(), self.grad_2d_accum.data_ptr() if want_stats else None,
                self.xy_grad_counts.data_ptr() if want_stats else None, ws.data_ptr(), nbytes)
        if pose is None:
            _lib.check(l.brush_render_backward_adam(*args, stream), "brush_render_backward_adam")
        else:
            _lib.check(l.brush_render_backward_adam_pose(*args, pose[0].data_ptr(), pose[1].data_ptr(),
                                                         pose[1].numel(), stream),
                       "brush_render_backward_adam_pose")
        self._store_rotation(splats, next_rot)

    def _update_separate(self, cfg, size, params, norm_rot, fwd, want_stats, pose, stream, effective, depth_grad,
                         grad_sync, batch_views, scene_extent, normal_grad=None, distortion_grad=None):
        """Separate calls: the dense backward (distortion_grad: None, or (cfg, stats, v_distortion) of an active
        distortion term: brush_render_backward_distortion with depth_grad's depth gradient), then whatever works on dense gradients (the splat-normal VJP of an active
        normal-consistency term, the 3D filter's VJP, grad_sync, the refinement statistics, the mcmc regularisers), then
        brush_adam_step on every splat.  normal_grad: None or the [N,3] gradient at the per-splat normals."""
        c = self.config
        use_mcmc = c.strategy == "mcmc"
        means, log_scales, quats, raw_opac, sh = params
        u, aux, pred, v_pred = fwd
        n, ncoef, l = means.shape[0], int(sh.shape[1]), _lib.lib()
        eff_scales, eff_opac = effective
        grads, block = R._backward_impl(u, aux, means, eff_scales, norm_rot, eff_opac, ncoef, pred, v_pred,
                                        depth=depth_grad, pose=pose, distortion=distortion_grad)
        if normal_grad is not None:  # the rendered normal map's gradient -> the quaternions the forward was fed
            from .normal_loss import splat_normals_backward_into
            splat_normals_backward_into(u, means, log_scales, norm_rot, normal_grad, grads["v_quats"])
        if self.filter3d is not None:  # gradients at the effective parameters -> at the raw ones, in place
            F3.backward_into(log_scales, raw_opac, self.filter3d, n, grads["v_scales"], grads["v_opac"], stream)
        if grad_sync is not None:  # view-sharded data parallelism: sum the per-view gradients
            grad_sync(block, aux)
        if want_stats:
            v_xy = grads["v_xy"]
            if torch.distributed.is_available() and torch.distributed.is_initialized() and batch_views > 1:
                from .dist import densification_stats
                stats = densification_stats(v_xy, aux, size)
                allreduce_densification_stats(stats)
                self.grad_2d_accum += stats[0] * float(batch_views)  # undo the 1/batch of the loss scale
                self.xy_grad_counts += stats[1]
            else:
                s_aux = aux._as_struct()
                _lib.check(l.brush_refine_stats(C.byref(s_aux), v_xy.data_ptr(), n, size[0], size[1],
                                                self.grad_2d_accum.data_ptr(), self.xy_grad_counts.data_ptr(),
                                                stream), "brush_refine_stats")
        if use_mcmc:  # the regularisers go through Adam, as in gsplat
            mcmc.reg_grads(raw_opac, log_scales, n, c.mcmc_opacity_reg, c.mcmc_scale_reg, grads["v_opac"],
                           grads["v_scales"], stream)
        _lib.check(l.brush_adam_step(C.byref(cfg), n, R.sh_degree_from_coeffs(ncoef), means.data_ptr(),
                                     log_scales.data_ptr(), quats.data_ptr(), raw_opac.data_ptr(), sh.data_ptr(),
                                     grads["v_means"].data_ptr(), grads["v_scales"].data_ptr(),
                                     grads["v_quats"].data_ptr(), grads["v_opac"].data_ptr(),
                                     grads["v_sh"].data_ptr(), self.moment1.data_ptr(), self.moment2.data_ptr(),
                                     stream),
                   "brush_adam_step")
        if use_mcmc and c.mcmc_noise_lr != 0.0:
            mcmc.inject_noise(means, log_scales, quats, raw_opac, n, c.mcmc_noise_lr * self._lr_mean(scene_extent),
                              c.seed, self.iter, stream)

    def step(self, splats: Splats, camera: Camera, gt_image: torch.Tensor, scene_extent: float = 1.0,
             batch_views: int = 1, grad_sync: Optional[Callable] = None, exchange=None,
             loss_out: Optional[torch.Tensor] = None, view_index: Optional[int] = None, poses=None,
             exposures=None, gt_depth: Optional[torch.Tensor] = None, depth_scale: float = 1.0,
             depth_offset: float = 0.0, background=None, gt_mask: Optional[torch.Tensor] = None, bilagrids=None):
        """One reference training iteration on one view (batch size is 1 in the reference, train.rs:216-219).  Returns
        (loss [1] device tensor, the raw render, its aux).
        `gt_image`: [h,w,3|4] float32 (0..1) or uint8 (read as b / 255 by the loss kernels, the same bits as its float32
        twin; brush_amd.scene_loader keeps the training images on the device in this form).
        `loss_out`: optional float32 [1] device tensor the loss is written into (l1_ssim_loss's `out`).
        `batch_views`, `grad_sync`, `exchange`: view-sharded data parallelism.  Call the step on each rank with
        `batch_views` = world size and either `exchange` = a brush_amd.dist.ViewExchange (per-view gradient records
        all-gathered, summed per splat in view order and fed straight into Adam: every rank applies the same bits) or
        `grad_sync(block, aux)` summing the dense gradient block over views (brush_amd.dist.allreduce_param_grads); not
        both.
        `poses` (a brush_amd.pose.PoseTable) with `view_index`: the view's pending pose update is applied, the view is
        rendered through its current matrix, the backward also returns the view-matrix gradient (the `_pose` entry
        points) and hands it to the table without waiting for it.
        `exposures` (a brush_amd.exposure.ExposureTable) with `view_index`: the view's affine colour map is applied to
        the render, the loss is taken on the result, and the table's backward returns the gradient at the raw render
        (which every backward path then receives beside the raw render) and steps the view's map, all on the device.
        `bilagrids` (a brush_amd.bilagrid.BilagridTable) with `view_index`: the view's bilateral grid takes exactly the
        place the exposure map takes: it is sliced through the raw render in front of the composition, the loss is taken
        on the result, and behind brush_compose_backward the table's backward returns the gradient at the raw render
        (through the colour map and through the luminance that indexes the grid) and steps the view's grid with the
        total-variation prior, all on the device.  On every optimizer path; refused with `exposures` (one colour model
        per view), `exchange` / `grad_sync` and densify_by = "error".
        `gt_depth` (the view's depth map, [h,w] uint16 or float32 on the device, read as raw * depth_scale +
        depth_offset; scene_loader keeps it there as stored) with a positive current TrainConfig.depth_weight: the view
        is rendered with its depth output, brush_depth_loss adds the depth term's alpha gradient into the colour loss's
        gradient and the term itself into the step's loss, and the backward carries the depth gradient
        (brush_render_backward_depth).  With gt_depth None or a zero weight the step is the one without the option.
        `background` (None, "white", "black", "random", an (r, g, b) tuple or a float32 [3] device tensor) and `gt_mask`
        (uint8 [h,w] on the device, nonzero = keep): the image the loss would see (the render, or its exposure-compensated
        form) and the target go through brush_compose_forward first, and the loss's gradient through
        brush_compose_backward, in place, before the exposure backward and every render backward path.  With a
        background the loss compares opaque RGB.  The depth term is not masked here: scene_loader zeroes the depth maps
        under the masks at load.  On every optimizer path; with both None the step is the one without the option.
        From the trainer: TrainConfig.strategy = "mcmc" puts brush_mcmc_reg_grads in front of brush_adam_step and
        brush_mcmc_inject_noise behind it, and a refinement step ends in mcmc.refine; a 3D filter (set_filter3d;
        TrainConfig.filter3d demands one, and one whose length is not the current splat count is refused) puts
        brush_filter3d_apply in front of the forward, which like the backward then works on the effective log-scales
        and opacities, and brush_filter3d_backward on the dense gradients in front of the refinement statistics and
        brush_adam_step on the raw parameters.
        TrainConfig.densify_by = "error": a refining step (will_refine) needs the scores of set_densify_scores for the
        current splats and is refused without them before anything is stepped; no step gathers the gradient statistics;
        refused with strategy "mcmc", `exchange` / `grad_sync`, `poses`, `exposures` and `bilagrids`.
        Single-view, that is refused with `exchange` / `grad_sync`: the 3D filter, `gt_depth`, strategy "mcmc", `poses`,
        `exposures` and `bilagrids` (_check_step); TrainConfig.antialiased is refused with `exchange` alone.  The optimizer path
        (optimizer_path): the records path with `exchange`; the separate-call path (backward, then brush_adam_step)
        with `grad_sync`, strategy "mcmc", an active depth term or a 3D filter, whatever `fused_backward` says;
        otherwise the fused path (brush_render_backward_adam[_pose]) unless `fused_backward` is False.
        TrainConfig.normal_weight > 0 from step normal_from_step on (the depth-normal consistency term, single-view,
        separate-call path): the view is rendered with its depth output; after the colour loss brush_splat_normals on
        the rotations the forward was fed and the feature replay of that forward give the rendered normal map,
        brush_normal_loss adds its alpha gradient into the colour loss's gradient and the term (weight / batch_views)
        into the step's loss, its depth gradient is summed with the depth term's when both are on, the replay's
        transpose gives the gradient at the per-splat normals and brush_splat_normals_backward adds it into v_quats
        behind the render backward.  The replay's blending weights are frozen; with `poses` the pose gets no gradient
        through the normals; the transpose's float atomics make the trajectory order dependent in its last bits, in
        deterministic mode too.  Before normal_from_step, or with weight 0, the step is the one without the option.
        TrainConfig.distortion_weight > 0 from step distortion_from_step on (the depth-distortion term, single-view,
        separate-call path, refused with `poses` and in deterministic mode): the view is rendered with its depth
        output; after the colour, depth and normal terms brush_render_distortion replays that forward,
        distortion_loss_into adds the term (weight / batch_views, masked by `gt_mask`) into the step's loss, and the
        backward is brush_render_backward_distortion with the one summed depth gradient of the other terms (a zero map
        without them): the term's gradient goes through the blending weights and the depths into every geometric
        parameter.  Before distortion_from_step, or with weight 0, the step is the one without the option."""
        c = self.config
        self._check_step(grad_sync, exchange, view_index, poses, exposures, gt_depth, bilagrids)
        use_mcmc = c.strategy == "mcmc"
        filt = self.filter3d
        depth_w = self._depth_weight() if gt_depth is not None else 0.0
        use_depth = depth_w > 0.0
        use_normal = self._normal_active()
        use_dist = self._distortion_active()
        path = optimizer_path(exchange is not None, grad_sync is not None, self.fused_backward, use_mcmc,
                              use_depth or use_normal or use_dist, filt is not None)
        h, w = int(gt_image.shape[0]), int(gt_image.shape[1])
        n, ncoef = splats.num_splats(), int(splats.sh_coeffs.shape[1])
        if self.moment1.numel() != n * (11 + 3 * ncoef):
            raise ValueError("the number of splats changed outside refine_splats: build a new SplatTrainer")
        means, log_scales, quats = splats.means.detach(), splats.log_scales.detach(), splats.rotation.detach()
        sh, raw_opac = splats.sh_coeffs.detach(), splats.raw_opacity.detach()
        params = (means, log_scales, quats, raw_opac, sh)
        for t in params:
            assert t.is_contiguous() and t.dtype == torch.float32
        if filt is not None:
            try:
                F3.check_filter(filt, n, means.device)
            except ValueError as e:
                raise ValueError(f"stale 3D filter: {e}; set one for the current splats (set_filter3d)") from None
        if c.densify_by == "error" and self.will_refine():
            self._check_densify_scores(n)  # before anything is stepped: the refinement below would refuse
        stream = _lib.current_stream(means.device)
        norm_rot = self._take_rotation(splats, stream)
        # on the records and fused paths the optimizer runs inside a kernel that sees which splats the step touches
        # (both take BrushAdamConfig.lazy_sh); the separate calls read and step every SH block
        lazy = self._lazy_state(splats, n, ncoef) if path != "separate" else None
        if lazy is None:
            self.sync(splats)  # nothing may stay pending
            self._lazy = None
        viewmat, pose = None, None
        if poses is not None:
            poses.apply(view_index)  # the update this view's previous draw left
            viewmat = poses.viewmat(view_index, camera).numpy()
            pose = R.pose_buffers(n, means.device)
        # (depth map, compact depth)
        depth_bufs = R._depth_buffers(n, (w, h), means.device) if use_depth or use_normal or use_dist else None
        # the renderer sees the effective log-scales and opacities; everything else keeps reading the raw ones
        effective = (log_scales, raw_opac)
        if filt is not None:
            with torch.cuda.device(means.device):
                effective = F3.apply_into(log_scales, raw_opac, filt, n, stream)
        pred, aux, u = R._forward_impl(camera, (w, h), means, effective[0], norm_rot, sh, effective[1], False, None,
                                       lazy_sh=lazy, antialiased=c.antialiased, viewmat=viewmat, depth=depth_bufs)
        if exchange is not None:
            exchange.begin(aux)  # the per-view counts start travelling while the loss and the backward run
        loss, v_pred = self._loss(pred, gt_image, batch_views, loss_out, view_index, exposures, background, gt_mask,
                                  bilagrids)
        depth_grad = None
        if use_depth:  # on the raw render: alpha gradient into v_pred, the term into the step's loss, no read-back
            from .depth_loss import depth_loss_into
            v_depth, _ = depth_loss_into(pred, depth_bufs[0], gt_depth, v_pred, weight=depth_w / batch_views,
                                         scale=depth_scale, offset=depth_offset, alpha_min=c.depth_alpha_min,
                                         mode=c.depth_mode, loss_accum=loss)
            depth_grad = (depth_bufs[1], v_depth)
        normal_grad = None
        if use_normal:  # on the same raw render; the raw log-scales pick the axis (see TrainConfig)
            from .features import feature_grads_from_aux, features_from_aux
            from .normal_loss import normal_loss_into, splat_normals_from
            normals_img = features_from_aux(u, aux, splat_normals_from(u, means, log_scales, norm_rot))
            v_depth, v_normals_img, _ = normal_loss_into(u, pred, depth_bufs[0], normals_img, v_pred,
                                                         weight=c.normal_weight / batch_views,
                                                         alpha_min=c.normal_alpha_min, loss_accum=loss,
                                                         v_depth_accum=None if depth_grad is None else depth_grad[1])
            depth_grad = (depth_bufs[1], v_depth)
            normal_grad = torch.zeros((n, 3), dtype=torch.float32, device=means.device)
            feature_grads_from_aux(u, aux, v_normals_img, normal_grad)
        distortion_grad = None
        if use_dist:  # a replay of the same forward; the backward adds its VJP into the compact rows
            from .distortion import distortion_config, distortion_from_aux, distortion_loss_into
            dcfg = distortion_config(c.distortion_mode, c.distortion_near, c.distortion_far)
            dstats = distortion_from_aux(u, aux, depth_bufs[1], dcfg)
            v_dist, _ = distortion_loss_into(dstats, torch.empty((h, w), dtype=torch.float32, device=means.device),
                                             weight=c.distortion_weight / batch_views, mask=gt_mask, loss_accum=loss)
            distortion_grad = (dcfg, dstats, v_dist)
            if depth_grad is None:  # no other term made a depth gradient
                depth_grad = (depth_bufs[1], torch.zeros((h, w), dtype=torch.float32, device=means.device))
        do_refine = self.will_refine()
        pre_step = None
        # refinement clones / splits the parameters *before* the optimizer step (train.rs:361-372)
        if do_refine and not use_mcmc:
            self.sync(splats)  # (the forward above has read the pending state; the clones need the eager values)
            pre_step = {"means": means.clone(), "rotation": quats.clone(), "sh": sh.clone(), "opac": raw_opac.clone(),
                        "scales": log_scales.clone()}
        cfg = _lib.BrushAdamConfig(self._lr_mean(scene_extent), c.lr_scale, c.lr_rotation, c.lr_opac,
                                   c.lr_coeffs_dc, 1.0 / c.lr_coeffs_sh_scale, 0.9, 0.999, 1e-15, self.opt_time + 1, 1,
                                   # v_pred carries 1/batch_views: keep the densification statistic at the magnitude the
                                   # reference's threshold was tuned for (batch 1, train.rs:284-316)
                                   float(batch_views))
        if lazy is not None:
            cfg.lazy_sh = C.pointer(lazy)
        # housekeeping, train.rs:284-316; the error rule does not read the gradient statistics
        want_stats = self.iter > c.warmup_steps and not use_mcmc and c.densify_by != "error"
        fwd = (u, aux, pred, v_pred)
        with torch.cuda.device(means.device):
            if path == "records":
                self._update_records(splats, exchange, cfg, (w, h), params, norm_rot, fwd, want_stats)
            elif path == "fused":
                self._update_fused(splats, cfg, (w, h), params, norm_rot, fwd, want_stats, pose, stream)
            else:
                self._update_separate(cfg, (w, h), params, norm_rot, fwd, want_stats, pose, stream, effective,
                                      depth_grad, grad_sync, batch_views, scene_extent, normal_grad, distortion_grad)
        if pose is not None:
            poses.push(view_index, pose[0])
        self.opt_time += 1
        if lazy is not None:
            self._lazy_pending = True
        if do_refine:
            self.sync(splats)  # refinement reads the post-step coefficients of every splat
            self.last_refine = mcmc.refine(self, splats) if use_mcmc else self.refine_splats(splats, pre_step)
        else:
            self.last_refine = None
        self.iter += 1
        return loss, pred, aux
