"""brush_amd — MI355X-native splat rasterizer behind brush-render's op surface.

Host-side mirror (Python, because no Rust toolchain exists in the build image) of
crates/brush-render's public interface for the forward+backward rasterizer path:

  render_splats / RenderAux  <- Backend::render_splats, RenderAux (src/lib.rs:20-86)
  render_splats_depth        <- render_splats plus the accumulated depth map (build extension, no reference)
  render_splats_pose         <- render_splats seen through an explicit world-to-camera matrix, differentiable with
                                respect to it (build extension; gsplat's v_viewmats is the model)
  se3_exp / apply_delta / PoseTable  <- camera-frame twists and the per-view pose optimiser (brush_amd/pose.py)
  apply_exposure / ExposureTable     <- per-view affine colour maps (exposure compensation) and their device-side
                                optimiser (brush_amd/exposure.py; build extension, 3DGS's exposure compensation)
  apply_bilagrid / bilagrid_identity / bilagrid_tv / BilagridTable  <- per-view bilateral grids: a lattice of affine
                                colour maps indexed by pixel position and luminance, sliced through the render before
                                the loss, the total-variation prior and the device-side optimiser (brush_amd/bilagrid.py;
                                build extension, gsplat's use_bilateral_grid is the model; TrainConfig.bilagrid_opt,
                                `python -m brush_amd.train_loop --bilagrid-opt`)
  Camera                     <- camera.rs
  Splats                     <- gaussian_splats.rs (render, from_safetensors / from_ply, from_point_cloud,
                                from_random_config)
  radix_argsort              <- brush-sort/src/lib.rs:32-37
  prefix_sum                 <- brush-prefix-sum/src/lib.rs:17
  eval_stats / EvalStats     <- brush-train/src/eval.rs (also `python -m brush_amd.eval`)
  train_scene / TrainLog     <- brush-viewer/src/train_loop.rs (also `python -m brush_amd.train_loop`)
  scene_loader.SceneLoader   <- brush-dataset/src/scene_loader.rs (training images resident on the device as u8)
  depth_loss / depth_loss_into       <- depth supervision: a fused L1 depth (or disparity) loss on the renderer's
                                depth output (brush_amd/depth_loss.py; build extension, 3DGS's depth regulariser)
  area_resize / nearest_resize / downscaled_size  <- device image pyramids: an exact integer area filter for the u8
                                images and a nearest pick for depth maps (brush_amd/pyramid.py; build extension,
                                nerfstudio's resolution schedule and Mip-Splatting's multi-scale eval are the users:
                                TrainConfig.downscale_schedule, SceneLoader.set_downscale, eval_stats(downscale=))
  Distortion / fit_scale / undistort_image / undistort_depth / undistorted_camera / undistort_dataset  <- COLMAP
                                views with lens distortion (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV) resampled on the
                                device into the pinhole camera the rasterizer assumes (brush_amd/undistort.py; build
                                extension, COLMAP's image_undistorter is the model; both command lines apply it)
  splat_contributions / Contributions / prune_mask / contributions_from_aux  <- per-splat rendered contribution
                                over a set of views (max and summed blending weight, hit and stop counts) from a
                                replay of the compositing walk, and pruning by it (brush_amd/contribution.py; build
                                extension, RadSplat and LightGaussian are the models; also `python -m brush_amd.prune`,
                                Splats.select, TrainConfig.contribution_prune_at)
  splat_error_scores / ErrorScoreBuffers / l1_error_map / error_scores_from_aux  <- per-splat image error over a
                                set of views (a per-pixel error map distributed to the splats by their blending weights,
                                from a replay of the compositing walk) and densification by it (brush_amd/error_score.py;
                                build extension, "Revising Densification in Gaussian Splatting" is the model;
                                TrainConfig.densify_by = "error", `python -m brush_amd.train_loop --densify-by error`)
  filter3d_rates / apply_filter3d / Splats.bake_filter3d  <- the 3D smoothing filter of Mip-Splatting: per-splat
                                filter lengths from the training views' sampling rates, and the map of log-scales and
                                raw opacity that applies them (brush_amd/filter3d.py; build extension;
                                TrainConfig.filter3d, `python -m brush_amd.train_loop --filter3d`)
  TsdfVolume / Mesh / mesh_to_ply / mesh_from_ply / default_bounds / grid_for  <- mesh export: rendered depth maps
                                fused into a dense TSDF volume of integers (order-independent, bitwise repeatable) and
                                an indexed, watertight triangle mesh cut out of it by marching tetrahedra
                                (brush_amd/tsdf.py, brush_amd/mesh.py; build extension, the TSDF exports of 2DGS, GOF
                                and nerfstudio are the models; also `python -m brush_amd.mesh`)
  render_median_depth / median_depth_from_aux  <- the median depth (the z of the splat at which the accumulated
                                opacity first reaches one half) and the id of that splat per pixel, from a replay of the
                                compositing walk; not differentiable (brush_amd/median_depth.py; build extension, the
                                depth 2DGS, GOF and RaDe-GS fuse; Splats.render_median_depth,
                                TsdfVolume.integrate_splats(depth="median"), `python -m brush_amd.mesh --depth median`)
  render_features / splat_feature_sums / lift_labels / FeatureSums / features_from_aux / feature_grads_from_aux /
  feature_sums_from_aux      <- per-splat feature vectors composited into an image (N-channel rasterisation, differentiable
                                with respect to the features only: the geometry is frozen), and the transpose that lifts 2D
                                feature maps or label images onto the splats as exact integer sums, from replays of the
                                compositing walk (brush_amd/features.py; build extension, gsplat's N-channel rasterisation,
                                LangSplat and FlashSplat are the models; Splats.render_features,
                                `python -m brush_amd.lift`)
  splat_normals / depth_normals / normal_loss_into / normal_consistency_loss / render_normals  <- per-splat normals
                                (the shortest axis, facing the camera), the normals a rendered depth map implies, and the
                                depth-normal consistency loss between the rendered normal map and them
                                (brush_amd/normal_loss.py; build extension, 2DGS, GOF, RaDe-GS and PGSR are the models;
                                Splats.render_normals, TrainConfig.normal_weight,
                                `python -m brush_amd.train_loop --normal-weight`)
  render_distortion / distortion_from_aux / distortion_compact_grads_from_aux / distortion_loss_into /
  distortion_config          <- the depth-distortion term sum w_i w_j (m_i - m_j)^2 per pixel (depth or 2DGS's NDC mapping)
                                from a replay of the compositing walk, and its gradient into the geometry, blending
                                weights included, added into the render backward's compact rows by a second replay
                                (brush_amd/distortion.py; build extension, 2DGS, GOF, RaDe-GS and gsplat's 2DGS path are
                                the models; Splats.render_distortion, TrainConfig.distortion_weight,
                                `python -m brush_amd.train_loop --distortion-weight`)
  pack_splats / PackedSplats / morton_order  <- the chunk-quantised "compressed PLY" layout packed and unpacked on the
                                device: Morton order, 256-row chunks, four words and one byte per higher-order SH value
                                per splat (brush_amd/compress.py; build extension; Splats.to_compressed_ply,
                                Splats.from_ply, `--export OUT.compressed.ply`, `python -m brush_amd.compress`)
  mcmc                       <- MCMC densification with a fixed splat budget (build extension; gsplat's MCMCStrategy
                                is the model): TrainConfig(strategy="mcmc"), sample_by_weight, relocation, refine

All compute goes through the C ABI of include/brush_hip.h (libbrush_hip.so, hand-written HIP for
gfx950).  There is no CPU fallback: importing the compute entry points without the built
library raises.
"""
from .camera import Camera, fov_to_focal, focal_to_fov  # noqa: F401
from .render import (RenderAux, render_rgba8, render_splats, render_splats_depth, render_splats_pose,  # noqa: F401
                     rgba8_row_pitch, sh_coeffs_for_degree, sh_degree_from_coeffs)
from .sort import radix_argsort  # noqa: F401
from .prefix_sum import prefix_sum  # noqa: F401
from .gaussian_splats import Splats  # noqa: F401
from .train import SplatTrainer, TrainConfig  # noqa: F401
from . import dataset  # noqa: F401
# (imported eagerly and after the submodule: the package attribute `depth_loss` is the function, the module stays
# reachable as `from brush_amd.depth_loss import ...`)
from .depth_loss import depth_loss, depth_loss_into  # noqa: F401
from .compose import as_background, compose, compose_backward, compose_forward  # noqa: F401  (as depth_loss above)
from .normal_loss import (depth_normals, normal_consistency_loss, normal_loss_into, render_normals,  # noqa: F401
                          splat_normals)
from .distortion import (distortion_compact_grads_from_aux, distortion_config, distortion_from_aux,  # noqa: F401
                         distortion_loss_into, render_distortion)
from .pyramid import area_resize, downscaled_size, nearest_resize  # noqa: F401
from .filter3d import apply_filter3d, filter3d_rates  # noqa: F401
from .undistort import (Distortion, fit_scale, undistort_dataset, undistort_depth, undistort_image,  # noqa: F401
                        undistorted_camera)

# brush_amd.eval and brush_amd.train_loop are imported on first use: importing them here would load the module before
# `python -m brush_amd.eval` / `python -m brush_amd.train_loop` runs it as __main__ (runpy then warns that it is loaded
# twice).
_EVAL_NAMES = ("eval_metrics", "eval_stats", "EvalStats", "EvalView", "eval_depth", "DepthEvalView")
_TRAIN_LOOP_NAMES = ("train_scene", "TrainLog", "TrainLoop")
# brush_amd.pose is imported on first use too: a run without pose refinement never loads it.
_POSE_NAMES = ("se3_exp", "apply_delta", "PoseTable")
_EXPOSURE_NAMES = ("apply_exposure", "ExposureTable")
_BILAGRID_NAMES = ("apply_bilagrid", "bilagrid_identity", "bilagrid_tv", "BilagridTable")
_CONTRIBUTION_NAMES = ("Contributions", "ContributionBuffers", "contributions_from_aux", "splat_contributions",
                       "prune_mask")
_ERROR_SCORE_NAMES = ("ErrorScores", "ErrorScoreBuffers", "l1_error_map", "error_scores_from_aux", "splat_error_scores")
_TSDF_NAMES = ("TsdfVolume", "TsdfArrays")
# (brush_amd.mesh is a command line too: imported on first use, as brush_amd.eval is)
_MEDIAN_DEPTH_NAMES = ("render_median_depth", "median_depth_from_aux")
_FEATURE_NAMES = ("render_features", "splat_feature_sums", "lift_labels", "FeatureSums", "labels_from_sums",
                  "features_from_aux", "feature_grads_from_aux", "feature_sums_from_aux")
_MESH_NAMES = ("Mesh", "mesh_to_ply", "mesh_from_ply", "default_bounds", "grid_for")
# (brush_amd.compress is a command line as well)
_COMPRESS_NAMES = ("pack_splats", "PackedSplats", "morton_order")


def __getattr__(name):
    if name in _EVAL_NAMES:
        from . import eval as _eval
        return getattr(_eval, name)
    if name in _TRAIN_LOOP_NAMES:
        from . import train_loop as _train_loop
        return getattr(_train_loop, name)
    if name in _POSE_NAMES:
        from . import pose as _pose
        return getattr(_pose, name)
    if name in _EXPOSURE_NAMES:
        from . import exposure as _exposure
        return getattr(_exposure, name)
    if name in _BILAGRID_NAMES:
        from . import bilagrid as _bilagrid
        return getattr(_bilagrid, name)
    if name in _CONTRIBUTION_NAMES:
        from . import contribution as _contribution
        return getattr(_contribution, name)
    if name in _ERROR_SCORE_NAMES:
        from . import error_score as _error_score
        return getattr(_error_score, name)
    if name in _TSDF_NAMES:
        from . import tsdf as _tsdf
        return getattr(_tsdf, name)
    if name in _MEDIAN_DEPTH_NAMES:
        from . import median_depth as _median_depth
        return getattr(_median_depth, name)
    if name in _FEATURE_NAMES:
        from . import features as _features
        return getattr(_features, name)
    if name in _MESH_NAMES:
        from . import mesh as _mesh
        return getattr(_mesh, name)
    if name in _COMPRESS_NAMES:
        from . import compress as _compress
        return getattr(_compress, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

__version__ = "0.4.0"
