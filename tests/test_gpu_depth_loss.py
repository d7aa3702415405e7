"""Depth supervision on the GPU: brush_depth_loss against its numpy restatement (tests/depth_loss_ref64.py) bit for
bit, repeatability and graph replay, the autograd form through the depth render, the trainer option (off: the trainer
without it; on: the manual composition of the calls), and a scene with 16-bit depth maps trained end to end with and
without supervision."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import depth_loss_ref64 as DR
from tests import eval_data as ED
from tests import helpers as H
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# (513, 512): 262656 pixels, more than one sweep of the kernel's grid cap (1024 workgroups x 256 lanes = 262144), so
# the grid-stride loop runs twice for the first 512 lanes.
SHAPES = [(1, 1), (33, 31), (128, 128), (513, 512)]
VARIANTS = [(m, d) for m in DR.MODES for d in (np.uint16, np.float32)]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = _np(t) if not isinstance(t, np.ndarray) else t
    return np.ascontiguousarray(a).view(np.uint32)


def _scale_offset(mode, gt_dtype):
    if gt_dtype == np.float32:
        return 1.7, -0.03
    return (0.00105, -0.05) if mode == "depth" else (1e-4, -0.001)


_CASES = {}


def _case(w, h, mode, gt_dtype):
    """Inputs and the f32 restatement of one (shape, variant), computed once and shared."""
    key = (w, h, mode, np.dtype(gt_dtype).name)
    if key not in _CASES:
        scale, offset = _scale_offset(mode, gt_dtype)
        seed = 1000 * w + h
        case = DR.make_case(w, h, gt_dtype, mode, seed, scale, offset)
        while w * h == 1 and not DR.valid_f32(case["alpha"], case["D"], case["raw"], scale, offset,
                                              case["alpha_min"]).all():
            seed += 1  # the single pixel must count: the first seed that leaves it valid
            case = DR.make_case(w, h, gt_dtype, mode, seed, scale, offset)
        kw = dict(weight=0.7, scale=scale, offset=offset, alpha_min=case["alpha_min"], mode=mode)
        pred = np.random.default_rng(seed + 1).random((h, w, 4), dtype=np.float32)
        pred[..., 3] = case["alpha"]
        _CASES[key] = (case, pred, kw, DR.reference_f32(case["alpha"], case["D"], case["raw"], **kw))
    return _CASES[key]


def _abi(dev, pred, depth, target, kw, v_depth=None, v_pred=None, stats=None, accum=None, ws=None):
    """brush_depth_loss on preallocated torch tensors (None: NULL)."""
    import torch

    from brush_amd import _lib as L
    from brush_amd.depth_loss import MODES, workspace_bytes

    h, w = pred.shape[:2]
    cfg = L.BrushDepthLoss(kw["weight"], kw["scale"], kw["offset"], kw["alpha_min"], MODES[kw["mode"]],
                           L.DEPTH_GT_U16 if target.dtype == torch.uint16 else L.DEPTH_GT_F32)
    n = workspace_bytes(w, h)
    ws = torch.empty(n, dtype=torch.uint8, device=dev) if ws is None else ws
    stats = torch.empty(2, dtype=torch.float32, device=dev) if stats is None else stats
    p = lambda t: None if t is None else t.data_ptr()
    L.check(L.lib().brush_depth_loss(pred.data_ptr(), depth.data_ptr(), target.data_ptr(), C.byref(cfg), w, h,
                                     p(v_depth), p(v_pred), stats.data_ptr(), p(accum), ws.data_ptr(), n,
                                     torch.cuda.current_stream().cuda_stream), "brush_depth_loss")
    return stats


def _upload(dev, case, pred):
    import torch

    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return tt(pred), tt(case["D"]), tt(case["raw"]), tt(case["v_pred"])


def _ulp32(x):
    return float(np.spacing(np.abs(F(x))))


# ---------------------------------------------------------------------------- 1. the kernel against the restatement
@pytest.mark.parametrize("mode,gt_dtype", VARIANTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_kernel_matches_the_restatement_bitwise(dev, w, h, mode, gt_dtype):
    import torch

    case, pred_np, kw, ref = _case(w, h, mode, gt_dtype)
    valid = ref["valid"]
    frac = float(valid.mean())
    if w * h >= 64:
        assert 0.25 <= frac <= 0.75, frac            # the test cannot pass on an all-invalid image
    else:
        assert frac == 1.0
    if w * h >= 1000:                                 # every invalidity rule occurs
        for name, m in case["rule"].items():
            assert m.any(), name
        assert {"alpha", "absent", "t<=0", "D=0"} <= set(case["rule"])
        if gt_dtype == np.float32:
            assert {"nan", "inf", "negative"} <= set(case["rule"])
    pred, depth, target, v_pred0 = _upload(dev, case, pred_np)
    assert target.dtype == (torch.uint16 if gt_dtype == np.uint16 else torch.float32)
    v_pred = v_pred0.clone()
    v_depth = torch.full((h, w), 7.0, device=dev)
    accum = torch.tensor([0.37], device=dev)
    stats = _np(_abi(dev, pred, depth, target, kw, v_depth, v_pred, accum=accum))
    # per-pixel outputs: the bits of the f32 restatement
    assert np.array_equal(_bits(v_depth), _bits(ref["v_depth"]))
    got = _np(v_pred)
    want_alpha = case["v_pred"][..., 3].copy()
    want_alpha[valid] = (want_alpha[valid] + ref["v_alpha"][valid]).astype(F)     # one f32 add
    assert np.array_equal(_bits(got[..., 3]), _bits(want_alpha))
    assert np.array_equal(_bits(got[..., :3]), _bits(case["v_pred"][..., :3]))    # r, g, b untouched
    assert np.array_equal(_bits(got[~valid]), _bits(case["v_pred"][~valid]))      # invalid pixels untouched
    assert (got[..., 3][valid] != case["v_pred"][..., 3][valid]).any()            # ... and valid ones moved
    assert not _np(v_depth)[~valid].any() and _np(v_depth)[valid].all()
    # the statistics
    want_loss = DR.loss_f64(ref)
    print(f"depth loss {w}x{h} {mode} {np.dtype(gt_dtype).name}: valid {frac:.4f}, loss {stats[0]!r} vs f64 "
          f"{want_loss!r} ({abs(float(stats[0]) - want_loss) / _ulp32(want_loss):.3f} ulp)")
    assert abs(float(stats[0]) - want_loss) <= _ulp32(want_loss)
    assert stats[1] == DR.valid_fraction(ref)
    assert _np(accum)[0] == F(0.37) + stats[0]                                    # loss_accum: one f32 add


# ---------------------------------------------------------------------------- 2. repeatability, graph replay, NULLs
@pytest.mark.parametrize("mode,gt_dtype", [("depth", np.uint16), ("disparity", np.float32)])
@pytest.mark.parametrize("w,h", [(33, 31), (513, 512)])
def test_repeatable_graph_replay_and_null_outputs(dev, w, h, mode, gt_dtype):
    import torch

    case, pred_np, kw, _ = _case(w, h, mode, gt_dtype)
    pred, depth, target, v_pred0 = _upload(dev, case, pred_np)

    def run():
        v_pred, v_depth = v_pred0.clone(), torch.empty((h, w), device=dev)
        stats = _abi(dev, pred, depth, target, kw, v_depth, v_pred)
        return v_depth, v_pred, stats

    first, again = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    # metrics only: the same statistics, nothing else written
    for vd, vp in ((None, None), (torch.empty((h, w), device=dev), None), (None, v_pred0.clone())):
        assert np.array_equal(_bits(_abi(dev, pred, depth, target, kw, vd, vp)), _bits(first[2]))
        if vd is not None:
            assert np.array_equal(_bits(vd), _bits(first[0]))
        if vp is not None:
            assert np.array_equal(_bits(vp), _bits(first[1]))
    # graph capture and replay
    from brush_amd.depth_loss import workspace_bytes

    v_depth, v_pred, stats = torch.zeros((h, w), device=dev), v_pred0.clone(), torch.zeros(2, device=dev)
    ws = torch.empty(workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        _abi(dev, pred, depth, target, kw, v_depth, v_pred, stats, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _abi(dev, pred, depth, target, kw, v_depth, v_pred, stats, ws=ws)
    for _ in range(2):
        v_depth.zero_(), stats.zero_(), v_pred.copy_(v_pred0)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (v_depth, v_pred, stats)):
            assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------- 3. autograd through the depth render
def _tiny(dev, grad):
    import torch

    import brush_amd

    d = H.load_case("tiny_case")
    h, w, _ = d["out_img"].shape
    c = H.reference_test_camera(w, h)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    t = {k: torch.as_tensor(np.ascontiguousarray(d[s]), device=dev) for k, s in
         (("means", "means"), ("log_scales", "scales"), ("quats", "quats"), ("sh", "coeffs"), ("raw_opac", "opacities"))}
    if grad:
        for v in t.values():
            v.requires_grad_(True)
    return cam, w, h, t


@pytest.mark.parametrize("mode", DR.MODES)
def test_depth_loss_autograd_is_the_manual_composition(dev, mode):
    import torch

    import brush_amd
    from brush_amd import render as R
    from brush_amd.depth_loss import depth_loss_into

    cam, w, h, t = _tiny(dev, True)
    img, depth, _ = brush_amd.render_splats_depth(cam, (w, h), t["means"], None, t["log_scales"], t["quats"], t["sh"],
                                                  t["raw_opac"], deterministic=True)
    a, D = _np(img)[..., 3], _np(depth)
    with np.errstate(divide="ignore", invalid="ignore"):
        rendered = np.where((a >= 0.05) & (D > 0), (D / a) if mode == "depth" else (a / D), 0.0)
    rng = np.random.default_rng(5)
    target_np = (rendered * rng.choice([0.8, 1.25], rendered.shape)).astype(F)    # either sign of r
    target_np[rng.random(rendered.shape) < 0.2] = 0.0
    target = torch.from_numpy(target_np).to(dev)
    kw = dict(weight=0.7, scale=1.1, offset=0.01, alpha_min=0.05, mode=mode)
    loss = brush_amd.depth_loss(img, depth, target, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    names = ("means", "log_scales", "quats", "sh", "raw_opac")
    grads = torch.autograd.grad(loss * 1.0, [t[k] for k in names])
    # the same by hand: forward with depth, the kernel into a zero gradient image, the depth backward
    d = {k: v.detach() for k, v in t.items()}
    bufs = R._depth_buffers(d["means"].shape[0], (w, h), dev)
    pred, aux, u = R._forward_impl(cam, (w, h), d["means"], d["log_scales"], d["quats"], d["sh"], d["raw_opac"], False,
                                   None, deterministic=True, depth=bufs)
    assert np.array_equal(_bits(pred), _bits(img)) and np.array_equal(_bits(bufs[0]), _bits(depth))
    v_pred = torch.zeros_like(pred)
    v_depth, stats = depth_loss_into(pred, bufs[0], target, v_pred, **kw)
    assert 0.1 < float(stats[1]) < 0.95 and float(stats[0]) > 0
    assert np.array_equal(_bits(loss), _bits(stats[0]))
    g, _ = R._backward_impl(u, aux, d["means"], d["log_scales"], d["quats"], d["raw_opac"], d["sh"].shape[1], pred,
                            v_pred, depth=(bufs[1], v_depth))
    for k, got in zip(("v_means", "v_scales", "v_quats", "v_sh", "v_opac"), grads):
        assert np.array_equal(_bits(got), _bits(g[k])), k
        assert bool(torch.isfinite(got).all())
    assert bool(grads[0].any())
    # the incoming scalar scales both gradients
    cam, w, h, t2 = _tiny(dev, True)
    img2, depth2, _ = brush_amd.render_splats_depth(cam, (w, h), t2["means"], None, t2["log_scales"], t2["quats"],
                                                    t2["sh"], t2["raw_opac"], deterministic=True)
    g_img, g_depth = torch.autograd.grad(brush_amd.depth_loss(img2, depth2, target, **kw) * 2.0, [img2, depth2])
    assert np.array_equal(_bits(g_img), _bits(v_pred * 2.0)) and np.array_equal(_bits(g_depth), _bits(v_depth * 2.0))


# ---------------------------------------------------------------------------- 4. trainer
W = Hh = 64
ORDER = [0, 1, 1, 2, 0, 1, 2, 2, 0, 1, 0, 2, 1, 1, 0, 2, 0, 1, 2, 0]   # 20 steps, back-to-back repeats included
ALPHA_MIN = 0.05  # the small test cloud covers few pixels well: count the thinly covered ones too


def _trainer_setup(dev):
    """512 splats seen by three 64x64 cameras, random colour targets, and per view a u16 millimetre depth map: the
    initial cloud's own expected depth pushed 20 % out, 0 where alpha < ALPHA_MIN and on a random tenth."""
    import torch

    import brush_amd

    cloud = H.synthetic_cloud(512, 3, seed=13, mean_mult=0.0005)
    cloud["log_scales"] = cloud["log_scales"] - 2.0
    cams = [c for _, c in TL._ring_cameras(3, W, Hh, 8.0, 1.0, 0.3)]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda: brush_amd.Splats(tt(cloud["means"]), tt(cloud["sh"]), tt(cloud["quats"] * 1.7), tt(cloud["raw_opac"]),
                                  tt(cloud["log_scales"]))
    torch.manual_seed(5)
    gts = [torch.rand((Hh, W, 3), device=dev) for _ in cams]
    depths = []
    rng = np.random.default_rng(9)
    s = mk()
    for cam in cams:
        with torch.no_grad():
            img, D, _ = s.render_depth(cam, (W, Hh))
        a, D = _np(img)[..., 3].astype(np.float64), _np(D).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mm = np.where((a >= ALPHA_MIN) & (D > 0), D / a * 1.2 * 1000.0, 0.0)
        mm[rng.random(mm.shape) < 0.1] = 0.0
        assert mm.max() < 65535 and (mm > 0).mean() > 0.1, ((mm > 0).mean(), mm.max())
        depths.append(tt(np.round(mm).astype(np.uint16)))
    return mk, cams, gts, depths


def _state(s, tr):
    st = {k: getattr(s, k).detach().clone() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")}
    st["moment1"], st["moment2"] = tr.moment1.clone(), tr.moment2.clone()
    st["grad_2d_accum"], st["xy_grad_counts"] = tr.grad_2d_accum.clone(), tr.xy_grad_counts.clone()
    return st


def _run_trainer(dev, setup, fused, deferred, with_depth, order=ORDER, poses=None, table=None, **cfg_kw):
    import brush_amd

    mk, cams, gts, depths = setup
    s = mk()
    cfg = brush_amd.TrainConfig(**{**dict(warmup_steps=0, max_refine_step=0, deferred_sh_adam=deferred,
                                          depth_alpha_min=ALPHA_MIN), **cfg_kw})
    tr = brush_amd.SplatTrainer(s, cfg)
    tr.fused_backward = fused
    losses = []
    for i in order:
        kw = dict(gt_depth=depths[i], depth_scale=0.001) if with_depth else {}
        if poses is not None:
            kw.update(view_index=i, poses=poses)
        if table is not None:
            kw.update(view_index=i, exposures=table)
        losses.append(float(tr.step(s, cams[i], gts[i], **kw)[0]))
    tr.sync(s)
    return losses, _state(s, tr)


PATHS = [(True, False), (True, True), (False, False)]  # fused eager, fused deferred-SH, separate-call


def test_trainer_with_zero_weight_is_the_trainer_without_the_option(dev, deterministic):
    import torch

    setup = _trainer_setup(dev)
    for fused, deferred in PATHS:
        off = _run_trainer(dev, setup, fused, deferred, with_depth=False)
        on = _run_trainer(dev, setup, fused, deferred, with_depth=True, depth_weight=0.0)
        assert on[0] == off[0], (fused, deferred)
        for k in off[1]:
            assert torch.equal(on[1][k], off[1][k]), (fused, deferred, k)
    sup = _run_trainer(dev, setup, True, True, with_depth=True, depth_weight=0.3)
    assert sup[0] != off[0] and not torch.equal(sup[1]["means"], off[1]["means"])   # a positive weight moves the run
    assert all(a > b for a, b in zip(sup[0][:1], off[0][:1]))                       # the first loss holds the depth term


def test_supervised_step_is_the_manual_composition(dev, deterministic):
    """Three steps (the second and third also feed the refinement statistics) against the five calls made by hand:
    forward with depth, colour loss, brush_depth_loss into v_pred and the loss word, backward with depth,
    brush_refine_stats and brush_adam_step."""
    import torch

    import brush_amd
    from brush_amd import _lib as L
    from brush_amd import render as R
    from brush_amd.depth_loss import depth_loss_into
    from brush_amd.train import l1_ssim_loss

    setup = _trainer_setup(dev)
    mk, cams, gts, depths = setup
    order = [0, 1, 1]
    kw = dict(depth_weight=0.3, depth_weight_final=0.03, depth_mode="disparity", total_steps=10)
    for fused in (True, False):  # a supervised step takes the separate-call path whatever fused_backward says
        got_losses, got = _run_trainer(dev, setup, fused, True, with_depth=True, order=order, **kw)
        s = mk()
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, depth_alpha_min=ALPHA_MIN, **kw)
        clock = brush_amd.SplatTrainer(mk(), cfg)      # only for the schedules (_lr_mean, _depth_weight)
        n, ncoef = s.num_splats(), int(s.sh_coeffs.shape[1])
        m1, m2 = torch.zeros(n * (11 + 3 * ncoef), device=dev), torch.zeros(n * (11 + 3 * ncoef), device=dev)
        accum, counts = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        l, stream = L.lib(), torch.cuda.current_stream().cuda_stream
        means, log_scales, quats = s.means.detach(), s.log_scales.detach(), s.rotation.detach()
        sh, raw_opac = s.sh_coeffs.detach(), s.raw_opacity.detach()
        losses = []
        for it, i in enumerate(order):
            clock.iter = it
            norm_rot = torch.empty_like(quats)
            L.check(l.brush_normalize_quats(quats.data_ptr(), norm_rot.data_ptr(), n, stream), "normalize")
            bufs = R._depth_buffers(n, (W, Hh), dev)
            pred, aux, u = R._forward_impl(cams[i], (W, Hh), means, log_scales, norm_rot, sh, raw_opac, False, None,
                                           depth=bufs)                                                         # 1
            loss, v_pred = l1_ssim_loss(pred, gts[i], cfg.ssim_weight, cfg.ssim_window_size, 1.0)              # 2
            v_depth, _ = depth_loss_into(pred, bufs[0], depths[i], v_pred, weight=clock._depth_weight(), scale=0.001,
                                         offset=0.0, alpha_min=ALPHA_MIN, mode="disparity", loss_accum=loss)   # 3
            g, _ = R._backward_impl(u, aux, means, log_scales, norm_rot, raw_opac, ncoef, pred, v_pred,
                                    depth=(bufs[1], v_depth))                                                  # 4
            if it > 0:                                                                                         # 5
                s_aux = aux._as_struct()
                L.check(l.brush_refine_stats(C.byref(s_aux), g["v_xy"].data_ptr(), n, W, Hh, accum.data_ptr(),
                                             counts.data_ptr(), stream), "stats")
            acfg = L.BrushAdamConfig(clock._lr_mean(1.0), cfg.lr_scale, cfg.lr_rotation, cfg.lr_opac, cfg.lr_coeffs_dc,
                                     1.0 / cfg.lr_coeffs_sh_scale, 0.9, 0.999, 1e-15, it + 1, 1, 1.0)
            L.check(l.brush_adam_step(C.byref(acfg), n, R.sh_degree_from_coeffs(ncoef), means.data_ptr(),
                                      log_scales.data_ptr(), quats.data_ptr(), raw_opac.data_ptr(), sh.data_ptr(),
                                      g["v_means"].data_ptr(), g["v_scales"].data_ptr(), g["v_quats"].data_ptr(),
                                      g["v_opac"].data_ptr(), g["v_sh"].data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                      stream), "adam")
            losses.append(float(loss))
        assert abs(clock._depth_weight() - 0.3 * 0.1 ** 0.2) < 1e-12
        want = dict(means=means, log_scales=log_scales, rotation=quats, raw_opacity=raw_opac, sh_coeffs=sh, moment1=m1,
                    moment2=m2, grad_2d_accum=accum, xy_grad_counts=counts)
        assert got_losses == losses, fused
        for k, v in want.items():
            assert np.array_equal(_bits(got[k]), _bits(v)), (fused, k)
        assert bool(accum.any())


@pytest.mark.parametrize("mode", ["antialiased", "poses", "exposures", "mcmc"])
def test_supervised_trainer_with_the_other_options(dev, mode):
    import torch

    from brush_amd.exposure import ExposureTable
    from brush_amd.pose import PoseTable

    setup = _trainer_setup(dev)
    kw, poses, table = {}, None, None
    if mode == "antialiased":
        kw = dict(antialiased=True)
    elif mode == "poses":
        poses = PoseTable(3, 1e-3, 1e-2, 1e-4)
    elif mode == "exposures":
        table = ExposureTable(3, dev, 1e-2, 1e-6)
    else:
        kw = dict(strategy="mcmc", mcmc_cap_max=512)
    order = ORDER[:8]
    on = _run_trainer(dev, setup, True, True, True, order=order, poses=poses, table=table, depth_weight=0.3, **kw)
    assert np.isfinite(on[0]).all()
    for k, v in on[1].items():
        assert bool(torch.isfinite(v).all()), k
    if poses is not None:
        poses.apply_all()
        assert bool(poses.delta.abs().sum() > 0)
    if table is not None:
        assert table.steps == [order.count(i) for i in range(3)]
    # the depth term is in the step: the same run without it holds other parameters
    poses2 = PoseTable(3, 1e-3, 1e-2, 1e-4) if poses is not None else None
    table2 = ExposureTable(3, dev, 1e-2, 1e-6) if table is not None else None
    off = _run_trainer(dev, setup, True, True, False, order=order, poses=poses2, table=table2, **kw)
    assert not torch.equal(on[1]["means"], off[1]["means"])


def test_supervised_steps_do_not_synchronise(dev):
    import torch

    import brush_amd

    mk, cams, gts, depths = _trainer_setup(dev)
    s = mk()
    tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, depth_weight=0.3,
                                                         depth_alpha_min=ALPHA_MIN))
    log = torch.zeros(7, device=dev)
    tr.step(s, cams[0], gts[0], gt_depth=depths[0], depth_scale=0.001, loss_out=log[0:1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k, i in enumerate(ORDER[:6]):
            tr.step(s, cams[i], gts[i], gt_depth=depths[i], depth_scale=0.001, loss_out=log[k + 1:k + 2])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(log).all()) and bool((log != 0).all())


# ---------------------------------------------------------------------------- 5. end to end
E2E_STEPS, E2E_WEIGHT = 300, 0.2


def _png16(a):
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint16)).save(buf, format="PNG")
    return buf.getvalue()


def _write_depth_scene(root, dev, w=64, h=64, n_train=3, n_val=4):
    """test_gpu_train_loop._write_scene's known cloud seen by few cameras, with 16-bit PNG depth maps beside the images:
    D / alpha in millimetres, 0 where alpha < 0.5."""
    import torch

    from brush_amd import Splats

    known = Splats.from_random_config(3000, 0, (np.full(3, -0.8), np.full(3, 0.8)), np.random.default_rng(11), dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.06))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        os.makedirs(os.path.join(root, "depth", split), exist_ok=True)
        frames = []
        for i, (c2w, cam) in enumerate(TL._ring_cameras(n, w, h, 4.0, 1.0, off)):
            with torch.no_grad():
                pred, D, _ = known.render_depth(cam, (w, h))
            img = np.clip(np.round(_np(pred)[..., :3] * 255.0), 0, 255).astype(np.uint8)
            a, D = _np(pred)[..., 3].astype(np.float64), _np(D).astype(np.float64)
            mm = np.where(a >= 0.5, D / np.maximum(a, 1e-6) * 1000.0, 0.0)
            assert mm.max() < 65535 and (mm > 0).mean() > 0.2
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(ED.png_bytes(img))
            with open(os.path.join(root, "depth", split, f"r_{i}.png"), "wb") as f:
                f.write(_png16(np.round(mm)))
            frames.append({"file_path": f"./{split}/r_{i}", "depth_file_path": f"./depth/{split}/r_{i}.png",
                           "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def depth_scene(tmp_path_factory, dev):
    return _write_depth_scene(str(tmp_path_factory.mktemp("depth_scene")), dev)


def test_depth_supervision_lowers_the_held_out_depth_error(dev, deterministic, depth_scene):
    """Three 64x64 training views of the known cloud, four held-out views, 1000 random initial splats, E2E_STEPS steps
    from the same seed in deterministic mode, once with depth_weight = 0 and once with E2E_WEIGHT: the held-out depth
    error (eval_depth: mean |D / alpha - t| over the valid pixels, averaged over the views) must be strictly lower with
    supervision.  Both runs are bitwise repeatable, so the unsupervised run is the yardstick as it stands.
    No measured values yet: the test prints both errors and both PSNRs before it asserts."""
    import torch

    from brush_amd import TrainConfig
    from brush_amd.eval import eval_depth, eval_stats
    from brush_amd.scene_loader import SceneLoader
    from brush_amd.train_loop import load_dataset, train_scene

    data, _ = load_dataset(depth_scene)
    assert len(data.train.views) == 3 and len(data.eval.views) == 4
    assert all(v.depth is not None and v.depth.dtype == np.uint16 and v.depth_scale == 0.001
               for v in data.train.views + data.eval.views)
    loader = SceneLoader(data.train, 1, dev)
    assert all(d.dtype == torch.uint16 for d in loader.depths) and loader.depth(1) is loader.depths[1]
    assert loader.total_bytes == sum(v.image.nbytes + v.depth.nbytes for v in data.train.views)

    def run(weight):
        cfg = TrainConfig(warmup_steps=50, refine_every=50, depth_weight=weight)
        splats, log = train_scene(data, cfg, steps=E2E_STEPS, init_count=1000, sh_degree=3, seed=5)
        rows = eval_depth(splats, data.eval)
        assert len(rows) == 4 and all(0.0 < r.valid_fraction <= 1.0 for r in rows)
        return (float(np.mean([r.mean_abs_error for r in rows])), eval_stats(splats, data.eval).mean_psnr(),
                float(np.mean([r.valid_fraction for r in rows])), log)

    mae_off, psnr_off, valid_off, log_off = run(0.0)
    mae_on, psnr_on, valid_on, log_on = run(E2E_WEIGHT)
    print(f"depth e2e ({E2E_STEPS} steps, weight {E2E_WEIGHT}): held-out depth error off {mae_off:.5f} on {mae_on:.5f} "
          f"(valid {valid_off:.3f} / {valid_on:.3f}); eval psnr off {psnr_off:.3f} on {psnr_on:.3f}; last loss off "
          f"{log_off.losses[-1]:.5f} on {log_on.losses[-1]:.5f}")
    assert np.isfinite([mae_off, mae_on]).all()
    assert mae_on < mae_off


def test_cli_trains_with_depth_and_reports_depth_metrics(depth_scene, tmp_path):
    ply, out_json = str(tmp_path / "out.ply"), str(tmp_path / "eval.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = ("import sys; from brush_amd import train_loop, eval as ev; "
            "r = train_loop.main([sys.argv[1], '--steps', '40', '--init-count', '500', '--depth-weight', '0.2', "
            "'--depth-weight-final', '0.05', '--export', sys.argv[2]]); "
            "sys.exit(r or ev.main([sys.argv[2], sys.argv[1], '--depth-metrics', '--json', sys.argv[3]]))")
    r = subprocess.run([sys.executable, "-c", code, depth_scene, ply, out_json], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "depth_mae" in r.stdout
    with open(out_json) as f:
        res = json.load(f)
    assert res["depth_mode"] == "depth" and len(res["depth_views"]) == 4
    for v in res["depth_views"]:
        assert set(v) == {"name", "mean_abs_error", "valid_fraction"} and 0.0 <= v["valid_fraction"] <= 1.0
    assert len(res["views"]) == 4 and "mean_psnr" in res
    assert math.isfinite(res["mean_depth_abs_error"])
