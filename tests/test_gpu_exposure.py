"""Per-view exposure compensation on the GPU: the three kernels of brush_amd/csrc/exposure.hip against the float64
restatement of tests/exposure_ref64.py, the Adam step, repeatability and graph replay, the autograd function, a frozen
scene fit, the trainer's three optimizer paths and a scene trained end to end from images with per-view gains.

Rounding bounds are stated in u = 2^-24 times the sum of the absolute values of an output's terms (exposure_ref64
returns it beside every output).  The two convergence thresholds come from runs on the MI355X and are recorded in
profiles/exposure_margins.json (BRUSH_EXPOSURE_MARGINS=path makes a run write its own figures there)."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as ED
from tests import exposure_ref64 as X
from tests import helpers as H
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# (1,1) .. (128,128): under a wave, a full wave, wave + 1, not a multiple of the workgroup, many workgroups; 1920x1080
# has more pixels than grid cap (512 workgroups) x 256, so the backward's stride loop runs more than once.
SHAPES = [(1, 1), (7, 5), (64, 1), (65, 3), (33, 31), (128, 128), (1920, 1080)]
MARGINS = {}

# Frozen-scene fit (test 8): FIT_STEPS Adam steps at FIT_LR from the identity.  max|E - E*| end / start measured on the
# MI355X; the gate is its square root (half of the improvement in log terms).
FIT_STEPS, FIT_LR = 300, 1e-2
FIT_RATIO_MEASURED = 0.02034
# End to end (test 10): cv(rho) / cv(1 / g) after 2000 steps, measured on the MI355X; the gate is its square root.
E2E_RATIO_MEASURED = 0.49928


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    path = os.environ.get("BRUSH_EXPOSURE_MARGINS")
    if MARGINS and path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


# ---------------------------------------------------------------------------- helpers: the ABI on torch tensors
def _lib():
    from brush_amd import _lib as L

    return L


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _ws(w, h, dev):
    import torch

    from brush_amd.exposure import workspace_bytes

    n = workspace_bytes(w, h)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def abi_forward(pred, E, out=None):
    import torch

    L = _lib()
    h, w = pred.shape[:2]
    out = torch.empty_like(pred) if out is None else out
    L.check(L.lib().brush_exposure_forward(pred.data_ptr(), E.data_ptr(), w, h, out.data_ptr(), _stream()), "forward")
    return out


def abi_backward(pred, v_out, E, alias=False, v_pred=None, v_E=None, ws=None):
    import torch

    L = _lib()
    h, w = pred.shape[:2]
    if alias:
        v_out = v_out.clone()
        v_pred = v_out
    elif v_pred is None:
        v_pred = torch.empty_like(pred)
    v_E = torch.empty(12, dtype=torch.float32, device=pred.device) if v_E is None else v_E
    ws, n = _ws(w, h, pred.device) if ws is None else ws
    L.check(L.lib().brush_exposure_backward(pred.data_ptr(), v_out.data_ptr(), E.data_ptr(), w, h, v_pred.data_ptr(),
                                            v_E.data_ptr(), ws.data_ptr(), n, _stream()), "backward")
    return v_pred, v_E


def abi_backward_adam(pred, v_out, cfg, E_row, m1_row, m2_row):
    """E_row / m1_row / m2_row: 12-word views into the tables, updated in place."""
    import ctypes as C

    import torch

    L = _lib()
    h, w = pred.shape[:2]
    v_pred = torch.empty_like(pred)
    v_E = torch.empty(12, dtype=torch.float32, device=pred.device)
    ws, n = _ws(w, h, pred.device)
    L.check(L.lib().brush_exposure_backward_adam(pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), w, h,
                                                 v_pred.data_ptr(), E_row.data_ptr(), m1_row.data_ptr(),
                                                 m2_row.data_ptr(), v_E.data_ptr(), ws.data_ptr(), n, _stream()),
            "backward_adam")
    return v_pred, v_E


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


_CASES = {}


def _case(w, h, dev):
    """Inputs and the float64 reference of one shape, computed once and shared: pred in [0,1] with a fifth of the pixels
    at alpha = 0 (half of those empty altogether), signed v_out, E = I + N(0, 0.2)."""
    import torch

    if (w, h) not in _CASES:
        rng = np.random.default_rng(1000 * w + h)
        pred = rng.random((h, w, 4), dtype=np.float32)
        empty = rng.random((h, w)) < 0.2
        pred[..., 3][empty] = 0.0
        pred[empty & (rng.random((h, w)) < 0.5)] = 0.0
        v_out = rng.standard_normal((h, w, 4)).astype(np.float32)
        E = (X.IDENTITY + 0.2 * rng.standard_normal((3, 4))).astype(np.float32).reshape(12)
        ref = {"out": X.forward(pred, E), "v_pred": X.backward_image(v_out, E), "v_E": X.backward_exposure(pred, v_out)}
        _CASES[(w, h)] = (pred, v_out, E, ref)
    pred, v_out, E, ref = _CASES[(w, h)]
    tt = lambda a: torch.from_numpy(a).to(dev)
    return tt(pred), tt(v_out), tt(E), ref


def _worst(got, want, tol):
    """max err / tol over the elements (0 / 0 counts as 0)."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / tol)
    return float(r.max())


# ---------------------------------------------------------------------------- 1-3. the kernels against the restatement
@pytest.mark.parametrize("w,h", SHAPES)
def test_forward_and_backward_match_the_restatement(dev, w, h):
    import torch

    pred, v_out, E, ref = _case(w, h, dev)
    out = abi_forward(pred, E)
    v_pred, v_E = abi_backward(pred, v_out, E)
    v_alias, v_E_alias = abi_backward(pred, v_out, E, alias=True)
    torch.cuda.synchronize()
    # 1. forward: four products and three additions
    want, mag = ref["out"]
    r_fwd = _worst(_np(out), want, 4 * U * mag)
    # 2. v_pred: colour three products and two additions, alpha one more addition
    want, mag = ref["v_pred"]
    r_col = _worst(_np(v_pred)[..., :3], want[..., :3], 3 * U * mag[..., :3])
    r_alp = _worst(_np(v_pred)[..., 3], want[..., 3], 4 * U * mag[..., 3])
    # 3. v_exposure: one rounding to f32 plus the float64 accumulation of exact products
    want, mag = ref["v_E"]
    tol = U * np.abs(want) + (w * h) * 2.0 ** -53 * mag
    r_E = _worst(_np(v_E).reshape(3, 4), want, tol)
    print(f"exposure {w}x{h}: err/tol forward {r_fwd:.3f} v_colour {r_col:.3f} v_alpha {r_alp:.3f} v_E {r_E:.3f}")
    MARGINS[f"kernels_{w}x{h}"] = dict(forward=r_fwd, v_colour=r_col, v_alpha=r_alp, v_exposure=r_E)
    assert r_fwd <= 1.0 and r_col <= 1.0 and r_alp <= 1.0 and r_E <= 1.0
    assert np.array_equal(_np(out)[..., 3], _np(pred)[..., 3])  # alpha is a copy
    # v_pred written over v_out: the same values
    assert np.array_equal(_bits(v_alias), _bits(v_pred)) and np.array_equal(_bits(v_E_alias), _bits(v_E))


# ---------------------------------------------------------------------------- 4. identity
@pytest.mark.parametrize("w,h", SHAPES)
def test_identity_is_the_identity(dev, w, h):
    import torch

    pred, v_out, _, _ = _case(w, h, dev)
    E = torch.tensor(X.IDENTITY.reshape(12), dtype=torch.float32, device=dev)
    out = abi_forward(pred, E)
    v_pred, _ = abi_backward(pred, v_out, E)
    assert bool((out == pred).all()) and bool((v_pred == v_out).all())


# ---------------------------------------------------------------------------- 5. Adam
def _ulp_ok(got, want):
    """|got - want| <= 1 f32 ulp of want, elementwise (want float64)."""
    got = np.asarray(got, dtype=np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return bool((np.abs(got - want) <= ulp).all()), float((np.abs(got - want) / ulp).max())


def test_adam_steps_follow_the_restatement(dev):
    import torch

    w, h = 33, 31
    pred, _, E0, _ = _case(w, h, dev)
    L = _lib()
    V, view = 3, 1
    params = torch.tensor(X.IDENTITY.reshape(12), dtype=torch.float32, device=dev).repeat(V, 1)
    params[view] = E0
    params[2] = E0 * 0.5
    m1 = torch.zeros((V, 12), device=dev)
    m2 = torch.zeros((V, 12), device=dev)
    m1[2], m2[2] = 0.25, 0.125
    lr, reg = 1e-2, 0.05
    worst = 0.0
    for t in range(1, 6):
        rng = np.random.default_rng(70 + t)
        v_out_np = rng.standard_normal((h, w, 4)).astype(np.float32)
        v_out = torch.from_numpy(v_out_np).to(dev)
        before = (_np(params).copy(), _np(m1).copy(), _np(m2).copy())
        E_before = params[view].clone()
        cfg = L.BrushExposureAdam(lr, X.BETA1, X.BETA2, X.EPS, reg, t)
        v_pred, v_E = abi_backward_adam(pred, v_out, cfg, params[view], m1[view], m2[view])
        v_pred_plain, v_E_plain = abi_backward(pred, v_out, E_before)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(v_E), _bits(v_E_plain)) and np.array_equal(_bits(v_pred), _bits(v_pred_plain))
        grad, _ = X.backward_exposure(_np(pred), v_out_np)
        wE, wm1, wm2 = X.adam_step(before[0][view], before[1][view], before[2][view], grad, lr, reg, t)
        for got, want, name in ((params, wE, "E"), (m1, wm1, "m1"), (m2, wm2, "m2")):
            ok, r = _ulp_ok(_np(got)[view].reshape(3, 4), want)
            worst = max(worst, r)
            assert ok, (name, t, r)
            for other in (0, 2):  # the other views' rows keep their bits
                b = before[("E", "m1", "m2").index(name)]
                assert np.array_equal(_np(got)[other].view(np.uint32), b[other].view(np.uint32)), (name, t, other)
        assert bool((params[view] != E_before).all())
    print(f"exposure adam: worst distance to the restatement {worst:.3f} ulp over 5 steps")
    MARGINS["adam_worst_ulp"] = worst
    # a zero gradient at the identity: the row keeps its bits, whatever reg and time
    ident = _bits(params[0]).copy()
    cfg = L.BrushExposureAdam(lr, X.BETA1, X.BETA2, X.EPS, reg, 1)
    abi_backward_adam(pred, torch.zeros_like(pred), cfg, params[0], m1[0], m2[0])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(params[0]), ident)
    assert np.array_equal(ident, np.asarray(X.IDENTITY.reshape(12), dtype=np.float32).view(np.uint32))
    assert not _np(m1[0]).any() and not _np(m2[0]).any()


# ---------------------------------------------------------------------------- 6. repeatability and graph replay
@pytest.mark.parametrize("w,h", [(33, 31), (128, 128)])
def test_repeatable_and_graph_replay(dev, w, h):
    import torch

    pred, v_out, E, _ = _case(w, h, dev)
    first = (abi_forward(pred, E),) + abi_backward(pred, v_out, E)
    again = (abi_forward(pred, E),) + abi_backward(pred, v_out, E)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    out, v_pred = torch.zeros_like(pred), torch.zeros_like(pred)
    v_E = torch.zeros(12, device=dev)
    ws = _ws(w, h, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        abi_forward(pred, E, out=out)
        abi_backward(pred, v_out, E, v_pred=v_pred, v_E=v_E, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        abi_forward(pred, E, out=out)
        abi_backward(pred, v_out, E, v_pred=v_pred, v_E=v_E, ws=ws)
    for _ in range(2):
        out.zero_(), v_pred.zero_(), v_E.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (out, v_pred, v_E)):
            assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------- 7. autograd
def test_apply_exposure_autograd(dev):
    import torch

    from brush_amd import apply_exposure

    w, h = 65, 3
    pred, v_out, E, _ = _case(w, h, dev)
    for shape in ((12,), (3, 4)):
        img = pred.clone().requires_grad_(True)
        e = E.clone().reshape(shape).requires_grad_(True)
        out = apply_exposure(img, e)
        g_img, g_e = torch.autograd.grad((out * v_out).sum(), [img, e])
        want_out = abi_forward(pred, E)
        want_img, want_e = abi_backward(pred, v_out, E)
        assert g_e.shape == shape
        assert np.array_equal(_bits(out), _bits(want_out))
        assert np.array_equal(_bits(g_img), _bits(want_img)) and np.array_equal(_bits(g_e).ravel(), _bits(want_e))
    # a caller's own optimizer on E
    E_true = torch.tensor([0.8, 0, 0, 0.02, 0, 0.7, 0, 0.01, 0, 0, 0.9, 0.03], device=dev)
    target = abi_forward(pred, E_true)
    e = torch.tensor(X.IDENTITY.reshape(12), dtype=torch.float32, device=dev).requires_grad_(True)
    opt = torch.optim.Adam([e], lr=0.02)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = ((apply_exposure(pred, e) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.25 * losses[0], (losses[0], losses[-1])


# ---------------------------------------------------------------------------- 8. frozen-scene fit
def _known_cloud(dev):
    """The cloud test_gpu_train_loop._write_scene renders (the same draws from the same generator)."""
    import torch

    from brush_amd import Splats

    known = Splats.from_random_config(3000, 0, (np.full(3, -0.8), np.full(3, 0.8)), np.random.default_rng(11), dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.06))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    return known


def test_table_fits_a_known_exposure_on_a_frozen_scene(dev):
    """The splats are never touched: the target is the restatement of a known E* applied to the render, and only the
    table is stepped from the identity through l1_ssim_loss and backward_step, FIT_STEPS steps at FIT_LR.
    Measured on the MI355X: max|E - E*| 0.1880 -> 0.00382, end / start = 0.02034 (FIT_RATIO_MEASURED); the gate is its
    square root, 0.1426 (profiles/exposure_margins.json: frozen_fit)."""
    import torch

    from brush_amd.exposure import ExposureTable
    from brush_amd.train import l1_ssim_loss

    w = h = 128
    cam = TL._ring_cameras(16, w, h, 4.0, 1.0, 0.1)[0][1]
    with torch.no_grad():
        pred, _ = _known_cloud(dev).render(cam, (w, h), False)
    pred = pred.detach().contiguous()
    rng = np.random.default_rng(21)
    E_star = np.zeros((3, 4))
    E_star[np.arange(3), np.arange(3)] = rng.uniform(0.6, 0.95, 3)
    E_star[:, 3] = rng.uniform(0.0, 0.05, 3)
    target = torch.from_numpy(X.forward(_np(pred), E_star)[0].astype(np.float32)).to(dev)
    table = ExposureTable(1, dev, FIT_LR)
    start = float(np.abs(table.matrices()[0] - E_star).max())
    for _ in range(FIT_STEPS):
        loss, v_out = l1_ssim_loss(table.forward(0, pred), target, 0.2)
        table.backward_step(0, pred, v_out)
    end = float(np.abs(table.matrices()[0] - E_star).max())
    print(f"exposure frozen fit: max|E - E*| {start:.4f} -> {end:.5f} (ratio {end / start:.5f}), loss {float(loss):.6f}")
    MARGINS["frozen_fit"] = dict(steps=FIT_STEPS, lr=FIT_LR, start=start, end=end, ratio=end / start,
                                 threshold=math.sqrt(FIT_RATIO_MEASURED))
    assert end / start < math.sqrt(FIT_RATIO_MEASURED)
    assert table.steps == [FIT_STEPS]
    # the state survives a deep copy and a state_dict round trip
    twin = copy.deepcopy(table)
    other = ExposureTable(1, dev, 1.0)
    other.load_state_dict(table.state_dict())
    for t in (twin, other):
        assert np.array_equal(_bits(t.params), _bits(table.params)) and t.steps == table.steps and t.lr == table.lr
        assert np.array_equal(_bits(t.moment1), _bits(table.moment1))


# ---------------------------------------------------------------------------- 9. trainer
def _trainer_cloud():
    cloud = H.synthetic_cloud(4096, 3, seed=13, mean_mult=0.0005)
    cloud["log_scales"] = cloud["log_scales"] - 3.0
    return cloud


def _trainer_setup(dev):
    import torch

    import brush_amd

    cloud = _trainer_cloud()
    w, h = 128, 80
    cams = [c for _, c in TL._ring_cameras(3, w, h, 8.0, 1.0, 0.3)]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda: brush_amd.Splats(tt(cloud["means"]), tt(cloud["sh"]), tt(cloud["quats"] * 1.7), tt(cloud["raw_opac"]),
                                  tt(cloud["log_scales"]))
    torch.manual_seed(5)
    gts = [torch.rand((h, w, 3), device=dev) for _ in cams]
    return mk, cams, gts


ORDER = [0, 1, 1, 2, 0, 1]  # six steps, a back-to-back repeat included; the table has a fourth view that is never drawn


def _run_trainer(dev, mk, cams, gts, fused, deferred, with_table=True, poses=None, **cfg_kw):
    import brush_amd
    from brush_amd.exposure import ExposureTable

    s = mk()
    cfg = brush_amd.TrainConfig(**{**dict(warmup_steps=0, max_refine_step=0, deferred_sh_adam=deferred), **cfg_kw})
    tr = brush_amd.SplatTrainer(s, cfg)
    tr.fused_backward = fused
    table = ExposureTable(4, dev, cfg.lr_exposure, cfg.exposure_reg) if with_table else None
    losses = []
    for i in ORDER:
        kw = dict(view_index=i, exposures=table) if with_table else {}
        if poses is not None:
            kw.update(view_index=i, poses=poses)
        losses.append(float(tr.step(s, cams[i], gts[i], **kw)[0]))
    tr.sync(s)
    state = {k: getattr(s, k).detach().clone() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")}
    state["moment1"], state["moment2"] = tr.moment1.clone(), tr.moment2.clone()
    return losses, state, table


PATHS = [(True, False), (True, True), (False, False)]  # fused eager, fused deferred-SH, separate-call


def test_trainer_with_zero_rate_is_the_trainer_without_the_option(dev, deterministic):
    import torch

    mk, cams, gts = _trainer_setup(dev)
    ident = np.tile(np.asarray(X.IDENTITY.reshape(12), dtype=np.float32), (4, 1))
    for fused, deferred in PATHS:
        off = _run_trainer(dev, mk, cams, gts, fused, deferred, with_table=False)
        on = _run_trainer(dev, mk, cams, gts, fused, deferred, lr_exposure=0.0, exposure_reg=0.0)
        assert on[0] == off[0], (fused, deferred)
        for k in off[1]:
            assert torch.equal(on[1][k], off[1][k]), (fused, deferred, k)
        assert np.array_equal(_bits(on[2].params), ident.view(np.uint32))
        assert on[2].steps == [ORDER.count(i) for i in range(4)]


def test_trainer_paths_hold_the_same_table_and_splats(dev, deterministic):
    mk, cams, gts = _trainer_setup(dev)
    runs = [_run_trainer(dev, mk, cams, gts, fused, deferred, lr_exposure=1e-2, exposure_reg=1e-3)
            for fused, deferred in PATHS]
    for r in runs[1:]:
        assert r[0] == runs[0][0]
        for k in runs[0][1]:
            assert np.array_equal(_bits(r[1][k]), _bits(runs[0][1][k])), k
        for name in ("params", "moment1", "moment2"):
            assert np.array_equal(_bits(getattr(r[2], name)), _bits(getattr(runs[0][2], name))), name
    table = runs[0][2]
    ident = np.asarray(X.IDENTITY.reshape(12), dtype=np.float32)
    E = _np(table.params)
    for i in range(3):  # drawn: every word moved (the first Adam step moves each by lr whatever the gradient's size)
        assert (E[i] != ident).all(), i
    assert np.array_equal(E[3].view(np.uint32), ident.view(np.uint32))  # never drawn: the identity's bits
    assert not _np(table.moment1)[3].any() and not _np(table.moment2)[3].any()
    off = _run_trainer(dev, mk, cams, gts, True, True, with_table=False)
    assert off[0] != runs[0][0]  # the table moved the trajectory


@pytest.mark.parametrize("mode", ["antialiased", "poses", "mcmc"])
def test_trainer_with_the_other_options(dev, mode):
    from brush_amd.pose import PoseTable

    mk, cams, gts = _trainer_setup(dev)
    kw, poses = {}, None
    if mode == "antialiased":
        kw = dict(antialiased=True)
    elif mode == "poses":
        poses = PoseTable(len(cams), 1e-3, 1e-2, 1e-4)
    else:
        kw = dict(strategy="mcmc", mcmc_cap_max=4096)
    losses, _, table = _run_trainer(dev, mk, cams, gts, True, True, poses=poses, **kw)
    assert np.isfinite(losses).all()
    E = table.matrices()
    assert np.isfinite(E).all() and (E[:3] != X.IDENTITY.astype(np.float32)).any()
    if poses is not None:
        poses.apply_all()
        assert bool(poses.delta.abs().sum() > 0)


def test_trainer_steps_with_exposures_do_not_synchronise(dev):
    import torch

    import brush_amd
    from brush_amd.exposure import ExposureTable

    mk, cams, gts = _trainer_setup(dev)
    for fused, deferred in PATHS:
        s = mk()
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0,
                                                             deferred_sh_adam=deferred))
        tr.fused_backward = fused
        table = ExposureTable(4, dev, 1e-2, 1e-6)
        tr.step(s, cams[0], gts[0], view_index=0, exposures=table)  # the first step fills the deferred-SH table
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for i in ORDER:
                tr.step(s, cams[i], gts[i], view_index=i, exposures=table)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert table.steps == [3, 3, 1, 0]


# ---------------------------------------------------------------------------- 10. end to end
GAIN_RANGE, OFFSET_RANGE = (0.55, 0.95), (0.0, 0.05)


def _scene_exposures(n, seed=31):
    """Per-view diagonal E_i: gains per channel from GAIN_RANGE, offsets from OFFSET_RANGE (out <= 0.95 + 0.05: no
    clipping)."""
    rng = np.random.default_rng(seed)
    E = np.zeros((n, 3, 4))
    E[:, np.arange(3), np.arange(3)] = rng.uniform(*GAIN_RANGE, (n, 3))
    E[:, :, 3] = rng.uniform(*OFFSET_RANGE, (n, 3))
    return E


def _write_exposed_scene(root, dev, exposures, w=128, h=128, n_train=16, n_val=4):
    """test_gpu_train_loop._write_scene with every training image passed through the restatement of its view's E before
    it is quantised (exposures = None: the clean scene); the val images are always clean."""
    import torch

    known = _known_cloud(dev)
    fovx = 0.6911112070083618
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, (c2w, cam) in enumerate(TL._ring_cameras(n, w, h, 4.0, 1.0, off)):
            with torch.no_grad():
                pred, _ = known.render(cam, (w, h), False)
            img64 = pred.cpu().numpy().astype(np.float64)
            if split == "train" and exposures is not None:
                img64 = X.forward(img64, exposures[i])[0]
            img = np.clip(np.round(img64[..., :3] * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(ED.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def exposed_scene(tmp_path_factory, dev):
    E = _scene_exposures(16)
    return _write_exposed_scene(str(tmp_path_factory.mktemp("exposed_scene")), dev, E), E


def _cv(x):
    """Coefficient of variation over the views (axis 0), per channel."""
    return x.std(axis=0) / x.mean(axis=0)


def test_train_scene_recovers_per_view_gains(dev, deterministic, exposed_scene, tmp_path):
    """2000 random splats, 2000 steps, the option off and on (same seed, deterministic) on images with per-view gains,
    and the clean scene with the option off for the report.  With rho = A_i[c,c] / g_i,c the coefficient of variation
    of rho over the views measures what is left of the views' disagreement (identity exposures leave cv(1 / g)); one
    global gain stays shared between the scene and the table, so the clean eval views are off by it and the three
    eval PSNRs are printed, not asserted.
    Measured on the MI355X: cv(rho) 0.07977 against cv(1 / g) 0.15977, ratio 0.49928 (E2E_RATIO_MEASURED); the gate is
    its square root, 0.7066.  Last-100 loss -0.18104 off, -0.19298 on; eval PSNR 21.68 dB off, 23.85 dB on, 37.82 dB on
    the clean scene (profiles/exposure_margins.json: e2e)."""
    from brush_amd import TrainConfig
    from brush_amd.train_loop import load_dataset, train_scene

    root, E_true = exposed_scene
    data, _ = load_dataset(root)
    clean, _ = load_dataset(_write_exposed_scene(str(tmp_path / "clean"), dev, None))
    assert len(data.train.views) == 16

    def run(d, on):
        cfg = TrainConfig(warmup_steps=50, refine_every=50, exposure_opt=on)
        rows = []
        _, log = train_scene(d, cfg, steps=2000, init_count=2000, sh_degree=3, seed=5, eval_every=2000,
                             on_eval=lambda r, s: rows.append(r))
        return log, rows[-1].psnr

    log_off, psnr_off = run(data, False)
    log_on, psnr_on = run(data, True)
    _, psnr_clean = run(clean, False)
    assert log_off.exposure_opt is False and log_off.exposures is None
    js = log_off.to_json()
    assert js["exposure_opt"] is False and js["exposures"] is None
    assert log_on.exposure_opt is True and len(log_on.exposures) == 16 and all(len(e) == 12 for e in log_on.exposures)
    assert len(log_on.to_json()["exposures"]) == 16
    tail_off, tail_on = float(np.mean(log_off.losses[-100:])), float(np.mean(log_on.losses[-100:]))
    A = np.asarray(log_on.exposures, dtype=np.float64).reshape(16, 3, 4)
    gains = E_true[:, np.arange(3), np.arange(3)]
    rho = A[:, np.arange(3), np.arange(3)] / gains
    cv_on, cv_ident = float(_cv(rho).mean()), float(_cv(1.0 / gains).mean())
    ratio = cv_on / cv_ident
    print(f"exposure e2e: last-100 loss off {tail_off:.6f} on {tail_on:.6f}; cv(rho) {cv_on:.5f} vs cv(1/g) "
          f"{cv_ident:.5f} (ratio {ratio:.5f}); eval psnr off {psnr_off:.3f} on {psnr_on:.3f} clean scene {psnr_clean:.3f}")
    MARGINS["e2e"] = dict(loss_off=tail_off, loss_on=tail_on, cv_rho=cv_on, cv_identity=cv_ident, ratio=ratio,
                          threshold=math.sqrt(E2E_RATIO_MEASURED), psnr_off=psnr_off, psnr_on=psnr_on,
                          psnr_clean_scene=psnr_clean)
    assert tail_on < tail_off
    assert cv_on < cv_ident
    assert ratio <= math.sqrt(E2E_RATIO_MEASURED)


# ---------------------------------------------------------------------------- 11. CLI
def test_cli_exports_the_exposures(exposed_scene, tmp_path):
    root, _ = exposed_scene
    out_json, out_exp = str(tmp_path / "log.json"), str(tmp_path / "exp.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", root, "--steps", "60", "--init-count", "1000",
                        "--exposure-opt", "--export-exposures", out_exp, "--json", out_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_json) as f:
        log = json.load(f)
    assert log["exposure_opt"] is True and len(log["exposures"]) == 16 and len(log["losses"]) == 60
    with open(out_exp) as f:
        exp = json.load(f)
    assert exp["exposure_opt"] is True and len(exp["views"]) == 16
    ident = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    names = set()
    for v in exp["views"]:
        assert set(v) == {"name", "exposure"} and np.asarray(v["exposure"]).shape == (3, 4)
        names.add(v["name"])
    assert len(names) == 16
    assert any(v["exposure"] != ident for v in exp["views"])
    assert [e for v in exp["views"] for row in v["exposure"] for e in row] == [x for e in log["exposures"] for x in e]
