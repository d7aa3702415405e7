"""CPU checks of per-view exposure compensation (brush_exposure_*, brush_amd/exposure.py): the float64 restatement
against central differences, the identity map, the entry points' argument checks, and the Python / CLI surface.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from tests import exposure_ref64 as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=3, w=8, h=6):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 4))
    E = X.IDENTITY + 0.2 * rng.standard_normal((3, 4))
    wgt = rng.standard_normal((h, w, 4))
    return img, E, wgt


# ---------------------------------------------------------------------------- 1. restatement vs central differences
def test_restatement_matches_central_differences():
    """L = sum out w with random w, in float64: v' = w.  The map is bilinear in (img, E), so the central difference
    quotient is exact up to rounding: relative error <= 1e-8 at h = 1e-6 for every entry of both gradients.  The two
    sums are subtracted term by term with math.fsum (exactly, rounded once), so that the quotient carries the rounding
    of the terms that changed and not that of two sums of 192 terms that cancel."""
    img, E, wgt = _case()
    terms = lambda im, e: (X.forward(im, e)[0] * wgt).ravel()
    step = 1e-6
    quotient = lambda plus, minus: math.fsum(np.concatenate([terms(*plus), -terms(*minus)])) / (2 * step)
    v_img, _ = X.backward_image(wgt, E)
    v_E, _ = X.backward_exposure(img, wgt)
    worst = 0.0
    for idx in np.ndindex(3, 4):
        d = np.zeros((3, 4))
        d[idx] = step
        worst = max(worst, abs(quotient((img, E + d), (img, E - d)) - v_E[idx]) / abs(v_E[idx]))
    for idx in np.ndindex(*img.shape):
        d = np.zeros_like(img)
        d[idx] = step
        worst = max(worst, abs(quotient((img + d, E), (img - d, E)) - v_img[idx]) / abs(v_img[idx]))
    print("exposure restatement vs central differences: worst relative error", worst)
    assert worst <= 1e-8


def test_identity_returns_the_image_and_alpha_weights_the_offset():
    img, E, wgt = _case(5)
    out, mag = X.forward(img, X.IDENTITY)
    assert np.array_equal(out, img) and np.array_equal(mag, np.abs(img))
    vp, _ = X.backward_image(wgt, X.IDENTITY)
    assert np.array_equal(vp, wgt)
    # an uncovered pixel stays empty whatever the offset; alpha passes through
    img[2, 3] = 0.0
    out, _ = X.forward(img, E)
    assert np.array_equal(out[2, 3], np.zeros(4)) and np.array_equal(out[..., 3], img[..., 3])
    # opaque pixels: 3DGS's A c + b
    img[..., 3] = 1.0
    out, _ = X.forward(img, E)
    assert np.allclose(out[..., :3], img[..., :3] @ E[:, :3].T + E[:, 3], rtol=0, atol=1e-15)


def test_adam_restatement_first_step_and_penalty():
    """First step from zero moments: the bias corrections cancel and E moves by lr sign(g) (eps = 1e-15); the penalty
    enters the gradient as reg (E - [I|0]); a zero gradient at the identity changes nothing."""
    E = X.IDENTITY + 0.1
    g = np.full((3, 4), 0.5)
    E1, m1, m2 = X.adam_step(E, np.zeros(12), np.zeros(12), g, lr=1e-2, reg=0.25, time=1)
    gg = g + float(np.float32(0.25)) * 0.1
    assert np.allclose(m1, (1 - float(np.float32(0.9))) * gg, rtol=1e-15)
    assert np.allclose(E1, E - float(np.float32(1e-2)), rtol=0, atol=1e-12)
    E1, m1, m2 = X.adam_step(X.IDENTITY, np.zeros(12), np.zeros(12), np.zeros(12), lr=1e-2, reg=0.25, time=1)
    assert np.array_equal(E1, X.IDENTITY) and not m1.any() and not m2.any()


# ---------------------------------------------------------------------------- 2. the ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_exposure_entry_points_validate_arguments_without_gpu(lib):
    from brush_amd import _lib

    INVALID, SMALL = -1, -2
    for name in ("brush_exposure_workspace_size", "brush_exposure_forward", "brush_exposure_backward",
                 "brush_exposure_backward_adam"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)
    n = C.c_size_t()
    assert lib.brush_exposure_workspace_size(16, 16, None) == INVALID
    assert lib.brush_exposure_workspace_size(0, 16, C.byref(n)) == INVALID
    assert lib.brush_exposure_workspace_size(16, 0, C.byref(n)) == INVALID
    assert lib.brush_exposure_workspace_size(1 << 14, 1 << 14, C.byref(n)) == INVALID      # 2^28 pixels
    assert lib.brush_exposure_workspace_size(1 << 16, 1 << 16, C.byref(n)) == INVALID      # 2^32: no wrap to 0 either
    assert lib.brush_exposure_workspace_size(1, 1, C.byref(n)) == 0 and n.value >= 96
    assert lib.brush_exposure_workspace_size((1 << 14) - 1, 1 << 14, C.byref(n)) == 0 and 96 <= n.value <= 48 * 1024
    assert lib.brush_exposure_workspace_size(1920, 1080, C.byref(n)) == 0
    big = n.value
    assert big == 512 * 12 * 8  # 1080p exceeds grid cap x 256 pixels: the stride loop runs more than once
    # non-null pointers that are never dereferenced: every call below fails before any device work
    a, b, c, e = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    w, h = 1920, 1080
    # brush_exposure_forward(pred, exposure, w, h, out, stream)
    assert lib.brush_exposure_forward(None, e, w, h, b, None) == INVALID
    assert lib.brush_exposure_forward(a, None, w, h, b, None) == INVALID
    assert lib.brush_exposure_forward(a, e, w, h, None, None) == INVALID
    assert lib.brush_exposure_forward(a, e, 0, h, b, None) == INVALID
    assert lib.brush_exposure_forward(a, e, 1 << 14, 1 << 14, b, None) == INVALID
    assert lib.brush_exposure_forward(a, e, w, h, a, None) == INVALID                    # out aliases pred
    assert lib.brush_exposure_forward(a, e, w, h, C.c_void_p(0x2004), None) == INVALID   # images are 16-byte aligned
    # brush_exposure_backward(pred, v_out, exposure, w, h, v_pred, v_exposure, ws, ws_bytes, stream)
    ok = [a, b, e, w, h, b, c, C.c_void_p(0x5000), big, None]
    for i in (0, 1, 2, 5, 6, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.brush_exposure_backward(*bad) == INVALID, i
    for dims in ((0, h), (w, 0), (1 << 14, 1 << 14)):
        bad = list(ok)
        bad[3], bad[4] = dims
        assert lib.brush_exposure_backward(*bad) == INVALID, dims
    bad = list(ok)
    bad[8] = big - 1
    assert lib.brush_exposure_backward(*bad) == SMALL   # the ABI's status for a workspace that is too small
    assert lib.brush_status_string(SMALL) == b"workspace too small"
    # brush_exposure_backward_adam(pred, v_out, cfg, w, h, v_pred, exposure, m1, m2, v_exposure, ws, ws_bytes, stream)
    cfg = _lib.BrushExposureAdam(1e-2, 0.9, 0.999, 1e-15, 1e-6, 1)
    m1, m2 = C.c_void_p(0x6000), C.c_void_p(0x7000)
    ok = [a, b, C.byref(cfg), w, h, b, e, m1, m2, c, C.c_void_p(0x5000), big, None]
    for i in (0, 1, 2, 5, 6, 7, 8, 9, 10):
        bad = list(ok)
        bad[i] = None
        assert lib.brush_exposure_backward_adam(*bad) == INVALID, i
    for dims in ((0, h), (w, 0), (1 << 14, 1 << 14)):
        bad = list(ok)
        bad[3], bad[4] = dims
        assert lib.brush_exposure_backward_adam(*bad) == INVALID, dims
    bad = list(ok)
    bad[11] = big - 1
    assert lib.brush_exposure_backward_adam(*bad) == SMALL
    zero_time = _lib.BrushExposureAdam(1e-2, 0.9, 0.999, 1e-15, 1e-6, 0)   # time is 1-based
    bad = list(ok)
    bad[2] = C.byref(zero_time)
    assert lib.brush_exposure_backward_adam(*bad) == INVALID
    assert C.sizeof(_lib.BrushExposureAdam) == 24


# ---------------------------------------------------------------------------- 3. Python surface and CLI
def test_python_surface_without_gpu():
    import torch

    import brush_amd
    from brush_amd import exposure as EX

    assert brush_amd.apply_exposure is EX.apply_exposure and brush_amd.ExposureTable is EX.ExposureTable
    c = brush_amd.TrainConfig()
    assert c.exposure_opt is False
    assert c.lr_exposure == 1e-2 and c.lr_exposure_decay == 0.1 and c.exposure_reg == 1e-6
    assert "exposures" in inspect.signature(brush_amd.SplatTrainer.step).parameters
    for name in ("forward", "backward_step", "matrices", "state_dict", "load_state_dict"):
        assert callable(getattr(EX.ExposureTable, name)), name
    # the schedule: lr_exposure at step 0, lr_exposure * lr_exposure_decay at total_steps
    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig(total_steps=1000)
    tr.iter = 0
    assert tr._lr_exposure() == 1e-2
    tr.iter = 1000
    assert abs(tr._lr_exposure() - 1e-3) < 1e-15
    # no CPU path
    with pytest.raises(AssertionError, match="no CPU path"):
        EX.apply_exposure(torch.zeros((4, 4, 4)), torch.zeros(12))
    with pytest.raises(AssertionError, match="no CPU path"):
        EX.ExposureTable(3, "cpu", 1e-2)


def test_step_rejects_exposures_with_exchange_and_without_view_index():
    """Both checks run before any device work: a trainer that was never initialised and no splats are enough."""
    import brush_amd

    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig()
    table = object()
    with pytest.raises(ValueError, match="single-view"):
        tr.step(None, None, None, exchange=object(), view_index=0, exposures=table)
    with pytest.raises(ValueError, match="single-view"):
        tr.step(None, None, None, grad_sync=lambda b, a: None, view_index=0, exposures=table)
    with pytest.raises(ValueError, match="view_index"):
        tr.step(None, None, None, exposures=table)


def test_cli_flags_and_log_keys():
    from brush_amd import train_loop as TL

    p = TL.parser()
    a = p.parse_args(["data"])
    assert a.exposure_opt is False and a.export_exposures is None
    a = p.parse_args(["data", "--exposure-opt", "--export-exposures", "exp.json"])
    assert a.exposure_opt is True and a.export_exposures == "exp.json"
    log = TL.TrainLog(0, np.zeros(0, np.float32))
    js = log.to_json()
    assert js["exposure_opt"] is False and js["exposures"] is None
    log.exposure_opt, log.exposures = True, [list(X.IDENTITY.reshape(12))]
    js = log.to_json()
    assert js["exposure_opt"] is True and js["exposures"] == [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]
