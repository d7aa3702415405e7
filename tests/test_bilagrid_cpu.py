"""CPU checks of the per-view bilateral grids (brush_bilagrid_*, brush_amd/bilagrid.py): the float64 restatement of
tests/bilagrid_ref64.py against central differences, the prior, the three consequences of the lerp form, the coordinate
table, the Adam step, the entry points' argument checks, the configuration / CLI surface and the kernels' resources.
Nothing here needs a GPU."""
import ctypes as C
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import bilagrid_ref64 as B
from tests import exposure_ref64 as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=3, w=7, h=5, shape=(5, 3, 4)):
    """Pixels whose luminance lies strictly inside a level (the fraction of z in [0.25, 0.75]), so that a difference
    step never moves a pixel to another level; alpha and colours otherwise random, one pixel at alpha 0."""
    gw, gh, gl = shape
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 4)) + 0.05
    level = rng.integers(0, gl - 1, (h, w))
    z = level + rng.uniform(0.25, 0.75, (h, w))
    lum = (B.LUMA[0] * img[..., 0] + B.LUMA[1] * img[..., 1]) + B.LUMA[2] * img[..., 2]
    img[..., :3] *= (z / (gl - 1) / lum)[..., None]
    img[1, 2, 3] = 0.0
    G = B.identity(shape) + 0.2 * rng.standard_normal((gl, gh, gw, 12))
    wgt = rng.standard_normal((h, w, 4))
    return img, G, wgt


# ---------------------------------------------------------------------------- 1. restatement vs central differences
def test_restatement_matches_central_differences():
    """L = sum out w in float64 with the continuous fz: v' = w.  L is linear in G and quadratic in the pixel (M is
    linear in fz, fz in the pixel, and M multiplies the pixel), so the central quotient is exact up to rounding.  The
    two sums are subtracted term by term with math.fsum.  Bound: the quotient's rounding is about 2^-52 |terms| / step
    ~ 1e-9 in absolute terms at step 1e-6, so 1e-6 relative to |want| + 1e-3 mean |want| leaves three decimal orders."""
    img, G, wgt = _case()
    shape = (G.shape[2], G.shape[1], G.shape[0])
    terms = lambda im, g: (B.forward(im, g, continuous=True)[0] * wgt).ravel()
    step = 1e-6
    quotient = lambda plus, minus: math.fsum(np.concatenate([terms(*plus), -terms(*minus)])) / (2 * step)
    v_img, _ = B.backward_image(img, wgt, G, continuous=True)
    v_G, _, _ = B.backward_grid(img, wgt, shape, continuous=True)
    worst = 0.0
    for want, arg in ((v_G, 1), (v_img, 0)):
        floor = 1e-3 * np.abs(want).mean()
        for idx in np.ndindex(*want.shape):
            d = np.zeros_like(want)
            d[idx] = step
            plus, minus = ((img + d, G), (img - d, G)) if arg == 0 else ((img, G + d), (img, G - d))
            worst = max(worst, abs(quotient(plus, minus) - want[idx]) / (abs(want[idx]) + floor))
    print("bilagrid restatement vs central differences: worst relative error", worst)
    assert worst <= 1e-6
    # the luminance path is there: without q the image gradient is another one
    assert np.abs(v_img[..., :3] - np.einsum("hwc,hwcm->hwm", wgt[..., :3],
                                             B.slice_grid(img, G, True)[0].reshape(5, 7, 3, 4)[..., :3])).max() > 1e-3


def test_float32_coordinates_agree_with_the_continuous_ones():
    """The f32 definition and the continuous functional place every test pixel in the same cell, fractions within f32
    rounding of each other."""
    img, G, _ = _case(7)
    shape = (G.shape[2], G.shape[1], G.shape[0])
    a, b = B.coords(img.astype(np.float32), shape), B.coords(img, shape, continuous=True)
    for i in (0, 2, 4):
        assert np.array_equal(a[i], b[i])
    for i in (1, 3, 5):
        assert np.abs(a[i] - b[i]).max() < 1e-5


def test_tv_gradient_matches_central_differences():
    _, G, _ = _case(11)
    g, _ = B.tv_grad(G)
    step, worst = 1e-6, 0.0
    floor = 1e-3 * np.abs(g).mean()
    for idx in np.ndindex(*G.shape):
        d = np.zeros_like(G)
        d[idx] = step
        # a quadratic: the quotient is exact up to rounding; the two sums are subtracted term by term, as above
        q = math.fsum(np.concatenate([B.tv_terms(G + d), -B.tv_terms(G - d)])) / (2 * step)
        worst = max(worst, abs(q - g[idx]) / (abs(g[idx]) + floor))
    print("bilagrid tv gradient vs central differences: worst relative error", worst)
    assert worst <= 1e-6
    assert B.tv(B.identity((5, 3, 4)))[0] == 0.0 and not B.tv_grad(B.identity((5, 3, 4)))[0].any()


def test_tv_agrees_with_the_torch_prior():
    import torch

    from brush_amd.bilagrid import bilagrid_identity, bilagrid_tv

    _, G, _ = _case(12)
    t = torch.from_numpy(G).requires_grad_(True)
    val = bilagrid_tv(t)
    (g,) = torch.autograd.grad(val, t)
    assert abs(float(val.detach()) - B.tv(G)[0]) <= 1e-14 * B.tv(G)[0]
    assert np.abs(g.numpy() - B.tv_grad(G)[0]).max() <= 1e-15
    ident = bilagrid_identity((5, 3, 4))
    assert tuple(ident.shape) == (4, 3, 5, 12) and np.array_equal(ident.numpy(), B.identity((5, 3, 4)).astype(np.float32))


# ---------------------------------------------------------------------------- 2. consequences of the lerp form
def test_lerp_form_consequences_in_the_restatement():
    rng = np.random.default_rng(5)
    img = rng.random((5, 7, 4)).astype(np.float32)
    img[0, 0, :3] = 2.0   # luminance above 1
    img[0, 1, :3] = -0.5  # and below 0
    wgt = rng.standard_normal((5, 7, 4)).astype(np.float32)
    shape = (5, 3, 4)
    # 1. the identity grid returns pred
    out, _ = B.forward(img, B.identity(shape))
    assert np.array_equal(out, img.astype(np.float64))
    # 2. a constant grid is the exposure map: forward and v_pred
    E = X.IDENTITY + 0.2 * rng.standard_normal((3, 4))
    G = np.tile(E.reshape(12), (4, 3, 5, 1))
    out, _ = B.forward(img, G)
    want, mag = X.forward(img, E)
    assert np.abs(out - want).max() <= 8 * 2.0 ** -53 * mag.max()
    vp, _ = B.backward_image(img, wgt, G)
    want, mag = X.backward_image(wgt, E)
    assert np.abs(vp - want).max() <= 8 * 2.0 ** -53 * mag.max()
    # 3. the vertices' gradients add up to the exposure gradient (the weights of a pixel sum to one)
    v_G, mag_G, reached = B.backward_grid(img, wgt, shape)
    want, mag = X.backward_exposure(img, wgt)
    assert np.abs(v_G.sum(axis=(0, 1, 2)).reshape(3, 4) - want).max() <= 35 * 8 * 2.0 ** -53 * mag.max()
    assert not v_G[~reached].any() and not mag_G[~reached].any()


# ---------------------------------------------------------------------------- 3. the coordinate table
def test_coordinate_table():
    i0, f = B.axis_coords(1, 16)
    assert i0.tolist() == [0] and f.tolist() == [0.0]
    i0, f = B.axis_coords(2, 16)  # only vertices 0 and 15 are reached
    assert i0.tolist() == [0, 14] and f.tolist() == [0.0, 1.0]
    img = np.full((1, 2, 4), 0.5, np.float32)
    _, _, reached = B.backward_grid(img, np.ones_like(img), (16, 2, 2))
    assert np.flatnonzero(reached.any(axis=(0, 1))).tolist() == [0, 15]
    i0, f = B.axis_coords(31, 16)  # w - 1 = 2 (GW - 1): every second pixel sits on a vertex
    assert f.dtype == np.float32 and (f[::2][:-1] == 0).all() and (f[1::2] == 0.5).all()
    assert i0[::2][:-1].tolist() == list(range(15))
    for w, g in ((31, 16), (33, 31), (128, 16), (7, 5), (3, 64)):
        i0, f = B.axis_coords(w, g)
        assert i0[-1] == g - 2 and f[-1] == 1.0 and i0[0] == 0 and f[0] == 0.0
        assert (np.diff(i0) >= 0).all() and (f >= 0).all() and (f <= 1).all()
        pos = i0 + f.astype(np.float64)  # the continuous coordinate x (g - 1) / (w - 1)
        assert np.abs(pos - np.arange(w) * (g - 1) / (w - 1)).max() < 1e-5
        # the kernel's rectangles: cell c holds exactly the pixels cell_first(c) .. cell_first(c + 1) - 1
        for c in range(g - 1):
            assert np.flatnonzero(i0 == c).tolist() == list(range(B.cell_first(c, w, g), B.cell_first(c + 1, w, g)))
    # guidance: NaN, <= 0 and >= 1 never leave [0, GL - 1]
    p = np.zeros((1, 5, 4), np.float32)
    p[0, :, 0] = [np.nan, -1.0, 0.0, 1.0 / 0.299, 5.0]
    k0, fz, inside = B.guidance(p, 8)
    assert k0[0].tolist() == [0, 0, 0, 6, 6] and fz[0, :3].tolist() == [0, 0, 0] and fz[0, 4] == 1.0
    assert inside[0].tolist() == [False, False, False, bool(np.float32(0.299) * np.float32(1 / 0.299) < 1), False]


# ---------------------------------------------------------------------------- 4. Adam
def test_adam_restatement_first_step_with_a_prior():
    """First step from zero moments: the bias corrections cancel and every word with a gradient moves by lr (eps =
    1e-15); the prior enters as tv dTV/dG; a zero gradient at the identity (whose TV gradient is zero) changes
    nothing."""
    _, G, _ = _case(13)
    g = np.full(G.shape, 0.5)
    G1, m1, m2 = B.adam_step(G, np.zeros_like(G), np.zeros_like(G), g, lr=2e-3, tv_weight=10.0, time=1)
    gg = g + float(np.float32(10.0)) * B.tv_grad(G)[0]
    assert np.allclose(m1, (1 - float(np.float32(0.9))) * gg, rtol=1e-15)
    assert np.allclose(G1, G - float(np.float32(2e-3)) * np.sign(gg), rtol=0, atol=1e-12)
    ident = B.identity((5, 3, 4))
    G1, m1, m2 = B.adam_step(ident, np.zeros_like(G), np.zeros_like(G), np.zeros_like(G), 2e-3, 10.0, 1)
    assert np.array_equal(G1, ident) and not m1.any() and not m2.any()


def test_frozen_fit_reference_reaches_a_quarter():
    """The step count of the GPU suite's frozen fit is chosen so that the float64 run on the host leaves less than a
    quarter of the residual; the device run is then held to the square root of this ratio."""
    start, end = B.fit_reference()
    print(f"bilagrid frozen fit, float64 on the host: residual {start:.5f} -> {end:.6f} (ratio {end / start:.5f})")
    assert end / start < 0.25


# ---------------------------------------------------------------------------- 5. the ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_bilagrid_entry_points_validate_arguments_without_gpu(lib):
    from brush_amd import _lib

    INVALID, SMALL = -1, -2
    for name in ("brush_bilagrid_workspace_size", "brush_bilagrid_forward", "brush_bilagrid_backward",
                 "brush_bilagrid_backward_adam"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)
    n = C.c_size_t()
    size = lib.brush_bilagrid_workspace_size
    bad_dims = [(0, 16), (16, 0), (1 << 14, 1 << 14), (1 << 16, 1 << 16), (32769, 1), (1, 32769)]
    bad_grids = [(1, 16, 8), (65, 16, 8), (16, 1, 8), (16, 65, 8), (16, 16, 1), (16, 16, 9), (0, 0, 0)]
    assert size(16, 16, 16, 16, 8, None) == INVALID
    for w, h in bad_dims:
        assert size(w, h, 16, 16, 8, C.byref(n)) == INVALID, (w, h)
    for g in bad_grids:
        assert size(64, 64, *g, C.byref(n)) == INVALID, g
    for (w, h), shape in (((1, 1), (2, 2, 2)), ((1, 1), (64, 64, 8)), ((32768, 1), (16, 16, 8)), ((1, 32768), (16, 16, 8)),
                          ((1920, 1080), (16, 16, 8)), ((33, 31), (2, 2, 2)), ((128, 128), (5, 3, 4)),
                          ((1, 107), (16, 16, 8)), ((1, 106), (16, 16, 8))):
        assert size(w, h, *shape, C.byref(n)) == 0 and n.value == B.workspace_bytes(w, h, shape), (w, h, shape)
    assert B.slice_count(1, 106, 16, 16) == 1 and B.slice_count(1, 107, 16, 16) == 2
    w, h, shape = 1920, 1080, (16, 16, 8)
    assert size(w, h, *shape, C.byref(n)) == 0
    big = n.value
    # non-null pointers that are never dereferenced: every call below fails before any device work
    a, b, c, g = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0x4000)
    # brush_bilagrid_forward(pred, grid, gw, gh, gl, w, h, out, stream)
    ok = [a, g, 16, 16, 8, w, h, b, None]
    for i in (0, 1, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.brush_bilagrid_forward(*bad) == INVALID, i
    for dims in bad_dims:
        bad = list(ok)
        bad[5], bad[6] = dims
        assert lib.brush_bilagrid_forward(*bad) == INVALID, dims
    for gr in bad_grids:
        bad = list(ok)
        bad[2:5] = gr
        assert lib.brush_bilagrid_forward(*bad) == INVALID, gr
    for i, p in ((7, a), (7, C.c_void_p(0x2004)), (0, C.c_void_p(0x1008)), (1, C.c_void_p(0x4004))):
        bad = list(ok)
        bad[i] = p  # out aliases pred; images and the grid are 16-byte aligned
        assert lib.brush_bilagrid_forward(*bad) == INVALID, (i, p)
    # brush_bilagrid_backward(pred, v_out, grid, gw, gh, gl, w, h, v_pred, v_grid, ws, ws_bytes, stream)
    ok = [a, b, g, 16, 16, 8, w, h, b, c, C.c_void_p(0x5000), big, None]
    # brush_bilagrid_backward_adam(pred, v_out, cfg, gw, gh, gl, w, h, v_pred, grid, m1, m2, v_grid, ws, ws_bytes, stream)
    cfg = _lib.BrushBilagridAdam(2e-3, 0.9, 0.999, 1e-15, 10.0, 1)
    m1, m2 = C.c_void_p(0x6000), C.c_void_p(0x7000)
    ok_adam = [a, b, C.byref(cfg), 16, 16, 8, w, h, b, g, m1, m2, c, C.c_void_p(0x5000), big, None]
    for fn, args, ptrs, ws_at, misalign in (
            (lib.brush_bilagrid_backward, ok, (0, 1, 2, 8, 9, 10), 11,
             ((0, 0x1004), (1, 0x2008), (8, 0x200c), (2, 0x4004), (9, 0x3002), (10, 0x5004))),
            (lib.brush_bilagrid_backward_adam, ok_adam, (0, 1, 2, 8, 9, 10, 11, 12, 13), 14,
             ((0, 0x1004), (1, 0x2008), (8, 0x200c), (9, 0x4004), (10, 0x6002), (11, 0x7001), (12, 0x3002),
              (13, 0x5004)))):
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == INVALID, i
        for dims in bad_dims:
            bad = list(args)
            bad[6], bad[7] = dims
            assert fn(*bad) == INVALID, dims
        for gr in bad_grids:
            bad = list(args)
            bad[3:6] = gr
            assert fn(*bad) == INVALID, gr
        for i, addr in misalign:
            bad = list(args)
            bad[i] = C.c_void_p(addr)
            assert fn(*bad) == INVALID, (i, hex(addr))
        bad = list(args)
        bad[8] = a  # v_pred == pred
        assert fn(*bad) == INVALID
        bad = list(args)
        bad[ws_at] = big - 1
        assert fn(*bad) == SMALL
    zero_time = _lib.BrushBilagridAdam(2e-3, 0.9, 0.999, 1e-15, 10.0, 0)  # time is 1-based
    bad = list(ok_adam)
    bad[2] = C.byref(zero_time)
    assert lib.brush_bilagrid_backward_adam(*bad) == INVALID
    assert C.sizeof(_lib.BrushBilagridAdam) == 24
    assert [f[0] for f in _lib.BrushBilagridAdam._fields_] == ["lr", "beta1", "beta2", "epsilon", "tv", "time"]


# ---------------------------------------------------------------------------- 6. configuration, Python surface, CLI
def test_config_refusals():
    import brush_amd

    c = brush_amd.TrainConfig()
    assert c.bilagrid_opt is False and tuple(c.bilagrid_shape) == (16, 16, 8)
    assert c.lr_bilagrid == 2e-3 and c.lr_bilagrid_decay == 0.01 and c.bilagrid_tv == 10.0
    brush_amd.TrainConfig(bilagrid_opt=True).check()
    for kw, field in ((dict(bilagrid_shape=(1, 16, 8)), "bilagrid_shape"), (dict(bilagrid_shape=(16, 65, 8)), "bilagrid_shape"),
                      (dict(bilagrid_shape=(16, 16, 9)), "bilagrid_shape"), (dict(bilagrid_shape=(16, 16)), "bilagrid_shape"),
                      (dict(bilagrid_shape=(16.5, 16, 8)), "bilagrid_shape"),
                      (dict(lr_bilagrid=-1.0), "lr_bilagrid"), (dict(lr_bilagrid_decay=-0.1), "lr_bilagrid_decay"),
                      (dict(bilagrid_tv=-1.0), "bilagrid_tv"), (dict(bilagrid_tv=float("nan")), "bilagrid_tv"),
                      (dict(bilagrid_opt=True, exposure_opt=True), "bilagrid_opt"),
                      (dict(bilagrid_opt=True, densify_by="error"), "bilagrid_opt")):
        with pytest.raises(ValueError, match=field):
            brush_amd.TrainConfig(**kw).check()
    with pytest.raises(ValueError, match="bilagrid_opt.*multi-rank"):
        brush_amd.TrainConfig(bilagrid_opt=True).check(multi_rank=True)


def test_python_surface_without_gpu():
    import torch

    import brush_amd
    from brush_amd import bilagrid as BG

    for name in ("apply_bilagrid", "bilagrid_identity", "bilagrid_tv", "BilagridTable"):
        assert getattr(brush_amd, name) is getattr(BG, name)
    assert "bilagrids" in inspect.signature(brush_amd.SplatTrainer.step).parameters
    for name in ("forward", "backward_step", "grids", "state_dict", "load_state_dict"):
        assert callable(getattr(BG.BilagridTable, name)), name
    sig = inspect.signature(BG.BilagridTable.__init__).parameters
    assert tuple(sig["shape"].default) == (16, 16, 8) and sig["tv"].default == 10.0
    # the schedule: lr_bilagrid at step 0, lr_bilagrid * lr_bilagrid_decay at total_steps
    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig(total_steps=1000)
    tr.iter = 0
    assert tr._lr_bilagrid() == 2e-3
    tr.iter = 1000
    assert abs(tr._lr_bilagrid() - 2e-5) < 1e-17
    with pytest.raises(AssertionError, match="no CPU path"):
        BG.apply_bilagrid(torch.zeros((4, 4, 4)), torch.zeros((8, 16, 16, 12)))
    with pytest.raises(AssertionError, match="no CPU path"):
        BG.BilagridTable(3, "cpu", 2e-3)
    with pytest.raises(ValueError, match="GW"):
        BG.check_shape((16, 16, 16))


def test_step_refuses_bilagrids_before_any_device_work():
    """Every check runs before any device work: a trainer that was never initialised and no splats are enough."""
    import brush_amd

    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig()
    tr.filter3d = None
    tr.iter = 0
    table = object()
    with pytest.raises(ValueError, match="bilateral grids is single-view"):
        tr.step(None, None, None, exchange=object(), view_index=0, bilagrids=table)
    with pytest.raises(ValueError, match="bilateral grids is single-view"):
        tr.step(None, None, None, grad_sync=lambda b, a: None, view_index=0, bilagrids=table)
    with pytest.raises(ValueError, match="bilagrids cannot be combined with exposures"):
        tr.step(None, None, None, view_index=0, bilagrids=table, exposures=object())
    with pytest.raises(ValueError, match="bilagrids needs view_index"):
        tr.step(None, None, None, bilagrids=table)
    tr.config = brush_amd.TrainConfig(densify_by="error")
    with pytest.raises(ValueError, match="densify_by='error' cannot be combined with the bilateral grids"):
        tr.step(None, None, None, view_index=0, bilagrids=table)


def test_cli_flags_and_log_keys():
    from brush_amd import train_loop as TL

    p = TL.parser()
    a = p.parse_args(["data"])
    assert a.bilagrid_opt is False and a.export_bilagrids is None and a.bilagrid_shape is None and a.bilagrid_tv == 10.0
    a = p.parse_args(["data", "--bilagrid-opt", "--bilagrid-shape", "8,8,4", "--bilagrid-tv", "2.5",
                      "--export-bilagrids", "g.npz"])
    assert a.bilagrid_opt is True and a.bilagrid_shape == "8,8,4" and a.bilagrid_tv == 2.5
    assert a.export_bilagrids == "g.npz"
    log = TL.TrainLog(0, np.zeros(0, np.float32))
    js = log.to_json()
    assert js["bilagrid_opt"] is False and js["bilagrid_shape"] is None
    log.bilagrid_opt, log.bilagrid_shape = True, (8, 8, 4)
    js = log.to_json()
    assert js["bilagrid_opt"] is True and js["bilagrid_shape"] == [8, 8, 4]
    # a bad shape or the two colour models together end the command line before a dataset is looked at
    for argv in (["nowhere", "--bilagrid-opt", "--bilagrid-shape", "8,8"],
                 ["nowhere", "--bilagrid-opt", "--bilagrid-shape", "8,x,4"],
                 ["nowhere", "--bilagrid-opt", "--exposure-opt"]):
        with pytest.raises(SystemExit):
            TL.main(argv)


# ---------------------------------------------------------------------------- 7. resources
def test_bilagrid_kernels_static_lds_and_spills(lib):
    """Every instantiation is present; static LDS is what bilagrid.hip's header says (the backward stages the wave sums
    of 48 doubles: 4 x 48 x 8 = 1536 bytes; the others none); no spills, no scratch."""
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_bilagrid_")
    want = {("k_bilagrid_forward", None): 0, ("k_bilagrid_backward", None): 1536,
            ("k_bilagrid_finalize", "Lb0E"): 0, ("k_bilagrid_finalize", "Lb1E"): 0}
    seen = []
    for name, r in res.items():
        m = re.search(r"N_1\d+(k_bilagrid_[a-z]+)(?:I(Lb\dE)E|E)", name)
        assert m, name
        key = (m.group(1), m.group(2))
        assert key in want, name
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"]) == (0, 0, 0), name
        assert r["group_segment_fixed_size"] == want[key], name
        seen.append(key)
    assert sorted(seen, key=str) == sorted(want, key=str)
