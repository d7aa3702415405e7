"""CPU checks of background colour and loss masks (brush_compose_*, brush_amd/compose.py): the float32 restatement
against float64 autograd, the kept / not-kept selection, the entry points' argument checks, the compiled kernels'
resources, the dataset readers' masks and the Python / CLI surface.  Nothing here needs a GPU.

Rounding bounds are stated in u = 2^-24 times the sum of the absolute values of an output's terms (compose_ref's
float64 functions return it beside every output), times the number n of f32 roundings a term of that output can pass
through, as gamma_n = n u / (1 - n u):
    v_pred.w  n = 4  (a product, two additions, the subtraction)        v_pred.c  n = 0 (a copy)
    out.c     n = 3  (1 - alpha, its product with b_c, the addition)    out.w     n = 0
    target.c  n = 3  (1 - G_a, its product with b_c, the addition; G_c G_a passes two), a u8 target one more (b / 255)
"""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest

from tests import compose_ref as R
from tests import eval_data as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BG = (0.3, 0.6, 0.9)   # no power of two: every product rounds


def gamma(n):
    return n * U / (1.0 - n * U)


COMBOS = [(bg, mk, cg) for bg in (None, BG) for mk in (None, "random") for cg in (3, 4) if bg is not None or mk]


# ---------------------------------------------------------------------------- 1. the restatements
def _torch_forward64(pred, gt, background, mask):
    """The definition in torch float64, differentiable in pred: an independent statement (where / broadcasting) of
    compose_ref.forward64."""
    import torch

    a = pred[..., 3:4]
    if background is not None:
        b = torch.tensor(np.asarray(background, dtype=np.float32).astype(np.float64))
        out = torch.cat([pred[..., :3] + (1.0 - a) * b, a], dim=2)
        target = gt[..., :3] * gt[..., 3:4] + (1.0 - gt[..., 3:4]) * b if gt.shape[2] == 4 else gt
    else:
        out, target = pred, gt
    if mask is not None:
        keep = torch.from_numpy(np.asarray(mask) != 0)[..., None]
        out = torch.where(keep, out, torch.zeros_like(out))
        target = torch.where(keep, target, torch.zeros_like(target))
    return out, target


@pytest.mark.parametrize("bg,mask_kind,cg", COMBOS)
def test_f32_restatement_against_float64_autograd(bg, mask_kind, cg):
    import torch

    pred, gt, mask, wgt = R.case(33, 31, cg, np.float32, mask_kind, 7 + cg)
    p64 = torch.from_numpy(pred.astype(np.float64)).requires_grad_(True)
    out_t, target_t = _torch_forward64(p64, torch.from_numpy(gt.astype(np.float64)), bg, mask)
    (out_t * torch.from_numpy(wgt.astype(np.float64))).sum().backward()
    # the two float64 statements agree (their own rounding: a few 2^-53 of the terms)
    out64, target64, out_mag, target_mag = R.forward64(pred, gt, None if bg is None else np.float32(bg), mask)
    assert np.abs(out_t.detach().numpy() - out64).max() <= 8 * 2.0 ** -53 * max(out_mag.max(), 1.0)
    assert np.abs(target_t.detach().numpy() - target64).max() <= 8 * 2.0 ** -53 * max(target_mag.max(), 1.0)
    v64, v_mag = R.backward64(wgt, None if bg is None else np.float32(bg), mask)
    assert np.abs(p64.grad.numpy() - v64).max() <= 8 * 2.0 ** -53 * max(v_mag.max(), 1.0)
    # the f32 restatement against them
    out32, target32 = R.forward32(pred, gt, bg, mask)
    v32 = R.backward32(wgt, bg, mask)
    assert out32.dtype == np.float32 and target32.dtype == np.float32 and v32.dtype == np.float32
    assert target32.shape == (31, 33, 3 if bg is not None else cg)
    want = p64.grad.numpy()
    assert (np.abs(v32[..., 3] - want[..., 3]) <= gamma(4) * v_mag[..., 3]).all()
    assert np.array_equal(v32[..., :3].astype(np.float64), want[..., :3])         # copies (or zeros)
    assert (np.abs(out32[..., :3] - out64[..., :3]) <= gamma(3) * out_mag[..., :3]).all()
    assert np.array_equal(out32[..., 3].astype(np.float64), out64[..., 3])
    assert (np.abs(target32 - target64) <= gamma(3) * target_mag).all()
    if bg is None:  # nothing is computed: bits kept
        assert np.array_equal(out32.view(np.uint32)[R._keep(mask, (31, 33))], pred.view(np.uint32)[R._keep(mask, (31, 33))])


def test_u8_target_is_one_division():
    gt = np.arange(256, dtype=np.uint8).reshape(1, 64, 4)
    g = R.gt_f32(gt)
    assert g.dtype == np.float32 and g[0, 0, 0] == 0.0 and g[0, 63, 3] == 1.0
    exact = gt.astype(np.float64) / 255.0
    assert (np.abs(g - exact) <= U * exact).all()
    assert not np.array_equal(g, gt.astype(np.float32) * np.float32(1.0 / 255.0))  # a reciprocal multiply differs
    pred, _, mask, _ = R.case(64, 1, 4, np.uint8, "random", 3)
    _, t8 = R.forward32(pred, gt, BG, mask)
    _, t32 = R.forward32(pred, g, BG, mask)
    assert np.array_equal(t8.view(np.uint32), t32.view(np.uint32))
    _, t64, _, mag = R.forward64(pred, gt, np.float32(BG), mask)
    assert (np.abs(t8 - t64) <= gamma(4) * mag).all()


@pytest.mark.parametrize("bg", [None, BG])
@pytest.mark.parametrize("cg", [3, 4])
def test_selection_zeroes_and_does_not_leak_nan(bg, cg):
    pred, gt, mask, v = R.case(7, 5, cg, np.float32, "random", 11)
    mask[0, 0], mask[0, 1], mask[4, 6] = 0, 0, 1          # 1 keeps as 255 does
    pred[0, 0], gt[0, 1], v[0, 0] = np.nan, np.inf, np.nan  # under the mask
    pred[1, 1, 3] = -0.0
    out, target = R.forward32(pred, gt, bg, mask)
    vp = R.backward32(v, bg, mask)
    gone = mask == 0
    for a in (out, target, vp):
        assert np.isfinite(a).all()
        assert (a.view(np.uint32)[gone] == 0).all()         # +0.0f: every word, the sign bit too
    assert out[4, 6, 3] == pred[4, 6, 3] and vp[4, 6, 0] == v[4, 6, 0]
    # all-zero and all-255 masks: everything gone / the call without a mask
    zero, full = np.zeros((5, 7), np.uint8), np.full((5, 7), 255, np.uint8)
    pred, gt, _, v = R.case(7, 5, cg, np.float32, None, 12)
    o0, t0 = R.forward32(pred, gt, bg, zero)
    assert not o0.view(np.uint32).any() and not t0.view(np.uint32).any()
    assert not R.backward32(v, bg, zero).view(np.uint32).any()
    o1, t1 = R.forward32(pred, gt, bg, full)
    if bg is not None:
        o2, t2 = R.forward32(pred, gt, bg, None)
        assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(t1, t2)
        assert np.array_equal(R.backward32(v, bg, full), R.backward32(v, bg, None))
    else:
        assert np.array_equal(o1.view(np.uint32), pred.view(np.uint32)) and np.array_equal(t1, gt)
        assert np.array_equal(R.backward32(v, None, full), v)


def test_background_black_and_opaque_pixels():
    """Over black a premultiplied render is itself and a straight-alpha target is premultiplied; an opaque pixel and an
    opaque target ignore the colour; the alpha gradient is -b . v."""
    pred, gt, _, v = R.case(9, 4, 4, np.float32, None, 5)
    out, target = R.forward32(pred, gt, (0.0, 0.0, 0.0), None)
    assert np.array_equal(out, pred) and np.array_equal(target, gt[..., :3] * gt[..., 3:4])
    assert np.array_equal(R.backward32(v, (0.0, 0.0, 0.0), None), v)
    pred[..., 3], gt[..., 3] = 1.0, 1.0
    out, target = R.forward32(pred, gt, BG, None)
    assert np.array_equal(out, pred) and np.array_equal(target, gt[..., :3])
    vp = R.backward32(np.concatenate([np.ones((4, 9, 3), np.float32), np.zeros((4, 9, 1), np.float32)], 2),
                      (0.25, 0.5, 1.0), None)
    assert (vp[..., 3] == -1.75).all()


# ---------------------------------------------------------------------------- 2. the ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_compose_entry_points_validate_arguments_without_gpu(lib):
    from brush_amd import _lib

    INVALID = -1
    for name in ("brush_compose_forward", "brush_compose_backward"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)
    # non-null pointers that are never dereferenced: every call below fails before any device work
    p, g, m, b, o, t = (C.c_void_p(x) for x in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))
    w, h = 1920, 1080
    U8, F32 = _lib.EVAL_GT_U8, _lib.EVAL_GT_F32
    # brush_compose_forward(pred, gt, gt_dtype, gt_channels, mask, background, w, h, out_pred, out_gt, stream)
    ok = [p, g, U8, 3, m, b, w, h, o, t, None]
    fwd = lib.brush_compose_forward

    def bad(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fwd(*a)

    assert bad(_4=None, _5=None) == INVALID                       # neither a mask nor a background
    for i in (0, 1, 8, 9):
        assert bad(**{f"_{i}": None}) == INVALID, i               # a required pointer
    for dtype in (2, 0xFFFFFFFF):
        assert bad(_2=dtype) == INVALID                           # gt_dtype
    for ch in (0, 1, 2, 5):
        assert bad(_3=ch) == INVALID                              # gt_channels
        assert bad(_2=F32, _3=ch) == INVALID
    for dims in ((0, h), (w, 0), (1 << 14, 1 << 14), (1 << 16, 1 << 16)):
        assert bad(_6=dims[0], _7=dims[1]) == INVALID, dims       # w h = 0, 2^28, 2^32 (no wrap to 0 either)
    for i in (0, 1, 8, 9):
        assert bad(**{f"_{i}": C.c_void_p(ok[i].value + 4)}) == INVALID, i   # images are 16-byte aligned
    assert bad(_5=C.c_void_p(0x4002)) == INVALID                  # background: 4 bytes
    assert bad(_8=p) == INVALID                                   # out_pred aliases pred
    assert bad(_9=g) == INVALID and bad(_9=o) == INVALID          # out_gt aliases gt / out_pred
    # brush_compose_backward(v_out, mask, background, w, h, v_pred, stream)
    bwd = lib.brush_compose_backward
    assert bwd(p, None, None, w, h, o, None) == INVALID
    assert bwd(None, m, b, w, h, o, None) == INVALID
    assert bwd(p, m, b, w, h, None, None) == INVALID
    for dims in ((0, h), (w, 0), (1 << 14, 1 << 14)):
        assert bwd(p, m, b, dims[0], dims[1], o, None) == INVALID, dims
    assert bwd(C.c_void_p(0x1008), m, b, w, h, o, None) == INVALID
    assert bwd(p, m, b, w, h, C.c_void_p(0x5004), None) == INVALID
    assert bwd(p, m, C.c_void_p(0x4001), w, h, o, None) == INVALID


def test_compose_kernels_use_no_lds_no_scratch_no_spills():
    """Every instantiation is in the library: the forward for {u8, f32} x {3, 4} channels x {background, mask, both},
    the backward for {background, mask, both}."""
    from brush_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_diff
    finally:
        sys.path.pop(0)
    res = kernel_diff.resources(_lib.LIB_PATH, r"k_compose_")
    options = ("Lb1ELb0E", "Lb0ELb1E", "Lb1ELb1E")   # <BG, MASK>
    want = {f"k_compose_forwardI{gt}Li{cg}E{o}" for gt in "hf" for cg in (3, 4) for o in options}
    want |= {f"k_compose_backwardI{o}" for o in options}
    found = set()
    for name, r in res.items():
        hit = [k for k in want if k in name]
        assert len(hit) == 1, name
        found.add(hit[0])
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (name, r)
    assert found == want and len(res) == 15, sorted(res)


# ---------------------------------------------------------------------------- 3. readers
def _mask_image(w, h, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) > 0.4).astype(np.uint8) * 255
    m[0, 0], m[h - 1, w - 1] = 0, 7   # any nonzero value keeps
    return m


def test_nerfstudio_mask_path(tmp_path):
    from brush_amd import dataset as D

    root = str(tmp_path / "nerf")
    w, h = 48, 40
    E.write_nerf(root, w, h, n_train=3, with_val=False)
    masks = {0: _mask_image(w, h, 1), 2: _mask_image(w, h, 2)}
    os.makedirs(os.path.join(root, "masks"))
    path = os.path.join(root, "transforms_train.json")
    with open(path) as f:
        scene = json.load(f)
    for i, m in masks.items():
        rgb = np.stack([m, np.zeros_like(m), np.zeros_like(m)], 2) if i == 2 else m  # the first channel counts
        with open(os.path.join(root, "masks", f"m_{i}.png"), "wb") as f:
            f.write(E.png_bytes(rgb))
        scene["frames"][i]["mask_path"] = f"masks/m_{i}.png"
    with open(path, "w") as f:
        json.dump(scene, f)
    views = D.read_nerf_synthetic(root).train.views
    assert views[1].mask is None
    for i, m in masks.items():
        assert views[i].mask.dtype == np.uint8 and np.array_equal(views[i].mask, m)
    # max_resolution: the mask follows the image through resize_nearest
    small = D.read_nerf_synthetic(root, max_resolution=24).train.views
    assert small[0].image.shape[:2] == (20, 24)
    assert np.array_equal(small[0].mask, D.resize_nearest(masks[0], (20, 24)))
    # a mask of another size names its view
    with open(os.path.join(root, "masks", "m_0.png"), "wb") as f:
        f.write(E.png_bytes(_mask_image(10, 10, 3)))
    with pytest.raises(ValueError, match=r"r_0.*mask is 10x10"):
        D.read_nerf_synthetic(root)


def test_colmap_masks_directory(tmp_path):
    from brush_amd import dataset as D

    root = str(tmp_path / "colmap")
    w, h = 48, 40
    E.write_colmap(root, w, h, n_images=3)
    os.makedirs(os.path.join(root, "masks"))
    by_name, by_stem, loser = _mask_image(w, h, 4), _mask_image(w, h, 5), _mask_image(w, h, 6)
    for name, m in (("img_00.png.png", by_name), ("img_00.png", loser), ("img_01.png", by_stem)):
        with open(os.path.join(root, "masks", name), "wb") as f:
            f.write(E.png_bytes(m))
    views = D.read_colmap(root).train.views
    assert np.array_equal(views[0].mask, by_name)   # masks/<image name>.png wins over masks/<stem>.png
    assert np.array_equal(views[1].mask, by_stem)
    assert views[2].mask is None
    small = D.read_colmap(root, max_resolution=24).train.views
    assert np.array_equal(small[1].mask, D.resize_nearest(by_stem, small[1].image.shape[:2]))
    assert all(v.mask is None for v in D.read_colmap(root, load_images=False).train.views)
    with open(os.path.join(root, "masks", "img_02.png"), "wb") as f:
        f.write(E.png_bytes(_mask_image(w, h + 1, 7)))
    with pytest.raises(ValueError, match=r"img_02.*mask is 48x41"):
        D.read_colmap(root)


# ---------------------------------------------------------------------------- 4. Python surface and parsers
def test_background_parsers():
    import torch

    from brush_amd import compose as _fn  # the package attribute is the function
    from brush_amd.compose import as_background, check_background, parse_background

    assert callable(_fn)
    assert parse_background("white") == "white" and parse_background("Black") == "black"
    assert parse_background("random") == "random"
    assert parse_background("0.25,0.5,1") == (0.25, 0.5, 1.0)
    for text in ("", "grey", "1,2", "1,2,3,4", "a,b,c", "nan,0,0", "inf,0,0"):
        with pytest.raises(ValueError, match="--background"):
            parse_background(text)
    assert as_background(None, "cpu") is None
    for spec, want in (("white", (1, 1, 1)), ("black", (0, 0, 0)), ((0.25, 0.5, 1.0), (0.25, 0.5, 1.0))):
        t = as_background(spec, "cpu")
        assert t.dtype == torch.float32 and tuple(t.shape) == (3,) and tuple(t.tolist()) == tuple(map(float, want))
    with pytest.raises(ValueError, match="Generator"):
        as_background("random", "cpu")
    g = torch.Generator().manual_seed(5)
    a = as_background("random", "cpu", g)
    assert np.array_equal(a.numpy(), torch.rand(3, generator=torch.Generator().manual_seed(5)).numpy())
    for bad in ("grey", (1, 2), (1, 2, "x"), 3, True):
        with pytest.raises(ValueError):
            check_background(bad)
    t = torch.zeros(3)
    assert as_background(t, "cpu") is t
    with pytest.raises(ValueError):
        as_background(torch.zeros(4), "cpu")


def test_python_surface_without_gpu():
    import torch

    import brush_amd
    from brush_amd import compose as CM  # noqa: F401
    from brush_amd.compose import compose_backward, compose_forward

    assert brush_amd.compose_forward is compose_forward and brush_amd.compose_backward is compose_backward
    c = brush_amd.TrainConfig()
    assert c.background is None and c.use_masks is True
    params = inspect.signature(brush_amd.SplatTrainer.step).parameters
    assert params["background"].default is None and params["gt_mask"].default is None
    from brush_amd.eval import EvalView, eval_stats
    params = inspect.signature(eval_stats).parameters
    assert params["background"].default is None and params["use_masks"].default is True
    assert EvalView(None, None, 1.0, 1.0).valid_fraction == 1.0
    assert brush_amd.dataset.SceneView("n", None, None).mask is None
    with pytest.raises(ValueError, match="background"):
        brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer).__init__(None, brush_amd.TrainConfig(background="grey"))
    with pytest.raises(AssertionError, match="no CPU path"):
        compose_forward(torch.zeros((4, 4, 4)), torch.zeros((4, 4, 3)), background=torch.zeros(3))
    with pytest.raises(AssertionError, match="no CPU path"):
        compose_backward(torch.zeros((4, 4, 4)), background=torch.zeros(3))


def test_cli_flags_and_log_keys():
    from brush_amd import eval as EV
    from brush_amd import train_loop as TL

    a = TL.parser().parse_args(["data"])
    assert a.background is None and a.no_masks is False
    a = TL.parser().parse_args(["data", "--background", "random", "--no-masks"])
    assert a.background == "random" and a.no_masks is True
    a = EV.parser().parse_args(["splats.ply", "data", "--background", "1,1,1", "--no-masks"])
    assert a.background == "1,1,1" and a.no_masks is True
    log = TL.TrainLog(0, np.zeros(0, np.float32))
    js = log.to_json()
    assert js["background"] is None and js["masked_views"] == 0
    log.background, log.masked_views = (0.25, 0.5, 1.0), 3
    js = json.loads(json.dumps(log.to_json()))
    assert js["background"] == [0.25, 0.5, 1.0] and js["masked_views"] == 3
