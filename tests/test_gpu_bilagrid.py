"""Per-view bilateral grids on the GPU: the kernels of brush_amd/csrc/bilagrid.hip against the float64 restatement of
tests/bilagrid_ref64.py, the consequences of the lerp form against the exposure kernels' own outputs, the Adam step with
the prior, repeatability and graph replay, the autograd function, a frozen fit, the trainer's three optimizer paths and a
scene trained end to end from images with per-view vignettes and luminance-dependent gains.

Rounding bounds are stated in u = 2^-24 times the sum of the absolute values of an output's terms (bilagrid_ref64
returns it beside every output).  The worst observed fraction of every bound is recorded through tests/margins.py
(section "bilagrid"); BRUSH_BILAGRID_MARGINS=path makes a run write the same figures there, which is how
profiles/bilagrid_margins.json was made."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bilagrid_ref64 as B
from tests import eval_data as ED
from tests import exposure_ref64 as X
from tests import margins
from tests import test_gpu_exposure as TE
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
DEFAULT = (16, 16, 8)
# (1,107): the smallest image at which the backward of the default grid cuts a cell's rows into more than one slice, and
# unevenly.  slice_count gives min(512 / 225 = 2, ceil(rows_max / 8)) slices with rows_max = ceil((h - 1) / 15) + 1, which
# first exceeds 8 at h = 107 (h = 106: ceil(105 / 15) + 1 = 8); the cells then hold 8 or 7 rows, and 7 = 4 + 3.  One
# column is the fewest pixels such an image can have.  (The small grids slice earlier: (2,2,2) on (33,31) runs 4 slices
# of 8, 8, 8 and 7 rows.)
SLICED = (1, 107)
IMAGES = [(1, 1), (2, 2), (7, 5), (64, 1), (1, 64), (31, 16), (65, 3), (33, 31), (128, 128), SLICED, (1920, 1080)]
CASES = [(w, h, DEFAULT) for w, h in IMAGES] + [(w, h, s) for s in ((2, 2, 2), (5, 3, 4))
                                                for w, h in ((7, 5), (33, 31), (128, 128))]
# Forward, per colour channel: M is three nested lerps of three rounded operations each (a subtraction, a product, an
# addition: 9 u on the sum of its terms), the expression on M four products and three additions, of which the chain
# carries 4 u as in the exposure kernel: 13 u to first order, 14 with the second-order terms.
C_FORWARD = 14
# v_pred: the M part as above with three products and two additions (9 + 3 = 12 u, alpha one more addition: 13).  The
# luminance part: S = L1 - L0 carries the two planes' 6 u and its own subtraction (7), the dot product 4, the product
# with v' 1, the sum over the channels 2, the products with GL - 1 and with the luma weight 2, the final addition 1: 17 u,
# 18 with the second-order terms.  One constant for all four channels.
C_V_PRED = 18
MARGINS = {}


def _record(name, value):
    MARGINS[name] = value
    margins.record("bilagrid", name, value, tid="tests/test_gpu_bilagrid.py")


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    path = os.environ.get("BRUSH_BILAGRID_MARGINS")
    if MARGINS and path:
        with open(path, "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)


deterministic = TE.deterministic
_np, _bits, _worst, _ulp_ok = TE._np, TE._bits, TE._worst, TE._ulp_ok


# ---------------------------------------------------------------------------- helpers: the ABI on torch tensors
def _lib():
    from brush_amd import _lib as L

    return L


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _shape_of(G):
    return int(G.shape[2]), int(G.shape[1]), int(G.shape[0])


def _ws(w, h, shape, dev):
    import torch

    from brush_amd.bilagrid import workspace_bytes

    n = workspace_bytes(w, h, shape)
    assert n == B.workspace_bytes(w, h, shape)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def abi_forward(pred, G, out=None):
    import torch

    L = _lib()
    h, w = pred.shape[:2]
    out = torch.empty_like(pred) if out is None else out
    L.check(L.lib().brush_bilagrid_forward(pred.data_ptr(), G.data_ptr(), *_shape_of(G), w, h, out.data_ptr(),
                                           _stream()), "forward")
    return out


def abi_backward(pred, v_out, G, alias=False, v_pred=None, v_G=None, ws=None):
    import torch

    L = _lib()
    h, w = pred.shape[:2]
    if alias:
        v_out = v_out.clone()
        v_pred = v_out
    elif v_pred is None:
        v_pred = torch.empty_like(pred)
    v_G = torch.empty_like(G) if v_G is None else v_G
    ws, n = _ws(w, h, _shape_of(G), pred.device) if ws is None else ws
    L.check(L.lib().brush_bilagrid_backward(pred.data_ptr(), v_out.data_ptr(), G.data_ptr(), *_shape_of(G), w, h,
                                            v_pred.data_ptr(), v_G.data_ptr(), ws.data_ptr(), n, _stream()), "backward")
    return v_pred, v_G


def abi_backward_adam(pred, v_out, cfg, G_view, m1_view, m2_view):
    """G_view / m1_view / m2_view: one view's [GL,GH,GW,12] slices of the tables, updated in place."""
    import torch

    L = _lib()
    h, w = pred.shape[:2]
    v_pred = torch.empty_like(pred)
    v_G = torch.empty_like(G_view)
    ws, n = _ws(w, h, _shape_of(G_view), pred.device)
    L.check(L.lib().brush_bilagrid_backward_adam(pred.data_ptr(), v_out.data_ptr(), C.byref(cfg), *_shape_of(G_view), w,
                                                 h, v_pred.data_ptr(), G_view.data_ptr(), m1_view.data_ptr(),
                                                 m2_view.data_ptr(), v_G.data_ptr(), ws.data_ptr(), n, _stream()),
            "backward_adam")
    return v_pred, v_G


_CASES = {}


def _inputs(w, h, shape):
    """pred in [0,1] with a fifth of the pixels at alpha = 0 (half of those empty altogether: luminance 0), a tenth of
    the colours doubled (luminance >= 1 at many) and a twentieth negated (luminance < 0); signed v_out;
    G = identity + N(0, 0.2).  No negative zeros."""
    gw, gh, gl = shape
    rng = np.random.default_rng(1000 * w + h + 7 * gw + gl)
    pred = rng.random((h, w, 4), dtype=np.float32)
    pred[..., :3][rng.random((h, w)) < 0.1] *= np.float32(2.0)
    pred[..., :3][rng.random((h, w)) < 0.05] *= np.float32(-0.3)
    empty = rng.random((h, w)) < 0.2
    pred[..., 3][empty] = 0.0
    pred[empty & (rng.random((h, w)) < 0.5)] = 0.0
    pred += np.float32(0.0)
    v_out = rng.standard_normal((h, w, 4)).astype(np.float32)
    G = (B.identity(shape) + 0.2 * rng.standard_normal((gl, gh, gw, 12))).astype(np.float32)
    return pred, v_out, G


def _case(w, h, shape, dev, ref=True):
    """Inputs and the float64 reference of one case, computed once and shared."""
    import torch

    key = (w, h, shape)
    if key not in _CASES:
        _CASES[key] = _inputs(w, h, shape) + (None,)
    pred, v_out, G, r = _CASES[key]
    if ref and r is None:
        r = {"out": B.forward(pred, G), "v_pred": B.backward_image(pred, v_out, G),
             "v_G": B.backward_grid(pred, v_out, shape)}
        _CASES[key] = (pred, v_out, G, r)
    tt = lambda a: torch.from_numpy(a).to(dev)
    return tt(pred), tt(v_out), tt(G), r


def _accumulation_terms(w, h, shape):
    """Float64 roundings behind one word of v_grid, counted: the longest per-lane chain of additions, 6 tree steps and
    3 wave additions of block_sum_words, 4 cells x slices rows in the finalize kernel; and per term the weight's three
    complements and two products and the product with v' p: 6."""
    gw, gh, _ = shape
    return B.longest_chain(w, h, gw, gh) + 6 + 3 + 4 * B.slice_count(w, h, gw, gh) + 6


# ---------------------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("w,h,shape", CASES)
def test_forward_and_backward_match_the_restatement(dev, w, h, shape):
    import torch

    pred, v_out, G, ref = _case(w, h, shape, dev)
    out = abi_forward(pred, G)
    v_pred, v_G = abi_backward(pred, v_out, G)
    v_alias, v_G_alias = abi_backward(pred, v_out, G, alias=True)
    torch.cuda.synchronize()
    want, mag = ref["out"]
    r_fwd = _worst(_np(out), want, C_FORWARD * U * mag)
    want, mag = ref["v_pred"]
    r_vp = _worst(_np(v_pred), want, C_V_PRED * U * mag)
    # v_grid: one rounding to f32 plus the float64 accumulation
    want, mag, reached = ref["v_G"]
    tol = U * np.abs(want) + _accumulation_terms(w, h, shape) * 2.0 ** -53 * mag
    r_G = _worst(_np(v_G), want, tol)
    print(f"bilagrid {w}x{h} {shape}: err/tol forward {r_fwd:.3f} v_pred {r_vp:.3f} v_grid {r_G:.3f}; "
          f"{int(reached.sum())} of {reached.size} vertices reached, {B.slice_count(w, h, shape[0], shape[1])} slices")
    _record(f"kernels_{w}x{h}_{'x'.join(map(str, shape))}", dict(forward=r_fwd, v_pred=r_vp, v_grid=r_G))
    assert r_fwd <= 1.0 and r_vp <= 1.0 and r_G <= 1.0
    assert np.array_equal(_bits(out)[..., 3], _bits(pred)[..., 3])  # alpha is a copy
    assert not _bits(v_G)[~reached].any()  # a vertex no pixel reaches: +0 in every word
    # v_pred written over v_out: the same bits
    assert np.array_equal(_bits(v_alias), _bits(v_pred)) and np.array_equal(_bits(v_G_alias), _bits(v_G))


def test_the_sliced_case_is_sliced_unevenly():
    w, h = SLICED
    assert B.slice_count(w, h - 1, 16, 16) == 1 and B.slice_count(w, h, 16, 16) == 2
    rows = [B.cell_first(c + 1, h, 16) - B.cell_first(c, h, 16) for c in range(15)]
    assert max(rows) == 8 and 7 in rows
    for ww, hh in IMAGES:
        if hh < h:
            assert B.slice_count(ww, hh, 16, 16) == 1, (ww, hh)


# ---------------------------------------------------------------------------- 2. consequences of the lerp form
@pytest.mark.parametrize("w,h,shape", [(33, 31, DEFAULT), (128, 128, (5, 3, 4)), SLICED + (DEFAULT,)])
def test_lerp_form_consequences_against_the_exposure_kernels(dev, w, h, shape):
    import torch

    from brush_amd.bilagrid import bilagrid_identity

    pred, v_out, _, _ = _case(w, h, shape, dev, ref=False)
    gw, gh, gl = shape
    # 1. the identity grid returns pred bit for bit
    out = abi_forward(pred, bilagrid_identity(shape, dev))
    assert np.array_equal(_bits(out), _bits(pred))
    # 2. a constant grid is the exposure map: the forward's bits, an equal v_pred
    rng = np.random.default_rng(9)
    E = torch.from_numpy((X.IDENTITY + 0.2 * rng.standard_normal((3, 4))).astype(np.float32).reshape(12)).to(dev)
    G = E.repeat(gl, gh, gw, 1).contiguous()
    assert np.array_equal(_bits(abi_forward(pred, G)), _bits(TE.abi_forward(pred, E)))
    v_pred, v_G = abi_backward(pred, v_out, G)
    want_pred, want_E = TE.abi_backward(pred, v_out, E)
    assert torch.equal(v_pred, want_pred)
    # 3. the vertices' gradients add up to the exposure gradient: each of them carries its own bound (one rounding to
    #    f32 and the float64 accumulation), the exposure kernel's sum its own
    ref, mag = X.backward_exposure(_np(pred), _np(v_out))
    got = _np(v_G).astype(np.float64)
    total = got.sum(axis=(0, 1, 2)).reshape(3, 4)
    acc = (_accumulation_terms(w, h, shape) + gw * gh * gl) * 2.0 ** -53 * mag
    tol = U * np.abs(got).sum(axis=(0, 1, 2)).reshape(3, 4) + acc
    r_ref = _worst(total, ref, tol)
    r_exp = _worst(total, _np(want_E).astype(np.float64).reshape(3, 4), tol + U * np.abs(ref) + w * h * 2.0 ** -53 * mag)
    print(f"bilagrid {w}x{h} {shape}: sum of v_grid vs exposure gradient err/tol {r_ref:.3f} (reference) {r_exp:.3f} "
          f"(exposure kernel)")
    _record(f"constant_grid_{w}x{h}_{'x'.join(map(str, shape))}", dict(sum_vs_reference=r_ref, sum_vs_exposure=r_exp))
    assert r_ref <= 1.0 and r_exp <= 1.0


# ---------------------------------------------------------------------------- 3. repeatability and graph replay
@pytest.mark.parametrize("w,h", [(33, 31), (128, 128)])
def test_repeatable_and_graph_replay(dev, w, h):
    import torch

    pred, v_out, G, _ = _case(w, h, DEFAULT, dev, ref=False)
    first = (abi_forward(pred, G),) + abi_backward(pred, v_out, G)
    again = (abi_forward(pred, G),) + abi_backward(pred, v_out, G)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    out, v_pred, v_G = torch.zeros_like(pred), torch.zeros_like(pred), torch.zeros_like(G)
    ws = _ws(w, h, DEFAULT, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        abi_forward(pred, G, out=out)
        abi_backward(pred, v_out, G, v_pred=v_pred, v_G=v_G, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        abi_forward(pred, G, out=out)
        abi_backward(pred, v_out, G, v_pred=v_pred, v_G=v_G, ws=ws)
    for _ in range(2):
        out.zero_(), v_pred.zero_(), v_G.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (out, v_pred, v_G)):
            assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------- 4. non-finite input
def test_a_nan_pixel_changes_no_other_pixel(dev):
    import torch

    w, h = 33, 31
    pred, v_out, G, _ = _case(w, h, DEFAULT, dev, ref=False)
    out, (v_pred, _) = abi_forward(pred, G), abi_backward(pred, v_out, G)
    bad = pred.clone()
    bad[7, 11] = float("nan")
    out_bad, (v_pred_bad, _) = abi_forward(bad, G), abi_backward(bad, v_out, G)
    torch.cuda.synchronize()
    keep = np.ones((h, w), bool)
    keep[7, 11] = False
    assert np.array_equal(_bits(out_bad)[keep], _bits(out)[keep])
    assert np.array_equal(_bits(v_pred_bad)[keep], _bits(v_pred)[keep])
    assert np.isnan(_np(out_bad)[7, 11, :3]).all()


# ---------------------------------------------------------------------------- 5. Adam
def _adam_run(dev, steps=5, check=True):
    import torch

    w, h = 33, 31
    pred, _, G0, _ = _case(w, h, DEFAULT, dev, ref=False)
    L = _lib()
    V, view = 3, 1
    params = torch.from_numpy(B.identity(DEFAULT).astype(np.float32)).to(dev).repeat(V, 1, 1, 1, 1).contiguous()
    params[view] = G0
    params[2] = G0 * 0.5
    m1, m2 = torch.zeros_like(params), torch.zeros_like(params)
    m1[2], m2[2] = 0.25, 0.125
    lr, tv = 1e-2, 10.0
    worst = 0.0
    for t in range(1, steps + 1):
        rng = np.random.default_rng(70 + t)
        v_out_np = rng.standard_normal((h, w, 4)).astype(np.float32)
        v_out = torch.from_numpy(v_out_np).to(dev)
        before = (_np(params).copy(), _np(m1).copy(), _np(m2).copy())
        G_before = params[view].clone()
        cfg = L.BrushBilagridAdam(lr, B.BETA1, B.BETA2, B.EPS, tv, t)
        v_pred, v_G = abi_backward_adam(pred, v_out, cfg, params[view], m1[view], m2[view])
        if not check:
            continue
        v_pred_plain, v_G_plain = abi_backward(pred, v_out, G_before)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(v_G), _bits(v_G_plain)) and np.array_equal(_bits(v_pred), _bits(v_pred_plain))
        grad, _, _ = B.backward_grid(_np(pred), v_out_np, DEFAULT)
        wG, wm1, wm2 = B.adam_step(before[0][view], before[1][view], before[2][view], grad, lr, tv, t)
        for got, want, name in ((params, wG, "G"), (m1, wm1, "m1"), (m2, wm2, "m2")):
            ok, r = _ulp_ok(_np(got)[view], want)
            worst = max(worst, r)
            assert ok, (name, t, r)
            for other in (0, 2):  # the other views' grids keep their bits
                b = before[("G", "m1", "m2").index(name)]
                assert np.array_equal(_np(got)[other].view(np.uint32), b[other].view(np.uint32)), (name, t, other)
        assert bool((params[view] != G_before).any())
    torch.cuda.synchronize()
    return params, m1, m2, worst


def test_adam_steps_follow_the_restatement_and_do_not_race(dev):
    """Five steps with the prior on: the stepped view within one f32 ulp of the restatement fed the stored state,
    v_grid and v_pred the plain backward's bits, the other views untouched; and two runs of the five steps end in the
    same bits (a prior read from vertices another workgroup had already stepped would not)."""
    a = _adam_run(dev)
    print(f"bilagrid adam: worst distance to the restatement {a[3]:.3f} ulp over 5 steps")
    _record("adam_worst_ulp", a[3])
    b = _adam_run(dev, check=False)
    c = _adam_run(dev, check=False)
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(y), _bits(z))


# ---------------------------------------------------------------------------- 6. autograd
def test_apply_bilagrid_autograd(dev):
    import torch

    from brush_amd import apply_bilagrid, bilagrid_tv

    w, h, shape = 65, 3, DEFAULT
    pred, v_out, G, _ = _case(w, h, shape, dev, ref=False)
    img = pred.clone().requires_grad_(True)
    g = G.clone().requires_grad_(True)
    out = apply_bilagrid(img, g)
    g_img, g_g = torch.autograd.grad((out * v_out).sum(), [img, g])
    want_img, want_g = abi_backward(pred, v_out, G)
    assert np.array_equal(_bits(out), _bits(abi_forward(pred, G)))
    assert np.array_equal(_bits(g_img), _bits(want_img)) and np.array_equal(_bits(g_g), _bits(want_g))
    # the prior in torch ops on the device agrees with the restatement
    val = bilagrid_tv(g)
    (g_tv,) = torch.autograd.grad(val, g)
    want, _ = B.tv_grad(_np(G))
    assert abs(float(val.detach()) - B.tv(_np(G))[0]) <= 1e-5 * B.tv(_np(G))[0]
    assert np.abs(_np(g_tv) - want).max() <= 1e-5 * np.abs(want).max()


# ---------------------------------------------------------------------------- 7. frozen fit
def test_table_fits_a_known_grid(dev):
    """Only the table is stepped, from the identity, FIT_STEPS steps at FIT_LR with tv = 0, driven by
    v_out = (out - target) / npix; the restatement runs the same steps in float64 on the host.  Adam with eps = 1e-15
    amplifies rounding in words whose gradient vanishes, so the grids are not comparable word by word: the device run
    must reach the square root of the reference's residual ratio."""
    import torch

    from brush_amd.bilagrid import BilagridTable

    pred_np, _, target_np = B.fit_case()
    start_ref, end_ref = B.fit_reference()
    r_ref = end_ref / start_ref
    assert r_ref < 0.25
    pred = torch.from_numpy(pred_np).to(dev)
    target = torch.from_numpy(target_np.astype(np.float32)).to(dev)
    table = BilagridTable(2, dev, B.FIT_LR, B.FIT_SHAPE, tv=0.0)
    npix = pred.shape[0] * pred.shape[1]
    start = B.fit_residual(_np(table.forward(1, pred)), target_np)
    for _ in range(B.FIT_STEPS):
        v_out = (table.forward(1, pred) - target) / npix
        v_out[..., 3] = 0.0
        table.backward_step(1, pred, v_out)
    end = B.fit_residual(_np(table.forward(1, pred)), target_np)
    r = end / start
    print(f"bilagrid frozen fit: residual {start:.5f} -> {end:.6f} (ratio {r:.5f}); float64 on the host {r_ref:.5f}, "
          f"gate {math.sqrt(r_ref):.5f}")
    _record("frozen_fit", dict(steps=B.FIT_STEPS, lr=B.FIT_LR, ratio=r, ratio_reference=r_ref,
                               threshold=math.sqrt(r_ref)))
    assert r < math.sqrt(r_ref)
    assert table.steps == [0, B.FIT_STEPS]
    ident = B.identity(B.FIT_SHAPE).astype(np.float32)
    assert np.array_equal(_bits(table.params[0]), ident.view(np.uint32))
    other = BilagridTable(2, dev, 1.0, B.FIT_SHAPE)
    other.load_state_dict(table.state_dict())
    assert np.array_equal(_bits(other.params), _bits(table.params)) and other.steps == table.steps
    assert other.lr == table.lr and other.tv == 0.0 and np.array_equal(_bits(other.moment2), _bits(table.moment2))
    assert table.grids().shape == (2, 4, 8, 8, 12)


# ---------------------------------------------------------------------------- 8. trainer
SHAPE_T = (8, 6, 4)


def _run_trainer(dev, mk, cams, gts, fused, deferred, with_table=True, poses=None, masks=None, **cfg_kw):
    import brush_amd
    from brush_amd.bilagrid import BilagridTable

    s = mk()
    cfg = brush_amd.TrainConfig(**{**dict(warmup_steps=0, max_refine_step=0, deferred_sh_adam=deferred,
                                          bilagrid_shape=SHAPE_T), **cfg_kw})
    tr = brush_amd.SplatTrainer(s, cfg)
    tr.fused_backward = fused
    table = BilagridTable(4, dev, cfg.lr_bilagrid, cfg.bilagrid_shape, cfg.bilagrid_tv) if with_table else None
    losses = []
    for i in TE.ORDER:
        kw = dict(view_index=i, bilagrids=table) if with_table else {}
        if poses is not None:
            kw.update(view_index=i, poses=poses)
        if masks is not None:
            kw.update(gt_mask=masks[i])
        losses.append(float(tr.step(s, cams[i], gts[i], **kw)[0]))
    tr.sync(s)
    state = {k: getattr(s, k).detach().clone() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")}
    state["moment1"], state["moment2"] = tr.moment1.clone(), tr.moment2.clone()
    return losses, state, table


def test_trainer_with_zero_rate_is_the_trainer_without_the_option(dev, deterministic):
    import torch

    mk, cams, gts = TE._trainer_setup(dev)
    ident = np.tile(B.identity(SHAPE_T).astype(np.float32), (4, 1, 1, 1, 1))
    for fused, deferred in TE.PATHS:
        off = _run_trainer(dev, mk, cams, gts, fused, deferred, with_table=False)
        on = _run_trainer(dev, mk, cams, gts, fused, deferred, lr_bilagrid=0.0, bilagrid_tv=0.0)
        assert on[0] == off[0], (fused, deferred)
        for k in off[1]:
            assert torch.equal(on[1][k], off[1][k]), (fused, deferred, k)
        assert np.array_equal(_bits(on[2].params), ident.view(np.uint32))
        assert on[2].steps == [TE.ORDER.count(i) for i in range(4)]


def test_trainer_paths_hold_the_same_table_and_splats(dev, deterministic):
    mk, cams, gts = TE._trainer_setup(dev)
    runs = [_run_trainer(dev, mk, cams, gts, fused, deferred, lr_bilagrid=1e-2) for fused, deferred in TE.PATHS]
    for r in runs[1:]:
        assert r[0] == runs[0][0]
        for k in runs[0][1]:
            assert np.array_equal(_bits(r[1][k]), _bits(runs[0][1][k])), k
        for name in ("params", "moment1", "moment2"):
            assert np.array_equal(_bits(getattr(r[2], name)), _bits(getattr(runs[0][2], name))), name
    table = runs[0][2]
    ident = B.identity(SHAPE_T).astype(np.float32)
    G = _np(table.params)
    for i in range(3):  # drawn
        assert (G[i] != ident).any(), i
    assert np.array_equal(G[3].view(np.uint32), ident.view(np.uint32))  # never drawn: the identity's bits
    assert not _np(table.moment1)[3].any() and not _np(table.moment2)[3].any()
    off = _run_trainer(dev, mk, cams, gts, True, True, with_table=False)
    assert off[0] != runs[0][0]  # the table moved the trajectory


@pytest.mark.parametrize("mode", ["antialiased", "poses", "mcmc", "mask"])
def test_trainer_with_the_other_options(dev, mode):
    import torch

    from brush_amd.pose import PoseTable

    mk, cams, gts = TE._trainer_setup(dev)
    kw, poses, masks = {}, None, None
    if mode == "antialiased":
        kw = dict(antialiased=True)
    elif mode == "poses":
        poses = PoseTable(len(cams), 1e-3, 1e-2, 1e-4)
    elif mode == "mcmc":
        kw = dict(strategy="mcmc", mcmc_cap_max=4096)
    else:
        torch.manual_seed(3)
        masks = [(torch.rand(g.shape[:2], device=dev) < 0.7).to(torch.uint8) for g in gts]
    losses, _, table = _run_trainer(dev, mk, cams, gts, True, True, poses=poses, masks=masks, lr_bilagrid=1e-2, **kw)
    assert np.isfinite(losses).all()
    G = table.grids()
    assert np.isfinite(G).all() and (G[:3] != B.identity(SHAPE_T).astype(np.float32)).any()
    if poses is not None:
        poses.apply_all()
        assert bool(poses.delta.abs().sum() > 0)


def test_trainer_steps_with_bilagrids_do_not_synchronise(dev):
    import torch

    import brush_amd
    from brush_amd.bilagrid import BilagridTable

    mk, cams, gts = TE._trainer_setup(dev)
    for fused, deferred in TE.PATHS:
        s = mk()
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0,
                                                             deferred_sh_adam=deferred))
        tr.fused_backward = fused
        table = BilagridTable(4, dev, 2e-3, SHAPE_T)
        tr.step(s, cams[0], gts[0], view_index=0, bilagrids=table)  # the first step fills the deferred-SH table
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for i in TE.ORDER:
                tr.step(s, cams[i], gts[i], view_index=i, bilagrids=table)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert table.steps == [3, 3, 1, 0]


# ---------------------------------------------------------------------------- 9. end to end
def _view_effects(n, seed=37):
    """Per view: a vignette 1 - a r^2 about a centre near the middle (r = 1 at the far corner) and a gain
    1 + b (lum - 0.5) that depends on the pixel's own luminance."""
    rng = np.random.default_rng(seed)
    return dict(a=rng.uniform(0.3, 0.7, n), cx=rng.uniform(0.35, 0.65, n), cy=rng.uniform(0.35, 0.65, n),
                b=rng.uniform(-0.5, 0.5, n))


def _apply_effects(img64, fx, i):
    h, w = img64.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = x / (w - 1) - fx["cx"][i], y / (h - 1) - fx["cy"][i]
    r2 = (dx * dx + dy * dy) / ((0.65 ** 2) * 2)
    lum = img64[..., :3] @ np.asarray(B.LUMA)
    gain = (1.0 - fx["a"][i] * r2) * (1.0 + fx["b"][i] * (lum - 0.5))
    out = img64.copy()
    out[..., :3] *= gain[..., None]
    return out


def _write_scene(root, dev, effects, w=128, h=128, n_train=16, n_val=4):
    """The written-scene recipe of test_gpu_exposure with every training image passed through its view's vignette and
    luminance-dependent gain before it is quantised; the val images are clean."""
    import torch

    known = TE._known_cloud(dev)
    fovx = 0.6911112070083618
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, (c2w, cam) in enumerate(TL._ring_cameras(n, w, h, 4.0, 1.0, off)):
            with torch.no_grad():
                pred, _ = known.render(cam, (w, h), False)
            img64 = pred.cpu().numpy().astype(np.float64)
            if split == "train":
                img64 = _apply_effects(img64, effects, i)
            img = np.clip(np.round(img64[..., :3] * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(ED.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def vignetted_scene(tmp_path_factory, dev):
    return _write_scene(str(tmp_path_factory.mktemp("vignetted_scene")), dev, _view_effects(16))


E2E_STEPS = 2000


def test_train_scene_explains_vignettes_with_the_grids(dev, deterministic, vignetted_scene):
    """2000 random splats, E2E_STEPS steps at one seed in deterministic mode on images with per-view vignettes and
    luminance-dependent gains: without a colour model, with exposure_opt, with bilagrid_opt.  The affine map can take
    a view's mean darkening, not its shape, so the grids must end below both in the mean of the last 100 losses.  The
    configuration is TrainConfig's defaults (16 x 16 x 8, rate 2e-3, tv 10).  The eval views are clean and one global
    gain stays shared between the scene and the colour model, so the eval PSNRs are printed, not asserted.
    Measured on the MI355X: last-100 loss -0.189860 off, -0.191657 with exposure_opt, -0.192061 with the grids; eval
    PSNR 31.25 / 20.70 / 29.32 dB (profiles/bilagrid_margins.json: e2e).  A rate of 1e-2 ends above the run without the
    option (-0.189311): Adam then moves every word of a vertex that sees some ten pixels by the rate per step."""
    from brush_amd import TrainConfig
    from brush_amd.train_loop import load_dataset, train_scene

    data, _ = load_dataset(vignetted_scene)
    assert len(data.train.views) == 16

    def run(**kw):
        cfg = TrainConfig(warmup_steps=50, refine_every=50, **kw)
        rows = []
        _, log = train_scene(data, cfg, steps=E2E_STEPS, init_count=2000, sh_degree=3, seed=5, eval_every=E2E_STEPS,
                             on_eval=lambda r, s: rows.append(r))
        return log, rows[-1].psnr

    log_off, psnr_off = run()
    log_exp, psnr_exp = run(exposure_opt=True)
    log_on, psnr_on = run(bilagrid_opt=True)
    assert log_off.bilagrid_opt is False and log_off.bilagrid_shape is None
    assert log_on.bilagrid_opt is True and tuple(log_on.bilagrid_shape) == DEFAULT
    js = log_on.to_json()
    assert js["bilagrid_opt"] is True and js["bilagrid_shape"] == [16, 16, 8] and js["exposure_opt"] is False
    tail = lambda log: float(np.mean(log.losses[-100:]))
    t_off, t_exp, t_on = tail(log_off), tail(log_exp), tail(log_on)
    print(f"bilagrid e2e: last-100 loss off {t_off:.6f} exposure {t_exp:.6f} bilagrid {t_on:.6f}; eval psnr off "
          f"{psnr_off:.3f} exposure {psnr_exp:.3f} bilagrid {psnr_on:.3f}")
    _record("e2e", dict(steps=E2E_STEPS, loss_off=t_off, loss_exposure=t_exp, loss_bilagrid=t_on, psnr_off=psnr_off,
                        psnr_exposure=psnr_exp, psnr_bilagrid=psnr_on))
    assert t_on < t_off and t_on < t_exp


# ---------------------------------------------------------------------------- 10. CLI
def test_cli_exports_the_grids(vignetted_scene, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for on in (True, False):
        out_json, out_npz = str(tmp_path / f"log{on}.json"), str(tmp_path / f"grids{on}.npz")
        flags = ["--bilagrid-opt", "--bilagrid-tv", "5"] if on else []
        r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", vignetted_scene, "--steps", "40" if on else "4",
                            "--init-count", "1000", "--bilagrid-shape", "8,6,4", "--export-bilagrids", out_npz,
                            "--json", out_json] + flags, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(out_json) as f:
            log = json.load(f)
        assert log["bilagrid_opt"] is on and log["bilagrid_shape"] == ([8, 6, 4] if on else None)
        z = np.load(out_npz)
        assert sorted(z.files) == ["grids", "names"]
        assert z["grids"].shape == (16, 4, 6, 8, 12) and z["grids"].dtype == np.float32
        assert z["names"].shape == (16,) and len(set(z["names"].tolist())) == 16
        ident = np.tile(B.identity((8, 6, 4)).astype(np.float32), (16, 1, 1, 1, 1))
        assert np.isfinite(z["grids"]).all() and np.array_equal(z["grids"], ident) is (not on)
