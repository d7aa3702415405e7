"""GPU checks of the antialiased mode (include/brush_hip.h: BRUSH_AUX_ANTIALIASED): the record's opacity is
sigmoid(raw) * comp, comp = sqrt(det(S) / det(S + 0.3 I)).

Anchors:
  * per splat, word 8 against float64 (tests/aa_ref64.py) within a forward-error bound derived from the expression,
    the other words bitwise equal to the plain render;
  * the image against the CPU oracle's render of a "twin" whose raw opacity is logit(word 8): the twin differs from
    the GPU render by about an ulp of opacity, and the check above pins that opacity to float64 separately;
  * the backward against the oracle's backward of the same twin plus the comp chain of aa_ref64 (the float64 VJP that
    tests/test_antialias_cpu.py checks against central differences).  No GPU central difference on purpose: where comp
    matters the alpha >= 1/255 cutoff makes the image discontinuous in the scales;
  * the purpose of the mode: rendered at a lower resolution, a scene keeps the coverage of its box-downsampled
    high-resolution render."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import aa_ref64 as A
from tests import eval_data as E
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0 = np.float32(0.2820947917738781)
PIX_TOL = 1e-4  # the forward gate's pixel tolerance on a colour channel (values in [0, 1])
MAX_FLIP_FRACTION = 1e-3  # at most 0.1 % of a scene's pixels may be flagged flip_risk by the oracle
GRADS = ("v_means", "v_xy", "v_scales", "v_quats", "v_sh", "v_opac")


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    return torch.device("cuda:0")


def _camera(w, h):
    import brush_amd

    c = H.reference_test_camera(w, h)
    return brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def _golden(name):
    d = H.load_case(name)
    h, w, _ = d["out_img"].shape
    return dict(means=d["means"], log_scales=d["scales"], quats=d["quats"], sh=d["coeffs"],
                raw_opac=d["opacities"]), w, h


def _scene(kind):
    """(cloud, w, h): the scenes of test_gpu_depth.py plus a cloud of sub-pixel splats."""
    if kind in ("tiny_case", "basic_case"):
        return _golden(kind)
    if kind == "ragged":
        return H.synthetic_cloud(20000, 2, seed=7, mean_mult=0.3), 203, 117
    if kind == "empty":
        c = H.synthetic_cloud(500, 1, seed=3)
        c["means"] = c["means"] * np.float32(1e-3) - np.float32([0.0, 0.0, 1e6])  # every splat behind the camera
        return c, 64, 48
    if kind == "c1":
        return H.synthetic_cloud(104_858, 3, seed=4, mean_mult=1.0), 400, 400
    if kind == "S1":
        return H.synthetic_cloud(1 << 20, 3, seed=4, mean_mult=1.0), 1920, 1080
    if kind == "subpixel":
        c = H.synthetic_cloud(30000, 1, seed=9, mean_mult=1.0)
        c["log_scales"] = (c["log_scales"] - np.float32(3.0)).astype(np.float32)
        return c, 320, 240
    raise ValueError(kind)


def _tensors(cloud, dev, grad=False):
    import torch

    t = {k: torch.as_tensor(np.ascontiguousarray(cloud[k]), device=dev) for k in
         ("means", "log_scales", "quats", "sh", "raw_opac")}
    if grad:
        for v in t.values():
            v.requires_grad_(True)
    t["xy"] = torch.zeros((cloud["means"].shape[0], 2), device=dev, requires_grad=grad)
    return t


def _args(t):
    return t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"]


def _render(dev, cloud, w, h, det, aa, grad=False, camera=None):
    """`camera` (here and below): a brush_amd.Camera in place of the reference test camera."""
    import brush_amd

    t = _tensors(cloud, dev, grad)
    img, aux = brush_amd.render_splats(camera or _camera(w, h), (w, h), *_args(t), deterministic=det, antialiased=aa)
    return t, img, aux


def _u(w, h, cloud, camera=None):
    from brush_amd.render import pack_uniforms, sh_degree_from_coeffs

    return pack_uniforms(camera or _camera(w, h), (w, h), sh_degree_from_coeffs(cloud["sh"].shape[1]),
                         cloud["means"].shape[0])


def _np(t):
    return t.detach().cpu().numpy()


def _visible(aux):
    V = aux.read_num_visible()
    gid = _np(aux.global_from_compact_gid[:V]).astype(np.int64)
    return V, gid, _np(aux.projected_splats[:V, 8])


def _twin(cloud, aux):
    """The cloud with raw' = logit(word 8) (float64, then f32) for every visible splat, mapped back to global ids."""
    V, gid, o = _visible(aux)
    tw = dict(cloud)
    raw = np.array(cloud["raw_opac"], np.float32, copy=True)
    o64 = o.astype(np.float64)
    with np.errstate(divide="ignore"):
        raw[gid] = (np.log(o64) - np.log1p(-o64)).astype(np.float32)
    tw["raw_opac"] = raw
    return tw


# ---------------------------------------------------------------------------- 1. per splat
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1", "S1", "empty", "subpixel"])
def test_word8_is_compensated_opacity_and_the_rest_unchanged(dev, kind):
    check_word8(dev, kind, *_scene(kind))


def check_word8(dev, kind, cloud, w, h, camera=None):
    """The body of test_word8_is_compensated_opacity_and_the_rest_unchanged; returns the worst err / bound."""
    import torch

    with torch.no_grad():
        _, _, a0 = _render(dev, cloud, w, h, False, False, camera=camera)
        _, _, a1 = _render(dev, cloud, w, h, False, True, camera=camera)
    assert a1.antialiased and not a0.antialiased
    V = a1.read_num_visible()
    assert V == a0.read_num_visible()
    assert bool(torch.equal(a0.global_from_compact_gid, a1.global_from_compact_gid))
    assert _np(a0.projected_splats[:V, :8]).tobytes() == _np(a1.projected_splats[:V, :8]).tobytes()
    if kind == "empty":
        assert V == 0
        return 0.0
    _, gid, o = _visible(a1)
    u = _u(w, h, cloud, camera)
    want, bound = A.word8_bound(u, cloud["means"][gid], cloud["log_scales"][gid], cloud["quats"][gid],
                                cloud["raw_opac"][gid])
    err = np.abs(o.astype(np.float64) - want)
    comp = want / A.sigmoid64(cloud["raw_opac"][gid])
    print(f"[{kind}] V={V} comp min {comp.min():.3g} median {np.median(comp):.3g}; max err {err.max():.3e}, "
          f"max err / bound {float((err / bound).max()):.3f}; "
          f"intersections {a0.read_num_intersections()} -> {a1.read_num_intersections()}")
    assert (err <= bound).all(), (kind, float(err.max()), int((err > bound).sum()))
    assert a1.read_num_intersections() <= a0.read_num_intersections()
    return float((err / bound).max())


# ---------------------------------------------------------------------------- 2. image against the oracle's twin
def _oracle_twin(aux, tw):
    from brush_amd.render import uniforms_to_numpy

    return O.render_forward(uniforms_to_numpy(aux), tw["means"], tw["log_scales"], tw["quats"], tw["sh"],
                            tw["raw_opac"])


def _check_against(kind, got, want, risk, tol):
    assert risk.mean() <= MAX_FLIP_FRACTION, (kind, int(risk.sum()))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[~risk]
    print(f"[{kind}] max|gpu - oracle twin| = {float(err.max()) if err.size else 0.0:.3e} "
          f"({int(risk.sum())} flip-risk px)")
    assert err.size == 0 or float(err.max()) <= tol, (kind, float(err.max()))
    return (float(err.max()) if err.size else 0.0) / tol


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1"])
def test_image_matches_oracle_twin(dev, kind, det):
    check_image_oracle_twin(dev, kind, det, *_scene(kind))


def check_image_oracle_twin(dev, kind, det, cloud, w, h, camera=None):
    """The body of test_image_matches_oracle_twin; returns the worst err / PIX_TOL."""
    import torch

    with torch.no_grad():
        _, img, aux = _render(dev, cloud, w, h, det, True, camera=camera)
    tw = _twin(cloud, aux)
    o_out, o_aux = _oracle_twin(aux, tw)
    assert int(o_aux["num_visible"][0]) == aux.read_num_visible()
    risk = o_aux["flip_risk"].astype(bool)
    return _check_against(kind, _np(img), o_out, np.repeat(risk[..., None], 4, axis=2), PIX_TOL)


@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1"])
def test_depth_matches_oracle_twin(dev, kind):
    """render_splats_depth in the mode: the colour as above, and D as the red channel of the depth-as-colour twin
    (test_gpu_depth.py) of the opacity twin."""
    import torch

    import brush_amd
    from brush_amd.render import uniforms_to_numpy

    cloud, w, h = _scene(kind)
    with torch.no_grad():
        t = _tensors(cloud, dev)
        img, depth, aux = brush_amd.render_splats_depth(_camera(w, h), (w, h), *_args(t), antialiased=True)
    assert aux.antialiased
    tw = _twin(cloud, aux)
    o_out, o_aux = _oracle_twin(aux, tw)
    risk = o_aux["flip_risk"].astype(bool)
    _check_against(kind, _np(img), o_out, np.repeat(risk[..., None], 4, axis=2), PIX_TOL)
    u = _u(w, h, cloud)
    vm = np.array(list(u.viewmat), np.float32)
    m = np.asarray(tw["means"], np.float32)
    z = ((vm[2] * m[:, 0] + vm[6] * m[:, 1]) + vm[10] * m[:, 2]) + vm[14]
    dtw = dict(tw)
    dtw["sh"] = np.repeat((((z - np.float32(0.5)) / C0).astype(np.float32))[:, None, None], 3, axis=2)
    d_out, d_aux = O.render_forward(uniforms_to_numpy(aux) | {"sh_degree": 0}, dtw["means"], dtw["log_scales"],
                                    dtw["quats"], dtw["sh"], dtw["raw_opac"])
    _, gid, _ = _visible(aux)
    zmax = float(np.abs(z[gid]).max()) if gid.size else 1.0
    _check_against(kind + " depth", _np(depth), d_out[..., 0], d_aux["flip_risk"].astype(bool),
                   PIX_TOL * max(zmax, 1.0))


@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1"])
def test_rgba8_matches_oracle_twin(dev, kind):
    """The display path in the mode: every packed byte is the truncation of clamp(c) * 255 (rasterize.hip) for some c
    within the forward gate's PIX_TOL of the oracle twin's colour, i.e. |byte + 1/2 - 255 c| <= 1/2 + 255 PIX_TOL."""
    import torch

    from brush_amd.render import render_rgba8

    cloud, w, h = _scene(kind)
    t = _tensors(cloud, dev)
    with torch.no_grad():
        out, aux = render_rgba8(_camera(w, h), (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                t["raw_opac"], antialiased=True)
    assert aux.antialiased
    got = _np(out).reshape(h, -1).view(np.uint8).reshape(h, -1, 4)[:, :w].astype(np.float64) + 0.5
    tw = _twin(cloud, aux)
    o_out, o_aux = _oracle_twin(aux, tw)
    risk = np.repeat(o_aux["flip_risk"].astype(bool)[..., None], 4, axis=2)
    want = np.clip(o_out.astype(np.float64), 0.0, 1.0) * 255.0
    _check_against(kind + " rgba8", got, want, risk, 0.5 + 255.0 * PIX_TOL + 1e-9)


# ---------------------------------------------------------------------------- 3. the purpose: zooming out
def test_zoom_out_keeps_coverage(dev):
    """synthetic_cloud(104858, 1, seed=4) at 640^2 and at 640/k: the low-resolution mean alpha within 10 % of the
    box-downsampled high-resolution mean alpha, and the mean |d alpha| at most half of the plain mode's.  The plain
    mode fails both (ISSUE table: 0.626 against 0.195 at k = 4)."""
    import torch

    cloud = H.synthetic_cloud(104858, 1, seed=4, mean_mult=1.0)
    res = {}
    with torch.no_grad():
        for aa in (False, True):
            _, hi, _ = _render(dev, cloud, 640, 640, False, aa)
            a_hi = hi[..., 3].double()
            for k in (2, 4):
                s = 640 // k
                _, lo, _ = _render(dev, cloud, s, s, False, aa)
                a_lo = lo[..., 3].double()
                box = a_hi.reshape(s, k, s, k).mean(dim=(1, 3))
                res[(aa, k)] = (float(a_lo.mean()), float(box.mean()), float((a_lo - box).abs().mean()))
    for (aa, k), (lo, box, d) in sorted(res.items()):
        print(f"{'antialiased' if aa else 'plain'} k={k}: mean alpha low {lo:.4f} / box {box:.4f} "
              f"({abs(lo / box - 1) * 100:.1f} %), mean |d alpha| {d:.4f}")
    for k in (2, 4):
        lo, box, d = res[(True, k)]
        assert abs(lo / box - 1.0) <= 0.10, (k, lo, box)
        assert d <= 0.5 * res[(False, k)][2], (k, d, res[(False, k)][2])
    lo, box, _ = res[(False, 4)]
    assert abs(lo / box - 1.0) > 0.10  # the defect the mode exists for


# ---------------------------------------------------------------------------- 4. backward against the oracle
def _upstream(dev, w, h, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand((h, w, 4), generator=g) - 0.5).to(dev)


def _grads(dev, cloud, w, h, det, v_out, camera=None):
    import torch

    t, img, aux = _render(dev, cloud, w, h, det, True, grad=True, camera=camera)
    ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"]]
    g = torch.autograd.grad([img], ps, [v_out])
    return dict(zip(GRADS, (_np(x) for x in g))), img, aux


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged"])
def test_backward_against_oracle_twin(dev, kind, det):
    """Expected: the oracle's backward of the twin, plus dL/do * sigmoid * d comp / d theta (aa_ref64), with
    dL/do = v_raw' / (o (1 - o)); for the opacity v_raw = dL/do * comp * sigmoid (1 - sigmoid).  Tolerances of the
    golden gate (test_gpu_depth.py: test_backward_against_oracle)."""
    check_backward_oracle_twin(dev, kind, det, *_scene(kind))


def check_backward_oracle_twin(dev, kind, det, cloud, w, h, camera=None):
    """The body of test_backward_against_oracle_twin; returns the worst err/tol per gradient."""
    from brush_amd.render import uniforms_to_numpy

    v_out = _upstream(dev, w, h, seed=6)
    got, img, aux = _grads(dev, cloud, w, h, det, v_out, camera=camera)
    tw = _twin(cloud, aux)
    ud = uniforms_to_numpy(aux)
    o_img, o_aux = O.render_forward(ud, tw["means"], tw["log_scales"], tw["quats"], tw["sh"], tw["raw_opac"])
    base = O.render_backward(ud, o_aux, tw["means"], tw["log_scales"], tw["quats"], tw["raw_opac"], o_img, _np(v_out))
    want = {k: np.asarray(base[k], np.float64).copy() for k in GRADS}
    _, gid, _ = _visible(aux)
    ot = A.sigmoid64(tw["raw_opac"][gid])
    dd = ot * (1.0 - ot)
    dldo = np.where(dd > 0, want["v_opac"][gid] / np.where(dd > 0, dd, 1.0), 0.0)
    u = _u(w, h, cloud, camera)
    sig = A.sigmoid64(cloud["raw_opac"][gid])
    comp = A.comp64(u, cloud["means"][gid], cloud["log_scales"][gid], cloud["quats"][gid])
    vm, vs, vq = A.comp_vjp64(u, cloud["means"][gid], cloud["log_scales"][gid], cloud["quats"][gid], dldo * sig)
    want["v_means"][gid] += vm
    want["v_scales"][gid] += vs
    want["v_quats"][gid] += vq
    want["v_opac"][gid] = dldo * comp * sig * (1.0 - sig)
    print(f"[{kind} det={det}] V={gid.size} comp min {comp.min() if gid.size else 1:.3g}")
    ratios = {}
    for k in GRADS:
        scale = float(np.abs(want[k]).max())
        rtol = 1e-1 if k == "v_quats" else 1e-3  # the golden gate's own v_quats tolerance
        ok, err, bad = H.all_close_report(got[k], want[k], rtol, 1e-4 * scale + 1e-12)
        print(f"  {k}: max_abs_err {err:.3e} scale {scale:.3e}")
        ratios[k] = float((np.abs(got[k] - want[k]) / (1e-4 * scale + 1e-12 + rtol * np.abs(want[k]))).max())
        assert ok, f"{kind} det={det} {k}: max_abs_err={err} bad={bad} scale={scale}"
    return ratios


def test_deterministic_backward_bitwise(dev):
    cloud, w, h = _scene("c1")
    v_out = _upstream(dev, w, h, seed=7)
    a, _, _ = _grads(dev, cloud, w, h, True, v_out)
    b, _, _ = _grads(dev, cloud, w, h, True, v_out)
    for k in GRADS:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------- 5. modes and paths
def test_trainer_paths_give_the_same_bits(dev):
    """test_gpu_train.py's fused / separate optimizer check in the mode: three deterministic steps leave the same bits
    on the fused eager, fused deferred-SH and separate-call paths."""
    import torch

    import brush_amd
    from brush_amd import render as R

    cloud = H.synthetic_cloud(4096, 3, seed=13, mean_mult=0.0005)
    cloud["log_scales"] = cloud["log_scales"] - 3.0
    w, h = 128, 80
    cam = _camera(w, h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda: brush_amd.Splats(t(cloud["means"]), t(cloud["sh"]), t(cloud["quats"] * 1.7), t(cloud["raw_opac"]),
                                  t(cloud["log_scales"]))
    torch.manual_seed(5)
    gt = torch.rand((h, w, 3), device=dev)
    runs = []
    saved, R.DETERMINISTIC = R.DETERMINISTIC, True
    try:
        for fused, deferred in ((True, False), (True, True), (False, False)):
            s = mk()
            tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0,
                                                                 deferred_sh_adam=deferred, antialiased=True))
            tr.fused_backward = fused
            losses = []
            for _ in range(3):
                loss, _, aux = tr.step(s, cam, gt)
                assert aux.antialiased
                losses.append(float(loss))
            assert (tr._lazy is not None) == (fused and deferred)
            tr.sync(s)
            runs.append((losses, {k: _np(getattr(s, k)).tobytes() for k in
                                  ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")},
                         _np(tr.moment1).tobytes(), _np(tr.moment2).tobytes()))
    finally:
        R.DETERMINISTIC = saved
    for r in runs[1:]:
        assert r == runs[0]
    # and the mode is in use: the plain mode takes another trajectory
    s = mk()
    tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0))
    plain = [float(tr.step(s, cam, gt)[0]) for _ in range(3)]
    assert plain != runs[0][0]


def test_graph_capture_and_no_host_sync(dev):
    import torch

    import brush_amd

    cloud, w, h = _scene("ragged")
    t = _tensors(cloud, dev, grad=True)
    cam = _camera(w, h)
    v_out = _upstream(dev, w, h, seed=8)
    ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"]]

    def step():
        img, _ = brush_amd.render_splats(cam, (w, h), *_args(t), deterministic=True, antialiased=True)
        gr = torch.autograd.grad([img], ps, [v_out])
        return [img.detach()] + list(gr)

    eager = [x.clone() for x in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the capture stream
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(s):
            step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        outs = step()
    for o in outs:
        o.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert _np(a).tobytes() == _np(b).tobytes()


def test_records_path_refuses_the_mode(dev):
    import ctypes as C

    import torch

    from brush_amd import _lib
    from brush_amd import render as R

    cloud, w, h = _scene("basic_case")
    t = _tensors(cloud, dev)
    n = cloud["means"].shape[0]
    l = _lib.lib()
    out, aux, u = R._forward_impl(_camera(w, h), (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                  t["raw_opac"], False, None, deterministic=False, expect_backward=False,
                                  antialiased=True)
    nb = C.c_size_t()
    # the workspace is sized by the bits that size it; the antialiased bit is not one of them and is refused there
    assert l.brush_bwd_workspace_size_flags(n, w, h, int(u.sh_degree), int(aux.max_intersects), int(aux.flags),
                                            C.byref(nb)) == -1
    _lib.check(l.brush_bwd_workspace_size_flags(n, w, h, int(u.sh_degree), int(aux.max_intersects),
                                                aux.workspace_flags, C.byref(nb)), "brush_bwd_workspace_size_flags")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    v_out = torch.zeros_like(out)
    records = torch.empty((n, 16), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(flags):
        s = aux._as_struct()
        s.flags = flags
        s.bwd_accum = None
        return l.brush_render_backward_records(C.byref(u), C.byref(s), t["means"].data_ptr(), t["log_scales"].data_ptr(),
                                               t["quats"].data_ptr(), t["raw_opac"].data_ptr(), n, out.data_ptr(),
                                               v_out.data_ptr(), records.data_ptr(), n, ws.data_ptr(), nb.value,
                                               stream)

    assert call(_lib.AUX_ANTIALIASED) == -1  # BRUSH_ERR_INVALID_ARG
    assert call(0) == 0  # the same call without the bit runs
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 6. end to end
def _write_scene(root, dev, w=128, h=128, n_train=16, n_val=4):
    """test_gpu_train_loop.py's NeRF-synthetic scene (renders of a known 3000-splat cloud), rendered in the mode."""
    import torch

    from brush_amd import Splats
    from tests.test_gpu_train_loop import _ring_cameras

    rng = np.random.default_rng(11)
    known = Splats.from_random_config(3000, 0, (np.full(3, -0.8), np.full(3, 0.8)), rng, dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.06))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    fovx = 0.6911112070083618
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, (c2w, cam) in enumerate(_ring_cameras(n, w, h, 4.0, 1.0, off)):
            with torch.no_grad():
                pred, _ = known.render(cam, (w, h), False, antialiased=True)
            img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(E.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def aa_scene_dir(tmp_path_factory, dev):
    return _write_scene(str(tmp_path_factory.mktemp("aa_scene")), dev)


def test_train_and_evaluate_in_the_mode(dev, aa_scene_dir):
    """600 steps trained and evaluated in the mode gain more than 6 dB: test_gpu_train_loop.py's own threshold."""
    from brush_amd import TrainConfig
    from brush_amd.train_loop import load_dataset, train_scene

    data, _ = load_dataset(aa_scene_dir)
    rows = []
    splats, log = train_scene(data, TrainConfig(warmup_steps=50, refine_every=50, antialiased=True), steps=600,
                              init_count=2000, sh_degree=3, seed=5, eval_every=200, on_eval=lambda r, s: rows.append(r))
    print("antialiased e2e psnr by step:", [(r.step, round(r.psnr, 3), r.splats) for r in rows])
    assert [r.step for r in rows] == [0, 200, 400, 600]
    assert rows[-1].psnr > rows[0].psnr + 6.0
    assert np.isfinite(log.losses).all()


def test_clis_run_in_the_mode(aa_scene_dir, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out_ply, out_json = str(tmp_path / "out.ply"), str(tmp_path / "log.json")
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", aa_scene_dir, "--steps", "60", "--eval-every",
                        "30", "--eval-views", "2", "--init-count", "1000", "--export", out_ply, "--json", out_json,
                        "--antialiased"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_json) as f:
        log = json.load(f)
    assert log["antialiased"] is True and len(log["losses"]) == 60
    ev_json = str(tmp_path / "eval.json")
    runs = {}
    for tag, extra in (("plain", []), ("aa", ["--antialiased"])):
        r = subprocess.run([sys.executable, "-m", "brush_amd.eval", out_ply, aa_scene_dir, "--json", ev_json] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(ev_json) as f:
            runs[tag] = json.load(f)
    assert runs["aa"]["antialiased"] is True and runs["plain"]["antialiased"] is False
    assert runs["aa"]["mean_psnr"] != runs["plain"]["mean_psnr"]
