"""GPU checks of the accumulated depth output (brush_render_forward_depth / brush_render_backward_depth,
render_splats_depth, Splats.render_depth, `python -m brush_amd.eval --depth-dir`).

The anchor is linearity: D = sum T alpha z is the red channel of a "depth-as-colour" twin of the scene (SH degree 0,
DC chosen so that C0 dc + 0.5 = z_i, every other parameter equal), which the existing forward, backward and CPU oracle
already cover.  The geometry, alphas and order of the twin are the scene's; only the rounding of the SH colour
differs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import eval_data as E
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0 = np.float32(0.2820947917738781)
PIX_TOL = 1e-4  # the forward gate's pixel tolerance on a colour channel (values in [0, 1])
EPS32 = 2.0 ** -24
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
    """(cloud, w, h): the golden cases, a ragged frame, an empty view and the c1- / S1-sized synthetic clouds."""
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


def _view_z(u, means):
    """Camera-space z of every mean, in f32 with the projection's own association (splat_math.hpp: to_view)."""
    vm = np.array(list(u.viewmat), np.float32)
    m = np.asarray(means, np.float32)
    return ((vm[2] * m[:, 0] + vm[6] * m[:, 1]) + vm[10] * m[:, 2]) + vm[14]


def _twin(cloud, u):
    """Depth-as-colour twin: SH degree 0 with C0 dc + 0.5 = z (r = g = b)."""
    z = _view_z(u, cloud["means"])
    dc = ((z - np.float32(0.5)) / C0).astype(np.float32)
    tw = dict(cloud)
    tw["sh"] = np.repeat(dc[:, None, None], 3, axis=2).astype(np.float32)
    return tw, z


def _render_depth(dev, cloud, w, h, det, grad=False, camera=None, max_intersects=None):
    """`camera` (here and below): a brush_amd.Camera in place of the reference test camera; `max_intersects`: an
    intersection capacity in place of the default."""
    import brush_amd

    t = _tensors(cloud, dev, grad)
    img, depth, aux = brush_amd.render_splats_depth(camera or _camera(w, h), (w, h), *_args(t),
                                                    max_intersects=max_intersects, deterministic=det)
    return t, img, depth, aux


def _render(dev, cloud, w, h, det, grad=False, camera=None, max_intersects=None):
    import brush_amd

    t = _tensors(cloud, dev, grad)
    img, aux = brush_amd.render_splats(camera or _camera(w, h), (w, h), *_args(t), max_intersects=max_intersects,
                                       deterministic=det)
    return t, img, aux


def _u(aux, w, h, cloud, camera=None):
    from brush_amd.render import pack_uniforms, sh_degree_from_coeffs

    return pack_uniforms(camera or _camera(w, h), (w, h), sh_degree_from_coeffs(cloud["sh"].shape[1]),
                         cloud["means"].shape[0])


def _z_row(u, column=False):
    """d z_view / d mean: row 2 of the world-to-camera rotation W (viewmat is column-major), float64 [3].  `column`:
    column 2 instead, the mistake that cannot be told from row 2 where W is symmetric (the negative controls of
    tests/test_gpu_general_camera.py)."""
    vm = np.array(list(u.viewmat), np.float64)
    return vm[[8, 9, 10]] if column else vm[[2, 6, 10]]


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------- 1. forward against the twin / oracle
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "empty", "c1", "S1"])
def test_forward_matches_depth_as_colour_twin(dev, kind):
    check_forward_twin(dev, kind, *_scene(kind))


def check_forward_twin(dev, kind, cloud, w, h, camera=None, max_risk=None, max_intersects=None, det=False):
    """The body of test_forward_matches_depth_as_colour_twin; returns (V, worst err/tol against the GPU twin, worst
    err/tol against the oracle's twin).  `max_risk`: the largest share of flip-risk pixels the caller accepts."""
    import torch

    from brush_amd.render import uniforms_to_numpy

    with torch.no_grad():
        _, img, depth, aux = _render_depth(dev, cloud, w, h, det, camera=camera, max_intersects=max_intersects)
        u = _u(aux, w, h, cloud, camera)
        tw, z = _twin(cloud, u)
        _, timg, taux = _render(dev, tw, w, h, det, camera=camera, max_intersects=max_intersects)
    D, R = _np(depth).astype(np.float64), _np(timg)[..., 0].astype(np.float64)
    assert depth.shape == (h, w) and depth.dtype == torch.float32
    V = aux.read_num_visible()
    assert V == taux.read_num_visible()
    assert bool(torch.equal(aux.final_index, taux.final_index))
    assert bool(torch.equal(img[..., 3], timg[..., 3]))  # same alphas, same order
    vis = _np(aux.global_from_compact_gid[:V]).astype(np.int64)
    zmax = float(np.abs(z[vis]).max()) if V else 1.0
    if kind == "empty":
        assert V == 0 and not D.any()
    # GPU twin: the same sums with the SH rounding of the colour (|C0 dc + 0.5 - z| of a few ulp of z per term)
    err = np.abs(D - R)
    tol = 64 * EPS32 * (np.maximum(np.abs(R), zmax * _np(img)[..., 3]) + 1.0)
    assert (err <= tol + 1e-30).all(), (kind, float(err.max()), int((err > tol).sum()))
    # the CPU oracle's twin, within the forward gate's colour margin scaled by the depth range
    o_out, o_aux = O.render_forward(uniforms_to_numpy(taux), tw["means"], tw["log_scales"], tw["quats"], tw["sh"],
                                    tw["raw_opac"], max_intersects=max_intersects)
    assert int(o_aux["num_visible"][0]) == V
    risk = o_aux["flip_risk"].astype(bool)
    assert max_risk is None or risk.mean() <= max_risk, (kind, int(risk.sum()))
    oerr = np.abs(D - o_out[..., 0])[~risk]
    print(f"[{kind}] V={V} max|D - twin|={float(err.max()):.3e} max|D - oracle|="
          f"{float(oerr.max()) if oerr.size else 0.0:.3e} (zmax {zmax:.3g}, {int(risk.sum())} flip-risk px)")
    assert oerr.size == 0 or float(oerr.max()) <= PIX_TOL * max(zmax, 1.0), (kind, float(oerr.max()))
    return V, float((err / (tol + 1e-30)).max()), (float(oerr.max()) if oerr.size else 0.0) / (PIX_TOL * max(zmax, 1.0))


# ---------------------------------------------------------------------------- 2. image unchanged
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["basic_case", "ragged", "c1"])
def test_image_and_aux_bitwise_equal(dev, kind, det):
    import torch

    cloud, w, h = _scene(kind)
    with torch.no_grad():
        _, img, _, aux = _render_depth(dev, cloud, w, h, det)
        _, img0, aux0 = _render(dev, cloud, w, h, det)
    assert _np(img).tobytes() == _np(img0).tobytes()
    for name in ("final_index", "tile_bins", "num_visible", "num_intersections", "projected_splats",
                 "global_from_compact_gid", "cum_tiles_hit"):
        a, b = getattr(aux, name), getattr(aux0, name)
        if name == "projected_splats":
            V = aux.read_num_visible()
            a, b = a[:V], b[:V]
        assert bool(torch.equal(a, b)), name
    I = aux.read_num_intersections()
    assert bool(torch.equal(aux.compact_gid_from_isect[:I], aux0.compact_gid_from_isect[:I]))


# ---------------------------------------------------------------------------- 3. backward by linearity
def _grads(dev, cloud, w, h, det, v_out, v_d=None, camera=None, max_intersects=None):
    """Gradients of <img, v_out> (+ <depth, v_d>) into the six parents: the depth op when v_d is given, else
    render_splats."""
    import torch

    if v_d is None:
        t, img, aux = _render(dev, cloud, w, h, det, grad=True, camera=camera, max_intersects=max_intersects)
        outs, gos = [img], [v_out]
    else:
        t, img, depth, aux = _render_depth(dev, cloud, w, h, det, grad=True, camera=camera,
                                           max_intersects=max_intersects)
        outs, gos = [img, depth], [v_out, v_d]
    ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"]]
    g = torch.autograd.grad(outs, ps, gos)
    return dict(zip(GRADS, (_np(x) for x in g))), img, aux


def _linear_parts(dev, cloud, w, h, det, v_out, v_d, camera=None, column=False, max_intersects=None, control=None):
    """existing backward(v_out) + twin backward with v_out = (v_D, 0, 0, 0), v_z = v_sh_dc_r / C0 into v_means.
    `column`: the mistaken depth term of _z_row, for the negative controls; `control`: another mistaken reference,
    "rotate_quadrants" or "no_depth_in_alpha" (arbiter_gate)."""
    import torch

    base, _, aux = _grads(dev, cloud, w, h, det, v_out, camera=camera, max_intersects=max_intersects)
    u = _u(aux, w, h, cloud, camera)
    tw, _ = _twin(cloud, u)
    vt = torch.zeros_like(v_out)
    vt[..., 0] = v_d
    if control == "rotate_quadrants":
        vt[..., 0] = torch.as_tensor(_quadrants_rotated(_np(v_d)), device=v_d.device)
    elif control not in (None, "no_depth_in_alpha"):
        raise ValueError(control)
    twin, _, _ = _grads(dev, tw, w, h, det, vt, camera=camera, max_intersects=max_intersects)
    row = _z_row(u, column)
    v_z = twin["v_sh"][:, 0, 0].astype(np.float64) / float(C0)
    omit = control == "no_depth_in_alpha"
    want = {k: base[k].astype(np.float64) + (0.0 if k == "v_sh" or omit else twin[k]) for k in GRADS}
    want["v_means"] = want["v_means"] + v_z[:, None] * row[None, :]
    mags = {k: np.abs(base[k]) + (0.0 if k == "v_sh" else np.abs(twin[k])) for k in GRADS}
    mags["v_means"] = mags["v_means"] + np.abs(v_z[:, None] * row[None, :])
    return want, mags, base, u, tw


def _upstream(dev, w, h, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    v_out = (torch.rand((h, w, 4), generator=g) - 0.5).to(dev)
    v_d = ((torch.rand((h, w), generator=g) - 0.5) * 1e-2).to(dev)
    return v_out, v_d


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1"])
def test_backward_is_sum_of_colour_and_twin_parts(dev, kind, det):
    check_backward_linearity(dev, kind, det, *_scene(kind))


def _gate_ratio(got, want, rtol, atol):
    """Worst |got - want| / (atol + rtol |want|) of H.all_close_report's gate."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max()) if got.size else 0.0


def check_backward_linearity(dev, kind, det, cloud, w, h, camera=None, column=False, max_intersects=None,
                             control=None):
    """The body of test_backward_is_sum_of_colour_and_twin_parts; returns the worst err/tol per gradient."""
    v_out, v_d = _upstream(dev, w, h, seed=5)
    got, _, _ = _grads(dev, cloud, w, h, det, v_out, v_d, camera=camera, max_intersects=max_intersects)
    want, mags, _, _, _ = _linear_parts(dev, cloud, w, h, det, v_out, v_d, camera=camera, column=column,
                                        max_intersects=max_intersects, control=control)
    ratios = {}
    for k in GRADS:
        scale = float(mags[k].max()) if mags[k].size else 0.0
        ok, err, bad = H.all_close_report(got[k], want[k], 1e-3, 1e-4 * scale + 1e-12)
        ratios[k] = _gate_ratio(got[k], want[k], 1e-3, 1e-4 * scale + 1e-12)
        assert ok, f"{kind} det={det} {k}: max_abs_err={err} bad={bad} scale={scale}"
    return ratios


@pytest.mark.parametrize("kind", ["tiny_case", "basic_case"])
def test_backward_against_oracle(dev, kind):
    """The depth backward against the oracle's backward of the image plus that of the twin (f64 sums)."""
    check_backward_oracle(dev, kind, *_scene(kind))


def check_backward_oracle(dev, kind, cloud, w, h, camera=None, column=False):
    """The body of test_backward_against_oracle; returns the worst err/tol per gradient."""
    from brush_amd.render import uniforms_to_numpy

    v_out, v_d = _upstream(dev, w, h, seed=6)
    got, img, aux = _grads(dev, cloud, w, h, False, v_out, v_d, camera=camera)
    ud = uniforms_to_numpy(aux)
    u = _u(aux, w, h, cloud, camera)
    tw, _ = _twin(cloud, u)
    o_img, o_aux = O.render_forward(ud, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                    cloud["raw_opac"])
    base = O.render_backward(ud, o_aux, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["raw_opac"],
                             o_img, _np(v_out))
    t_img, t_aux = O.render_forward(ud | {"sh_degree": 0}, tw["means"], tw["log_scales"], tw["quats"], tw["sh"],
                                    tw["raw_opac"])
    vt = np.zeros((h, w, 4), np.float32)
    vt[..., 0] = _np(v_d)
    twin = O.render_backward(ud | {"sh_degree": 0}, t_aux, tw["means"], tw["log_scales"], tw["quats"],
                             tw["raw_opac"], t_img, vt)
    v_z = twin["v_sh"][:, 0, 0].astype(np.float64) / float(C0)
    ratios = {}
    for k in GRADS:
        want = base[k].astype(np.float64) + (0.0 if k == "v_sh" else twin[k])
        if k == "v_means":
            want = want + v_z[:, None] * _z_row(u, column)[None, :]
        scale = float(np.abs(want).max())
        rtol = 1e-1 if k == "v_quats" else 1e-3  # the golden gate's own v_quats tolerance
        ok, err, bad = H.all_close_report(got[k], want, rtol, 1e-4 * scale + 1e-12)
        ratios[k] = _gate_ratio(got[k], want, rtol, 1e-4 * scale + 1e-12)
        assert ok, f"{kind} {k}: max_abs_err={err} bad={bad} scale={scale}"
    return ratios


# ---------------------------------------------------------------------------- 3b. backward against the f64 arbiter
# The depth gradient element by element, under the allowance the colour gradient is held to (test_gpu_render.
# _assert_grad_parity: every term tied to a mechanism, none a fraction of a tensor's maximum).  By linearity the exact
# value is arbiter(cloud, v_out) + arbiter(twin at SH degree 0, (v_D, 0, 0, 0)), the twin's v_sh left out and
# v_z = twin v_sh[:, 0, 0] / C0 sent into v_means along row 2 of W; the kernel adds the two parts' terms in one f32
# accumulator, so its allowance is the sum of the two calls' allowances, the v_z part priced like the value it is made
# from.  One term is new: the twin's f32 colour fl(fl(C0 dc) + 0.5), dc = fl((z - 0.5) / C0), is z only to four
# roundings, 4 eps32 (|z| + 0.5) per depth term, where the kernel works from z itself: 4 eps32 of the twin's mag_*.
TWIN_COLOUR_ROUNDINGS = 4.0
ARBITER_GRADS = ("v_means", "v_scales", "v_quats", "v_sh", "v_opac", "v_xy")


def _np_u32(t):
    return t.detach().cpu().numpy().astype(np.int32).view(np.uint32)


def _quadrants_rotated(v_d):
    """v_D with the four 8 x 8 quadrants of every 16 x 16 tile moved on by one (0 -> 1 -> 2 -> 3 -> 0, quadrant
    q = (x / 8 & 1) + 2 (y / 8 & 1)): what a quadrant mix-up in the multi-quadrant forms would consume.  Zero-padded to
    whole tiles first."""
    h, w = v_d.shape
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    p = np.zeros((hp, wp), v_d.dtype)
    p[:h, :w] = v_d
    q = p.reshape(hp // 16, 2, 8, wp // 16, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(hp // 16, wp // 16, 4, 8, 8)
    q = np.roll(q, 1, axis=2)
    p = q.reshape(hp // 16, wp // 16, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(hp, wp)
    return np.ascontiguousarray(p[:h, :w])


def arbiter_state(dev, kind, det, cloud, w, h, camera=None, max_intersects=None, zero_v_out=False):
    """One depth backward on the GPU and the two arbiter calls on the forward state it consumed: the oracle's aux of
    the cloud (of the twin) with final_index replaced by the GPU's, and the GPU's own images.  Returns a dict with the
    GPU's gradients (`got`), the float64 arbiter's and the f32-sum oracle's results of both calls, and what a control
    needs to build another reference.  `zero_v_out`: v_out = 0, the depth gradient alone; every term of the colour
    call then carries a factor 0, so its results and allowance are zeros and the call is not made."""
    import torch

    from brush_amd.render import uniforms_to_numpy
    from tests import binning_check as BK

    v_out, v_d = _upstream(dev, w, h, seed=5)
    if zero_v_out:
        v_out = torch.zeros_like(v_out)
    got, img, aux = _grads(dev, cloud, w, h, det, v_out, v_d, camera=camera, max_intersects=max_intersects)
    ud = uniforms_to_numpy(aux)
    u = _u(aux, w, h, cloud, camera)
    tw, _ = _twin(cloud, u)
    with torch.no_grad():
        _, timg, taux = _render(dev, tw, w, h, det, camera=camera, max_intersects=max_intersects)
    # one forward state: the twin composites the same entries with the same alphas
    assert bool(torch.equal(aux.final_index, taux.final_index)), kind
    assert bool(torch.equal(img[..., 3], timg[..., 3])), kind
    fin = _np_u32(aux.final_index)
    ut = ud | {"sh_degree": 0}
    o_img, o_aux = O.render_forward(ud, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                    cloud["raw_opac"], max_intersects=aux.max_intersects)
    BK.assert_integer_parity(BK.aux_arrays(aux, ud["num_visible"]), o_aux)  # the lists the arbiter walks are the GPU's
    _, t_aux = O.render_forward(ut, tw["means"], tw["log_scales"], tw["quats"], tw["sh"], tw["raw_opac"],
                                max_intersects=aux.max_intersects)
    shared, t_shared = dict(o_aux, final_index=fin), dict(t_aux, final_index=fin)
    g_img, g_timg = _np(img), _np(timg)
    vo = _np(v_out)
    vt = np.zeros((h, w, 4), np.float32)
    vt[..., 0] = _np(v_d)
    geo = (cloud["means"], cloud["log_scales"], cloud["quats"], cloud["raw_opac"])
    st = dict(kind=kind, det=det, got=got, u=u, ut=ut, t_shared=t_shared, g_timg=g_timg, geo=geo, v_d=_np(v_d),
              V=int(o_aux["num_visible"][0]), gids=o_aux["global_from_compact_gid"][:int(o_aux["num_visible"][0])],
              twin64=O.render_backward_f64(ut, t_shared, *geo, g_timg, vt),
              twin32=O.render_backward(ut, t_shared, *geo, g_timg, vt, f32_sums=True))
    if zero_v_out:
        zeros = {k: np.zeros(cloud["sh"].shape if k.endswith("sh") else v.shape) for k, v in st["twin64"].items()}
        st.update(base64=zeros, base32={k: zeros[k] for k in ARBITER_GRADS})
    else:
        st.update(base64=O.render_backward_f64(ud, shared, *geo, g_img, vo),
                  base32=O.render_backward(ud, shared, *geo, g_img, vo, f32_sums=True))
    return st


def _call_allowance(f64, f32, name):
    """The allowance test_gpu_render._grad_ratio grants one arbiter call on tensor `name`, per element: its constants
    and RTOL by import, the C_REF row term from the f32-sum oracle `f32` of the same call."""
    from tests import test_gpu_render as TR

    t = f64[name]
    row_ref = TR._rowmax(np.abs(f32[name].astype(np.float64).reshape(t.shape) - t), t.shape)
    _, _, parts = TR._grad_ratio(t, f64, row_ref, name, TR.CANDIDATES[TR.ACTIVE])
    tol = np.zeros(t.shape)
    for p in parts:
        tol = tol + p
    return tol


def arbiter_gate(st, control=None):
    """Asserts the GPU gradients of `st` (arbiter_state) within the allowance of the expected value, element by element;
    returns, per tensor, dict(worst err/tol, worst_noflip: the same over the elements without a flip allowance).  `control` swaps in a WRONG expected value, the allowance unchanged, for the
    negative controls: "column" (v_z along column 2 of W), "rotate_quadrants" (the twin backward fed v_D with every
    tile's quadrants moved on by one), "no_depth_in_alpha" (the depth channel left out of the colour term of v_alpha:
    of the twin only v_z survives, its v_opac / v_xy / conic parts and what they become are omitted)."""
    base64, twin64 = st["base64"], st["twin64"]
    src = twin64
    if control == "rotate_quadrants":
        vt = np.zeros(st["g_timg"].shape, np.float32)
        vt[..., 0] = _quadrants_rotated(st["v_d"])
        src = O.render_backward_f64(st["ut"], st["t_shared"], *st["geo"], st["g_timg"], vt)
    elif control not in (None, "column", "no_depth_in_alpha"):
        raise ValueError(control)
    row = _z_row(st["u"], column=control == "column")
    c0 = float(C0)
    ratios, noflip = {}, {}
    for k in ARBITER_GRADS:
        mag, flip = "mag_" + k[2:], "flip_" + k[2:]
        want, tol, flips = base64[k], _call_allowance(base64, st["base32"], k), base64[flip] != 0
        if k != "v_sh":
            if control != "no_depth_in_alpha":
                want = want + src[k]
            tol = tol + _call_allowance(twin64, st["twin32"], k) + TWIN_COLOUR_ROUNDINGS * EPS32 * twin64[mag]
            flips = flips | (twin64[flip] != 0)
        if k == "v_means":
            flips = flips | (twin64["flip_sh"][:, 0, 0] != 0)[:, None]
            want = want + (src["v_sh"][:, 0, 0] / c0)[:, None] * row[None, :]
            tz = _call_allowance(twin64, st["twin32"], "v_sh")[:, 0, 0] + \
                TWIN_COLOUR_ROUNDINGS * EPS32 * twin64["mag_sh"][:, 0, 0]
            tol = tol + (tz / c0)[:, None] * np.abs(_z_row(st["u"]))[None, :]
        err = np.abs(st["got"][k].astype(np.float64).reshape(want.shape) - want)
        ratio = err / (tol + 1e-300)
        i = int(np.argmax(ratio)) if ratio.size else 0
        ratios[k] = float(ratio.reshape(-1)[i]) if ratio.size else 0.0
        noflip[k] = float(ratio[~flips].max()) if (~flips).any() else 0.0
        print(f"[depth arbiter {st['kind']} det={st['det']} control={control}] {k}: worst err/tol {ratios[k]:.3f} "
              f"(err {float(err.reshape(-1)[i]) if ratio.size else 0.0:.3e}, want "
              f"{float(want.reshape(-1)[i]) if ratio.size else 0.0:.3e}), {int((ratio > 1.0).sum())} of {ratio.size} over; "
              f"off the {int(flips.sum())} elements with a flip allowance {noflip[k]:.3f}")
    for k in ARBITER_GRADS:
        assert ratios[k] <= 1.0, f"{st['kind']} det={st['det']} {k}: worst err/tol {ratios[k]:.3f} against the f64 arbiter"
    return {k: dict(worst=ratios[k], worst_noflip=noflip[k]) for k in ARBITER_GRADS}


def check_backward_arbiter(dev, kind, det, cloud, w, h, camera=None, max_intersects=None, control=None):
    """The depth backward against the float64 arbiter, element by element; returns the worst err/tol per tensor."""
    return arbiter_gate(arbiter_state(dev, kind, det, cloud, w, h, camera=camera, max_intersects=max_intersects), control)


def test_deterministic_backward_bitwise(dev):
    import torch

    cloud, w, h = _scene("c1")
    v_out, v_d = _upstream(dev, w, h, seed=7)
    a, _, _ = _grads(dev, cloud, w, h, True, v_out, v_d)
    b, _, _ = _grads(dev, cloud, w, h, True, v_out, v_d)
    for k in GRADS:
        assert a[k].tobytes() == b[k].tobytes(), k
    # v_D = 0: bit for bit the gradients of brush_render_backward
    z, _, _ = _grads(dev, cloud, w, h, True, v_out, torch.zeros_like(v_d))
    ref, _, _ = _grads(dev, cloud, w, h, True, v_out)
    for k in GRADS:
        assert z[k].tobytes() == ref[k].tobytes(), k
    assert np.abs(a["v_means"] - ref["v_means"]).max() > 0  # the depth term is there


# ---------------------------------------------------------------------------- 4. independent sanity checks
SMOOTH_CAMERA = dict(position=[0.0, 0.0, 0.0], rotation_xyzw=[0.0, 0.0, 0.0, 1.0], fov_x=0.5, fov_y=0.5,
                     center_uv=(0.5, 0.5))


def _smooth_scene(dev):
    """Four large splats in front of an identity camera: alpha >= 1/255 on the whole 32 x 32 frame and T far above
    the stop, so D is smooth in the means (no threshold crossings for the finite difference)."""
    import torch

    import brush_amd

    c = SMOOTH_CAMERA
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    means = torch.tensor([[0.2, -0.1, 5.0], [-0.3, 0.2, 6.5], [0.1, 0.3, 8.0], [-0.2, -0.25, 4.5]], device=dev)
    log_scales = torch.log(torch.tensor([[2.0, 1.6, 0.7], [1.8, 2.2, 1.0], [2.5, 2.0, 1.5], [1.7, 1.9, 0.5]],
                                        device=dev))
    quats = torch.nn.functional.normalize(torch.tensor([[1.0, 0.1, 0.0, 0.05], [0.9, 0.0, 0.2, 0.0],
                                                       [1.0, -0.1, 0.1, 0.1], [1.0, 0.0, 0.0, -0.2]], device=dev),
                                          dim=1)
    sh = torch.full((4, 1, 3), 0.3, device=dev)
    raw = torch.tensor([0.0, -0.5, 0.3, -1.0], device=dev)
    return cam, means, log_scales, quats, sh, raw


def test_central_difference_wrt_means(dev):
    check_central_difference(dev, *_smooth_scene(dev))


def check_central_difference(dev, cam, means, log_scales, quats, sh, raw):
    """The body of test_central_difference_wrt_means; returns (analytic, fd)."""
    import torch

    import brush_amd

    w = h = 32
    g = torch.Generator(device="cpu").manual_seed(3)
    r = torch.rand((h, w), generator=g).to(dev)
    d = torch.randn((4, 3), generator=g).to(dev)

    def loss(m):
        _, depth, _ = brush_amd.render_splats_depth(cam, (w, h), m, None, log_scales, quats, sh, raw)
        return (depth.double() * r.double()).sum()

    with torch.no_grad():
        img, depth, _ = brush_amd.render_splats_depth(cam, (w, h), means, None, log_scales, quats, sh, raw)
        assert float(img[..., 3].min()) > 0.05 and float(img[..., 3].max()) < 0.99
    m = means.clone().requires_grad_(True)
    loss(m).backward()
    analytic = float((m.grad.double() * d.double()).sum())
    eps = 1e-2
    with torch.no_grad():
        fd = (float(loss(means + eps * d)) - float(loss(means - eps * d))) / (2 * eps)
    # without the z term the directional derivative moves by sum v_z (d . viewmat row 2): far outside this margin
    assert abs(analytic - fd) <= 2e-3 * abs(fd) + 1e-3, (analytic, fd)
    return analytic, fd


def test_opaque_wall_at_known_distance(dev):
    import torch

    import brush_amd

    cam = brush_amd.Camera([0, 0, 0], [0, 0, 0, 1], 0.8, 0.8, (0.5, 0.5))
    w = h = 96
    dist = 7.25
    xs = torch.linspace(-3.0, 3.0, 25)
    gx, gy = torch.meshgrid(xs, xs, indexing="ij")
    n = gx.numel()
    means = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((n,), dist)], 1).to(dev)
    log_scales = torch.log(torch.tensor([0.4, 0.4, 1e-3])).repeat(n, 1).to(dev)  # flat, facing the camera
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1).to(dev)
    sh = torch.zeros((n, 1, 3), device=dev)
    raw = torch.full((n,), 6.0, device=dev)
    with torch.no_grad():
        img, depth, _ = brush_amd.render_splats_depth(cam, (w, h), means, None, log_scales, quats, sh, raw)
    a = img[..., 3]
    covered = a > 0.5
    assert float(covered.float().mean()) > 0.9
    norm = (depth / a)[covered]
    assert float((norm - dist).abs().max()) <= 1e-4 * dist, float((norm - dist).abs().max())


# ---------------------------------------------------------------------------- 5. capture and sync
def test_graph_capture_and_no_host_sync(dev):
    import torch

    import brush_amd

    cloud, w, h = _scene("ragged")
    t = _tensors(cloud, dev, grad=True)
    cam = _camera(w, h)
    v_out, v_d = _upstream(dev, w, h, seed=8)
    ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"]]

    def step():
        img, depth, _ = brush_amd.render_splats_depth(cam, (w, h), *_args(t), deterministic=True)
        gr = torch.autograd.grad([img, depth], ps, [v_out, v_d])
        return [img.detach(), depth.detach()] + list(gr)

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


# ---------------------------------------------------------------------------- 6. Splats.render_depth with a trainer
def test_splats_render_depth_with_lazy_sh_trainer(dev):
    import torch

    import brush_amd

    cloud, w, h = _scene("ragged")
    splats = brush_amd.Splats(*(torch.as_tensor(cloud[k], device=dev)
                                for k in ("means", "sh", "quats", "raw_opac", "log_scales")))
    tr = brush_amd.SplatTrainer(splats, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0,
                                                              deferred_sh_adam=True))
    cam = _camera(w, h)
    gt = torch.rand((h, w, 3), generator=torch.Generator(device="cpu").manual_seed(1)).to(dev)
    for _ in range(5):
        tr.step(splats, cam, gt)
    with torch.no_grad():
        img, depth, _ = splats.render_depth(cam, (w, h))
        img0, _ = splats.render(cam, (w, h))
    assert _np(img).tobytes() == _np(img0).tobytes()
    assert depth.shape == (h, w) and bool(torch.isfinite(depth).all())


# ---------------------------------------------------------------------------- 7. eval CLI --depth-dir
def test_eval_cli_depth_dir(dev, tmp_path):
    import torch

    import brush_amd

    rng = np.random.default_rng(21)
    n = 3000
    means = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, (n, 4, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    raw = rng.uniform(-1.0, 3.0, n).astype(np.float32)
    log_scales = np.log(rng.uniform(0.01, 0.05, (n, 3))).astype(np.float32)
    src = brush_amd.Splats(*(torch.from_numpy(a).to(dev) for a in (means, sh, quats, raw, log_scales)))
    ply = tmp_path / "cloud.ply"
    ply.write_bytes(src.to_ply())
    E.write_nerf(str(tmp_path / "nerf"), 120, 90, n_train=1, n_val=2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    runs = {}
    for tag, extra in (("plain", []), ("depth", ["--depth-dir", str(tmp_path / "depth")])):
        out = tmp_path / f"{tag}.json"
        r = subprocess.run([sys.executable, "-m", "brush_amd.eval", str(ply), str(tmp_path / "nerf"), "--json",
                            str(out)] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = (r.stdout, json.loads(out.read_text()))
    assert runs["plain"] == runs["depth"]
    assert not (tmp_path / "plain").exists()
    names = [v["name"] for v in runs["depth"][1]["views"]]
    assert len(names) == 2
    for name in names:
        stem = os.path.splitext(os.path.basename(name))[0]
        d = np.load(tmp_path / "depth" / f"{stem}_depth.npy")
        dn = np.load(tmp_path / "depth" / f"{stem}_depth_norm.npy")
        assert d.shape == (90, 120) and d.dtype == np.float32
        assert dn.shape == (90, 120) and dn.dtype == np.float32
        assert np.isfinite(dn).all() and (d > 0).any()
        assert ((dn[d > 0] > 2.0) & (dn[d > 0] < 6.5)).all()  # the cloud lies 4 +- sqrt(3) from the cameras
