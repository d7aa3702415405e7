"""GPU checks of the depth-distortion term (brush_render_distortion, brush_distortion_compact_grads,
brush_render_backward_distortion, brush_amd/distortion.py, TrainConfig.distortion_weight): the hand-made kernel inputs
of tests/contrib_cases.py (and distortion_ref64's clamped pair) against the float64 reference of
tests/distortion_ref64.py in both modes; a rendered scene under an off-centre rotated camera (linearity, the reference
rows pushed through a float64 autograd projection, a central difference, v_sh = 0); autograd against the bare calls;
refusals; the trainer.

The gradient replay accumulates with float atomics and so does the compositing backward in the default mode (the only
one the term has): wherever two GPU results are compared with each other the gate is test_gpu_depth's linearity gate
(rtol 1e-3, atol 1e-4 of the gradient's largest magnitude), not equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import camera_cases as CamC
from tests import distortion_ref64 as R
from tests import distortion_scene as S
from tests import helpers as H
from tests import margins

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c["name"] for c in CASES]
MODES = {"depth": dict(mode="depth"), "ndc": R.NDC}
WORDS = list(R.ROW_WORDS)
OTHER_WORDS = [k for k in range(16) if k not in WORDS]
U = R.U
GRADS = ("v_means", "v_scales", "v_quats", "v_opac", "v_sh", "v_xy")


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def default_mode():
    """The term's only mode, whatever BRUSH_DETERMINISTIC says."""
    from brush_amd import render as Rn

    old = Rn.DETERMINISTIC
    Rn.DETERMINISTIC = False
    yield
    Rn.DETERMINISTIC = old


@functools.lru_cache(maxsize=None)
def ref(name, mode, mutate=None):
    """(depth, v, reference walk) of a case: computed once, shared and left unchanged."""
    case = BY_NAME[name]
    z, v = R.seeded_depth(case), R.seeded_v(case)
    return z, v, R.walk(case, z, v, mutate=mutate, **MODES[mode])


def _np(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = _np(a) if not isinstance(a, np.ndarray) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a, dev):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _cfg(mode):
    from brush_amd.distortion import distortion_config

    return distortion_config(**MODES[mode])


def _aux(case, dev):
    """The case's arrays as a RenderAux; what the entries do not read are one-word dummies."""
    import torch

    from brush_amd import _lib
    from brush_amd.render import RenderAux

    def t(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)

    dummy = torch.zeros(1, dtype=torch.int32, device=dev)
    aux = RenderAux(projected_splats=t(case["projected"], torch.float32), uniforms_buffer=dummy,
                    num_intersections=dummy, num_visible=t([case["num_visible"]], torch.int32), final_index=dummy,
                    cum_tiles_hit=dummy, tile_bins=t(case["tile_bins"], torch.int32),
                    compact_gid_from_isect=t(case["isect"], torch.int32),
                    global_from_compact_gid=t(case["g_from_c"], torch.int32), compact_from_global_gid=dummy,
                    overflow=dummy, max_intersects=int(case["isect"].shape[0]))
    u = _lib.BrushUniforms()
    u.img_size[:] = [case["w"], case["h"]]
    u.tile_bounds[:] = [case["tile_bins"].shape[1], case["tile_bins"].shape[0]]
    u.total_splats = case["n"]
    return u, aux


def prefill(case):
    """Seeded non-zero rows [n,16]: magnitudes around 1, both signs."""
    rng = np.random.default_rng(7200 + case["n"])
    a = rng.uniform(0.5, 2.0, (case["n"], 16)) * rng.choice([-1.0, 1.0], (case["n"], 16))
    return a.astype(np.float32)


def run_grads(case, dev, mode, v, stats=None, rows0=None):
    """(stats, rows after the add) of the two bare calls on a case."""
    from brush_amd.distortion import distortion_compact_grads_from_aux, distortion_from_aux

    u, aux = _aux(case, dev)
    z = _t(R.seeded_depth(case), dev)
    cfg = _cfg(mode)
    st = distortion_from_aux(u, aux, z, cfg) if stats is None else stats
    rows = _t(prefill(case) if rows0 is None else rows0, dev)
    distortion_compact_grads_from_aux(u, aux, z, cfg, st, _t(v, dev), rows)
    return st, _np(rows)


# ---------------------------------------------------------------------------- 1. the forward replay
@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_gate_repeatability_graph_and_frame(dev, case, mode):
    import torch

    from brush_amd.distortion import distortion_from_aux

    z, _, want = ref(case["name"], mode)
    u, aux = _aux(case, dev)
    zt, cfg = _t(z, dev), _cfg(mode)
    h, w = case["h"], case["w"]
    # the output lies inside a larger buffer: nothing outside the frame's h w 4 words may be touched
    guard = 4096
    big = torch.full((guard + h * w * 4 + guard,), float("nan"), device=dev)
    out = big[guard:guard + h * w * 4].view(h, w, 4)
    assert distortion_from_aux(u, aux, zt, cfg, out=out) is out
    got = _np(out)
    r = R.gate(want, stats=got)["stats"]
    per_word = [R.ratio(got[..., k], want["stats"][..., k], want["tol_stats"][..., k]) for k in range(4)]
    print(f"{case['name']} {mode}: stats err/tol {r:.4f} per word {per_word}")
    margins.record("distortion_stats", mode, r)
    assert r <= 1.0, (mode, per_word)
    assert not bits(got[~want["added"]]).any()  # exactly +0 where the reference adds nothing
    edge = _np(big)
    assert np.isnan(edge[:guard]).all() and np.isnan(edge[guard + h * w * 4:]).all()
    again = distortion_from_aux(u, aux, zt, cfg)
    assert np.array_equal(bits(got), bits(again))
    # graph replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    rep = torch.empty((h, w, 4), device=dev)
    with torch.cuda.stream(s):
        distortion_from_aux(u, aux, zt, cfg, out=rep)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        distortion_from_aux(u, aux, zt, cfg, out=rep)
    rep.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(rep))
    assert case["num_isect"] <= 1 or want["added"].any()


def test_forward_with_no_splats_writes_zeros(dev):
    import torch

    from brush_amd.distortion import distortion_from_aux

    case = BY_NAME["ragged_17x9"]
    u, aux = _aux(case, dev)
    u.total_splats = 0
    out = torch.full((case["h"], case["w"], 4), float("nan"), device=dev)
    distortion_from_aux(u, aux, torch.zeros(1, device=dev), _cfg("depth"), out=out)
    assert not bits(out).any()


# ---------------------------------------------------------------------------- 2. the gradient replay
@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compact_grads_gate_untouched_words_and_zero_v(dev, case, mode):
    _, v, want = ref(case["name"], mode)
    pre = prefill(case)
    _, rows = run_grads(case, dev, mode, v)
    added = rows[:, WORDS].astype(np.float64) - pre[:, WORDS].astype(np.float64)
    # the atomics round at the magnitude of the row: one rounding per partial sum at |prefill| + sum |terms|
    extra = R.C_DIST * want["partials"][:, None] * U * (np.abs(pre[:, WORDS]) + want["abs_rows"] + want["tol_rows"])
    r = R.gate(want, rows=added, extra_rows_tol=extra)["rows"]
    per_word = [R.ratio(added[:, j], want["rows"][:, j], (want["tol_rows"] + extra)[:, j]) for j in range(7)]
    print(f"{case['name']} {mode}: rows err/tol {r:.4f} per word {per_word}")
    margins.record("distortion_rows", mode, r)
    assert r <= 1.0, (mode, per_word)
    assert np.array_equal(bits(rows[:, OTHER_WORDS]), bits(pre[:, OTHER_WORDS]))      # words 5-7, 10-15
    assert np.array_equal(bits(rows[~want["touched"]]), bits(pre[~want["touched"]]))  # splats in no pixel's sum
    if case["num_isect"] > 1 and want["abs_rows"].any():
        assert not np.array_equal(bits(rows), bits(pre))
    # a zero upstream gradient leaves every bit
    _, same = run_grads(case, dev, mode, np.zeros_like(v))
    assert np.array_equal(bits(same), bits(pre))


def test_non_finite_v_stays_inside_its_own_records(dev):
    """An infinite v at one pixel reaches only the rows of the splats that pixel added."""
    case = BY_NAME["four_tiles"]
    z, v, want = ref(case["name"], "depth")
    v2 = v.copy()
    v2[3, 3] = np.inf
    only = R.walk(case, z, np.where(np.isinf(v2), 1.0, 0.0).astype(np.float32))["abs_rows"].any(axis=1)
    assert only.any() and not only.all()
    _, rows = run_grads(case, dev, "depth", v2, rows0=np.zeros((case["n"], 16), np.float32))
    assert np.isfinite(rows[~only]).all() and not np.isfinite(rows[only]).all()
    r = R.ratio(rows[~only][:, WORDS], want["rows"][~only], want["tol_rows"][~only])
    assert r <= 1.0, r


WRONG = [("pairs_twice", "random_200", "depth"), ("ignore_T", "random_200", "depth"), ("stop_added", "saturating", "depth"),
         ("global_row", "four_tiles", "depth"), ("global_row", "random_200", "ndc"), ("no_dmu", "random_200", "ndc"),
         ("clamp_grad", "clamped_pair", "depth"), ("suffix_incl", "random_200", "depth"), ("suffix_incl", "batch_65", "ndc")]


def test_every_mutation_is_named():
    assert {m for m, _, _ in WRONG} == set(R.MUTATIONS)


@pytest.mark.parametrize("mutation,name,mode", WRONG)
def test_each_wrong_reference_is_rejected_by_the_gpu_result(dev, mutation, name, mode):
    case = BY_NAME[name]
    _, v, want = ref(name, mode)
    _, _, bad = ref(name, mode, mutation)
    st, rows = run_grads(case, dev, mode, v, rows0=np.zeros((case["n"], 16), np.float32))
    got = dict(stats=_np(st), rows=rows[:, WORDS])
    assert R.passes(R.gate(want, **got))
    r = R.gate(bad, **got)
    print(mutation, name, mode, r)
    assert not R.passes(r), (mutation, name, r)


def test_deterministic_mode_is_refused(dev):
    import torch

    from brush_amd import _lib
    from brush_amd import render as Rn
    from brush_amd.distortion import distortion_compact_grads_from_aux, distortion_from_aux, render_distortion

    case = BY_NAME["four_tiles"]
    u, aux = _aux(case, dev)
    z, cfg = _t(R.seeded_depth(case), dev), _cfg("depth")
    st = distortion_from_aux(u, aux, z, cfg)
    aux.flags = _lib.AUX_DETERMINISTIC
    v = torch.ones((case["h"], case["w"]), device=dev)
    rows = torch.zeros((case["n"], 16), device=dev)
    with pytest.raises(ValueError, match="deterministic"):
        distortion_compact_grads_from_aux(u, aux, z, cfg, st, v, rows)
    s = aux._as_struct()
    rc = _lib.lib().brush_distortion_compact_grads(C.byref(u), C.byref(s), z.data_ptr(), C.byref(cfg), st.data_ptr(),
                                                   v.data_ptr(), case["n"], rows.data_ptr(), None)
    assert rc == -1 and not bool(rows.any())  # BRUSH_ERR_INVALID_ARG, nothing launched
    cloud = S.smooth_scene()
    t = {k: _t(a, dev) for k, a in cloud.items()}
    old = Rn.DETERMINISTIC
    Rn.DETERMINISTIC = True
    try:
        with pytest.raises(ValueError, match="deterministic"):
            render_distortion(CamC.camera(S.CAMERA, 32, 32), (32, 32), t["means"], t["log_scales"], t["quats"], t["sh"],
                              t["raw_opac"])
    finally:
        Rn.DETERMINISTIC = old


# ---------------------------------------------------------------------------- 3. a rendered scene
def _forward(dev, cloud, w, h, antialiased, cam=None):
    """(tensors, u, aux, img, depth map, compact depth) of one default-mode depth forward."""
    import torch

    from brush_amd import render as Rn

    t = {k: _t(a, dev) for k, a in cloud.items()}
    bufs = Rn._depth_buffers(cloud["means"].shape[0], (w, h), dev)
    with torch.no_grad():
        img, aux, u = Rn._forward_impl(cam or CamC.camera(S.CAMERA, w, h), (w, h), t["means"], t["log_scales"],
                                       t["quats"], t["sh"], t["raw_opac"], False, None, deterministic=False,
                                       depth=bufs, antialiased=antialiased)
    return t, u, aux, img, bufs[0], bufs[1]


def _backward(t, u, aux, img, zc, v_out, v_depth, dist=None):
    """The dense gradients (float64 numpy) of brush_render_backward_depth, or with dist = (cfg, stats, v) of
    brush_render_backward_distortion.  A second backward of the same forward zero-fills itself."""
    from brush_amd import render as Rn
    from brush_amd.distortion import backward_distortion

    if dist is None:
        g, _ = Rn._backward_impl(u, aux, t["means"], t["log_scales"], t["quats"], t["raw_opac"], t["sh"].shape[1], img,
                                 v_out, depth=(zc, v_depth))
    else:
        g, _ = backward_distortion(u, aux, t["means"], t["log_scales"], t["quats"], t["raw_opac"], t["sh"].shape[1],
                                   img, v_out, zc, v_depth, *dist)
    return {k: _np(g[k]).astype(np.float64) for k in GRADS}


def _upstream(dev, w, h, seed):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    v_out = (torch.rand((h, w, 4), generator=g) - 0.5).to(dev)
    v_d = ((torch.rand((h, w), generator=g) - 0.5) * 1e-2).to(dev)
    v = ((torch.rand((h, w), generator=g) - 0.3) * 0.5).to(dev)
    return v_out, v_d, v


@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("antialiased", [False, True], ids=["plain", "antialiased"])
def test_scene_linearity_reference_rows_and_zero_v_sh(dev, antialiased, mode):
    import torch

    from brush_amd.distortion import distortion_from_aux

    w, h = S.W, S.H
    cloud = S.scene()
    n = cloud["means"].shape[0]
    t, u, aux, img, _, zc = _forward(dev, cloud, w, h, antialiased)
    cfg = _cfg(mode)
    stats = distortion_from_aux(u, aux, zc, cfg)
    v_out, v_d, v = _upstream(dev, w, h, seed=11)
    zero4, zero2 = torch.zeros_like(v_out), torch.zeros_like(v_d)
    # (a) linearity: (v_out, v_depth, v) = backward_depth(v_out, v_depth) + (0, 0, v)
    full = _backward(t, u, aux, img, zc, v_out, v_d, (cfg, stats, v))
    base = _backward(t, u, aux, img, zc, v_out, v_d)
    term = _backward(t, u, aux, img, zc, zero4, zero2, (cfg, stats, v))
    for k in GRADS:
        want = base[k] + term[k]
        scale = float((np.abs(base[k]) + np.abs(term[k])).max())
        ok, err, bad = H.all_close_report(full[k], want, 1e-3, 1e-4 * scale + 1e-12)
        assert ok, f"linearity {k}: max_abs_err={err} bad={bad} scale={scale}"
    # (d) the term gives the colours nothing
    assert not term["v_sh"].any()
    assert np.abs(term["v_means"]).max() > 0 and np.abs(term["v_opac"]).max() > 0
    # (b) the (0, 0, v) gradients against the float64 reference rows of the aux read back, through the projection
    auxd = {k: _np(getattr(aux, k)) for k in ("projected_splats", "num_visible", "tile_bins", "compact_gid_from_isect",
                                              "global_from_compact_gid")}
    case = S.case_from_aux(auxd, w, h, n)
    nv = case["num_visible"]
    want = R.walk(case, _np(zc), _np(v), **MODES[mode])
    r_stats = R.gate(want, stats=_np(stats))["stats"]
    bad, share = S.excluded(want, nv)
    print(f"scene antialiased={antialiased} {mode}: visible {nv}, excluded {int(bad.sum())} ({share:.3f}), "
          f"stats err/tol {r_stats:.4f}")
    assert nv >= 150 and share <= S.MAX_EXCLUDED
    assert r_stats <= 1.0 or bad.any()
    pushed = S.push_rows(u, cloud, antialiased, want["rows"], want["tol_rows"], case["g_from_c"], nv)
    keep = np.ones(n, bool)
    keep[case["g_from_c"][:nv][bad[:nv]]] = False
    worst = {}
    for k, (grad, tol) in pushed.items():
        worst[k] = R.ratio(term[k][keep], grad[keep], tol[keep])
    print(f"scene antialiased={antialiased} {mode}: |GPU - reference| / allowance {worst}")
    for k, x in worst.items():
        margins.record("distortion_scene", f"{k}_{mode}_{'aa' if antialiased else 'plain'}", x)
    assert all(x <= 1.0 for x in worst.values()), worst
    unseen = np.ones(n, bool)
    unseen[case["g_from_c"][:nv]] = False
    assert not term["v_means"][unseen].any()


def test_central_difference_wrt_means(dev, default_mode):
    """Modelled on test_gpu_depth's: the directional derivative of sum r(p) L(p) along a random direction of the
    means against a central difference on a scene without threshold crossings."""
    import torch

    import brush_amd

    w = h = 32
    cloud = S.smooth_scene(w, h)
    t = {k: _t(a, dev) for k, a in cloud.items()}
    cam = CamC.camera(S.CAMERA, w, h)
    g = torch.Generator(device="cpu").manual_seed(3)
    r = torch.rand((h, w), generator=g).to(dev)
    d = (torch.randn((5, 3), generator=g) * 0.5).to(dev)
    for kw in (dict(mode="depth"), dict(mode="ndc", near=0.2, far=50.0)):
        def loss(m):
            _, _, dist, _ = brush_amd.render_distortion(cam, (w, h), m, t["log_scales"], t["quats"], t["sh"],
                                                        t["raw_opac"], **kw)
            return (dist.double() * r.double()).sum()

        with torch.no_grad():
            img, _, dist, _ = brush_amd.render_distortion(cam, (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                                          t["raw_opac"], **kw)
            assert float(img[..., 3].min()) > 0.05 and float(img[..., 3].max()) < 0.99 and float(dist.min()) > 0
        m = t["means"].clone().requires_grad_(True)
        loss(m).backward()
        analytic = float((m.grad.double() * d.double()).sum())
        eps = 1e-2
        with torch.no_grad():
            fd = (float(loss(t["means"] + eps * d)) - float(loss(t["means"] - eps * d))) / (2 * eps)
        print(f"central difference {kw['mode']}: analytic {analytic:.6g} fd {fd:.6g}")
        # the finite difference's own error: O(eps^2) relative, and the float32 roundings of the two losses over 2 eps
        assert abs(analytic - fd) <= 2e-3 * abs(fd) + 1e-4 * float((dist.double() * r.double()).sum()), (kw, analytic, fd)


def test_render_distortion_autograd_is_the_bare_calls(dev, default_mode):
    import torch

    import brush_amd
    from brush_amd.distortion import distortion_from_aux

    w, h = S.W, S.H
    cloud = S.scene()
    cam = CamC.camera(S.CAMERA, w, h)
    kw = dict(mode="ndc", near=0.2, far=50.0)
    t = {k: _t(a, dev).requires_grad_(True) for k, a in cloud.items()}
    img, depth, dist, aux = brush_amd.render_distortion(cam, (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                                        t["raw_opac"], antialiased=True, **kw)
    assert dist.shape == (h, w) and dist.requires_grad and img.requires_grad and depth.requires_grad
    v_out, v_d, v = _upstream(dev, w, h, seed=12)
    names = ("means", "log_scales", "quats", "sh", "raw_opac")
    got = torch.autograd.grad([img, depth, dist], [t[k] for k in names], [v_out, v_d, v])
    got = dict(zip(("v_means", "v_scales", "v_quats", "v_sh", "v_opac"), (_np(x).astype(np.float64) for x in got)))
    # the same by hand
    t2, u, aux2, img2, depth2, zc = _forward(dev, cloud, w, h, True)
    cfg = _cfg("ndc")
    stats = distortion_from_aux(u, aux2, zc, cfg)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(depth), bits(depth2))
    assert np.array_equal(bits(dist), bits(stats[..., 0]))
    want = _backward(t2, u, aux2, img2, zc, v_out, v_d, (cfg, stats, v))
    for k in got:
        scale = float(np.abs(want[k]).max())
        ok, err, bad = H.all_close_report(got[k], want[k], 1e-3, 1e-4 * scale + 1e-12)
        assert ok, f"{k}: max_abs_err={err} bad={bad} scale={scale}"
    # a gradient on the distortion alone reaches every parameter tensor but the colours
    only = torch.autograd.grad(brush_amd.render_distortion(cam, (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                                           t["raw_opac"], **kw)[2].sum(), [t[k] for k in names])
    assert all(bool(x.any()) for x, k in zip(only, names) if k != "sh") and not bool(only[3].any())
    # untracked: no graph; Splats.render_distortion is the same call on the normalised rotations
    with torch.no_grad():
        s = brush_amd.Splats(t["means"].detach(), t["sh"].detach(), t["quats"].detach() * 1.7, t["raw_opac"].detach(),
                             t["log_scales"].detach())
        i3, d3, x3, _ = s.render_distortion(cam, (w, h), antialiased=True, **kw)
        rot = s.rotation.detach()
        nrm = (rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))).contiguous()
        i4, d4, x4, _ = brush_amd.render_distortion(cam, (w, h), t["means"].detach(), t["log_scales"].detach(), nrm,
                                                    t["sh"].detach(), t["raw_opac"].detach(), antialiased=True, **kw)
    assert not x3.requires_grad and np.array_equal(bits(x3), bits(x4)) and np.array_equal(bits(i3), bits(i4))
    with pytest.raises(ValueError, match="far"):
        brush_amd.render_distortion(cam, (w, h), t["means"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"],
                                    mode="ndc")


def test_distortion_loss_into(dev):
    import torch

    from brush_amd.distortion import distortion_loss_into

    g = torch.Generator(device="cpu").manual_seed(4)
    h, w = 9, 17
    stats = torch.rand((h, w, 4), generator=g).to(dev)
    mask = (torch.rand((h, w), generator=g) < 0.6).to(torch.uint8).to(dev)
    accum = torch.full((1,), 0.25, device=dev)
    v = torch.empty((h, w), device=dev)
    out, term = distortion_loss_into(stats, v, weight=3.0, loss_accum=accum)
    kappa = 3.0 / (w * h)
    assert out is v and bool((v == np.float32(kappa)).all())
    want = kappa * float(stats[..., 0].double().sum())
    assert abs(float(term) - want) <= 2 * U * want and abs(float(accum) - (0.25 + want)) <= 4 * U * (0.25 + want)
    out, term = distortion_loss_into(stats, v, weight=3.0, mask=mask)
    assert bool((v[mask != 0] == np.float32(kappa)).all()) and not bool(v[mask == 0].any())
    want = kappa * float(stats[..., 0].double()[mask != 0].sum())
    assert abs(float(term) - want) <= 2 * U * want


# ---------------------------------------------------------------------------- 4. the trainer
def _moment_gate(got, want, what):
    scale = float(np.abs(want).max())
    ok, err, bad = H.all_close_report(got, want, 1e-3, 1e-4 * scale + 1e-12)
    assert ok, f"{what}: max_abs_err={err} bad={bad} scale={scale}"


@pytest.mark.parametrize("others", [False, True], ids=["alone", "with_depth_and_normal"])
def test_an_active_step_is_the_manual_composition(dev, default_mode, others):
    """One step with the term on against the calls made by hand: forward with depth, colour loss, (brush_depth_loss,
    the normal term,) brush_render_distortion, distortion_loss_into, brush_render_backward_distortion with the ONE
    summed depth gradient, brush_adam_step.  The loss is reproduced to the bits (no atomics in front of it); the first
    moments (0.1 times the gradient) within the float-atomics gate."""
    import torch

    import brush_amd
    from brush_amd import _lib as L
    from brush_amd import render as Rn
    from brush_amd.depth_loss import depth_loss_into
    from brush_amd.distortion import (backward_distortion, distortion_config, distortion_from_aux,
                                      distortion_loss_into)
    from brush_amd.features import feature_grads_from_aux, features_from_aux
    from brush_amd.normal_loss import normal_loss_into, splat_normals_backward_into, splat_normals_from
    from brush_amd.train import l1_ssim_loss
    from tests import test_gpu_depth_loss as TD

    W, Hh, AM = TD.W, TD.Hh, TD.ALPHA_MIN
    setup = TD._trainer_setup(dev)
    mk, cams, gts, depths = setup
    kw = dict(distortion_weight=50.0, distortion_from_step=0, distortion_mode="ndc", distortion_far=40.0)
    if others:
        kw.update(depth_weight=0.3, normal_weight=0.4, normal_from_step=0, normal_alpha_min=AM)
    for fused in (True, False):  # an active term takes the separate-call path whatever fused_backward says
        got_losses, got = TD._run_trainer(dev, setup, fused, True, with_depth=others, order=[1], **kw)
        s = mk()
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, depth_alpha_min=AM, **kw)
        clock = brush_amd.SplatTrainer(mk(), cfg)
        n, ncoef = s.num_splats(), int(s.sh_coeffs.shape[1])
        m1, m2 = torch.zeros(n * (11 + 3 * ncoef), device=dev), torch.zeros(n * (11 + 3 * ncoef), device=dev)
        l, stream = L.lib(), torch.cuda.current_stream().cuda_stream
        means, log_scales, quats = s.means.detach(), s.log_scales.detach(), s.rotation.detach()
        sh, raw_opac = s.sh_coeffs.detach(), s.raw_opacity.detach()
        norm_rot = torch.empty_like(quats)
        L.check(l.brush_normalize_quats(quats.data_ptr(), norm_rot.data_ptr(), n, stream), "normalize")
        bufs = Rn._depth_buffers(n, (W, Hh), dev)
        pred, aux, u = Rn._forward_impl(cams[1], (W, Hh), means, log_scales, norm_rot, sh, raw_opac, False, None,
                                        depth=bufs)
        loss, v_pred = l1_ssim_loss(pred, gts[1], cfg.ssim_weight, cfg.ssim_window_size, 1.0)
        v_depth, v_normals = None, None
        if others:
            v_depth, _ = depth_loss_into(pred, bufs[0], depths[1], v_pred, weight=0.3, scale=0.001, offset=0.0,
                                         alpha_min=AM, mode="depth", loss_accum=loss)
            nimg = features_from_aux(u, aux, splat_normals_from(u, means, log_scales, norm_rot))
            v_depth, v_nimg, _ = normal_loss_into(u, pred, bufs[0], nimg, v_pred, weight=0.4, alpha_min=AM,
                                                  loss_accum=loss, v_depth_accum=v_depth)
            v_normals = torch.zeros((n, 3), device=dev)
            feature_grads_from_aux(u, aux, v_nimg, v_normals)
            assert bool(v_depth.any())
        before = float(loss)
        dcfg = distortion_config("ndc", 0.2, 40.0)
        dstats = distortion_from_aux(u, aux, bufs[1], dcfg)
        v_dist, term = distortion_loss_into(dstats, torch.empty((Hh, W), device=dev), weight=50.0, loss_accum=loss)
        assert float(term) > 0 and float(loss) > before
        if v_depth is None:
            v_depth = torch.zeros((Hh, W), device=dev)
        g, _ = backward_distortion(u, aux, means, log_scales, norm_rot, raw_opac, ncoef, pred, v_pred, bufs[1], v_depth,
                                   dcfg, dstats, v_dist)
        plain, _ = Rn._backward_impl(u, aux, means, log_scales, norm_rot, raw_opac, ncoef, pred, v_pred,
                                     depth=(bufs[1], v_depth))
        assert not torch.equal(g["v_means"], plain["v_means"])  # the term is in the gradient
        if v_normals is not None:
            splat_normals_backward_into(u, means, log_scales, norm_rot, v_normals, g["v_quats"])
        acfg = L.BrushAdamConfig(clock._lr_mean(1.0), cfg.lr_scale, cfg.lr_rotation, cfg.lr_opac, cfg.lr_coeffs_dc,
                                 1.0 / cfg.lr_coeffs_sh_scale, 0.9, 0.999, 1e-15, 1, 1, 1.0)
        L.check(l.brush_adam_step(C.byref(acfg), n, Rn.sh_degree_from_coeffs(ncoef), means.data_ptr(),
                                  log_scales.data_ptr(), quats.data_ptr(), raw_opac.data_ptr(), sh.data_ptr(),
                                  g["v_means"].data_ptr(), g["v_scales"].data_ptr(), g["v_quats"].data_ptr(),
                                  g["v_opac"].data_ptr(), g["v_sh"].data_ptr(), m1.data_ptr(), m2.data_ptr(), stream),
                "adam")
        assert got_losses == [float(loss)], (fused, got_losses, float(loss))  # the loss to the bits
        # [means 3N | log_scales 3N | quats 4N | raw_opac N | sh]
        for name, sl in (("means", slice(0, 3 * n)), ("log_scales", slice(3 * n, 6 * n)), ("quats", slice(6 * n, 10 * n)),
                         ("raw_opac", slice(10 * n, 11 * n)), ("sh", slice(11 * n, None))):
            _moment_gate(_np(got["moment1"])[sl].astype(np.float64), _np(m1)[sl].astype(np.float64),
                         f"fused={fused} moment1 {name}")


def test_trainer_with_the_term_off_is_the_trainer_without_the_option(dev):
    """Off, or before distortion_from_step: bit for bit the step without the option, on the fused, deferred-SH and
    separate paths in deterministic mode; from distortion_from_step on the term is refused there."""
    import torch

    from brush_amd import render as Rn
    from tests import test_gpu_depth_loss as TD

    old = Rn.DETERMINISTIC
    Rn.DETERMINISTIC = True
    try:
        setup = TD._trainer_setup(dev)
        order = [0, 1, 1]
        for fused, deferred in TD.PATHS:
            off = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order)
            zero = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order, distortion_weight=0.0,
                                   distortion_from_step=0)
            early = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order, distortion_weight=50.0,
                                    distortion_from_step=3)
            for on in (zero, early):
                assert on[0] == off[0], (fused, deferred)
                for k in off[1]:
                    assert torch.equal(on[1][k], off[1][k]), (fused, deferred, k)
        with pytest.raises(ValueError, match="distortion_weight.*deterministic mode"):
            TD._run_trainer(dev, setup, True, True, with_depth=False, order=order, distortion_weight=50.0,
                            distortion_from_step=2)
    finally:
        Rn.DETERMINISTIC = old


def test_the_term_works_with_the_other_options(dev, default_mode):
    import torch

    import brush_amd
    from tests import test_gpu_depth_loss as TD

    setup = TD._trainer_setup(dev)
    mk, cams, gts, depths = setup
    kw = dict(distortion_weight=50.0, distortion_from_step=0)
    order = TD.ORDER[:5]
    for mode, extra in (("antialiased", dict(antialiased=True)), ("mcmc", dict(strategy="mcmc", mcmc_cap_max=512)),
                        ("depth+normal", dict(depth_weight=0.3, normal_weight=0.4, normal_from_step=0,
                                              normal_alpha_min=TD.ALPHA_MIN))):
        wd = mode == "depth+normal"
        on = TD._run_trainer(dev, setup, True, True, wd, order=order, **kw, **extra)
        off = TD._run_trainer(dev, setup, True, True, wd, order=order, **extra)
        assert np.isfinite(on[0]).all() and on[0][0] > off[0][0], mode
        for k, v in on[1].items():
            assert bool(torch.isfinite(v).all()), (mode, k)
        assert not torch.equal(on[1]["means"], off[1]["means"]), mode
    # masks: the term is masked by gt_mask; the 3D filter: gradients at the effective parameters
    s = mk()
    tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, filter3d=True, **kw))
    tr.set_filter3d(torch.full((s.num_splats(),), 0.01, device=dev))
    mask = torch.zeros((TD.Hh, TD.W), dtype=torch.uint8, device=dev)
    mask[:, : TD.W // 2] = 1
    full = float(tr.step(s, cams[0], gts[0])[0])
    assert np.isfinite(full) and bool(torch.isfinite(s.means).all())
    s2 = mk()
    tr2 = brush_amd.SplatTrainer(s2, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, **kw))
    s3 = mk()
    tr3 = brush_amd.SplatTrainer(s3, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0))
    l_on = float(tr2.step(s2, cams[0], gts[0], gt_mask=mask)[0])
    l_off = float(tr3.step(s3, cams[0], gts[0], gt_mask=mask)[0])
    s4 = mk()
    tr4 = brush_amd.SplatTrainer(s4, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, **kw))
    s5 = mk()
    tr5 = brush_amd.SplatTrainer(s5, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0))
    l_on_all = float(tr4.step(s4, cams[0], gts[0])[0])
    l_off_all = float(tr5.step(s5, cams[0], gts[0])[0])
    assert 0 < l_on - l_off < l_on_all - l_off_all  # half the frame carries less of the term than all of it
    # single-view: refused with grad_sync before anything is touched
    before = s2.means.detach().clone()
    with pytest.raises(ValueError, match="distortion_weight.*single-view"):
        tr2.step(s2, cams[0], gts[0], batch_views=2, grad_sync=lambda block, aux: None)
    assert torch.equal(s2.means.detach(), before) and tr2.iter == 1


E2E_STEPS = 200
E2E_WEIGHT = 100.0  # 2DGS's lambda for bounded scenes is 100 to 1000: a hyper-parameter, not a measured number


def test_training_with_the_term_lowers_the_distortion(dev, default_mode):
    """A 64 x 64 scene of 6 views of a textured plane; 1000 splats scattered in a slab around it are trained for 200
    steps from the same seed with and without the term (weight on from step 0, no refinement).  Afterwards the mean of
    L over the training views' pixels must be lower with the term: a comparison, asserted as one."""
    import torch

    import brush_amd
    from tests import test_gpu_train_loop as TL

    w = h = 64
    rng = np.random.default_rng(31)
    m = 900
    known = brush_amd.Splats.from_random_config(m, 0, (np.full(3, -1.0), np.full(3, 1.0)), rng, dev)
    with torch.no_grad():  # flat discs in the plane z = 0
        xy = rng.uniform(-1.4, 1.4, (m, 2))
        known.means.copy_(_t(np.c_[xy, np.zeros(m)].astype(np.float32), dev))
        known.rotation.copy_(_t(np.tile([1.0, 0.0, 0.0, 0.0], (m, 1)).astype(np.float32), dev))
        known.log_scales.copy_(_t(np.tile(np.log([0.09, 0.09, 0.005]), (m, 1)).astype(np.float32), dev))
        known.raw_opacity.fill_(float(np.log(0.9 / 0.1)))
    cams = [c for _, c in TL._ring_cameras(6, w, h, 4.0, 2.5, 0.1)]
    with torch.no_grad():
        gts = [known.render(cam, (w, h), False)[0][..., :3].clamp(0, 1).contiguous() for cam in cams]
    assert float(gts[0].max()) > 0.2

    def mean_distortion(splats):
        with torch.no_grad():
            return float(np.mean([float(splats.render_distortion(cam, (w, h))[2].mean()) for cam in cams]))

    out = {}
    for name, weight in (("without", 0.0), ("with", E2E_WEIGHT)):
        splats = brush_amd.Splats.from_random_config(1000, 0, (np.array([-1.4, -1.4, -0.4]), np.array([1.4, 1.4, 0.4])),
                                                     np.random.default_rng(5), dev)
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, seed=7, total_steps=E2E_STEPS,
                                    distortion_weight=weight, distortion_from_step=0)
        tr = brush_amd.SplatTrainer(splats, cfg)
        order = np.random.default_rng(9).integers(0, len(cams), E2E_STEPS)
        start = mean_distortion(splats)
        losses = [tr.step(splats, cams[i], gts[i], 1.0)[0] for i in order]
        tr.sync(splats)
        assert bool(torch.isfinite(torch.cat(losses)).all()) and splats.num_splats() == 1000
        out[name] = (start, mean_distortion(splats))
    print(f"mean L over the training views after {E2E_STEPS} steps (start, end): without the term {out['without']}, "
          f"with weight {E2E_WEIGHT} {out['with']}")
    margins.record("distortion_e2e", "without", out["without"][1])
    margins.record("distortion_e2e", "with", out["with"][1])
    assert out["without"][0] == out["with"][0] and out["without"][0] > 0
    assert out["with"][1] < out["without"][1]
