"""Host checks of the normal kernels' references (tests/normal_ref64.py) and of what brush_amd/normal_loss.py and the
trainer's configuration decide without a device: the float32 restatement (which the GPU tests hold the kernels to, bit for
bit) against float64 autograd within the derived running error bound, a tilted plane's analytic normal, every validity
rule, the seeded GPU inputs' masks, the restated reduction order, TrainConfig's refusals and the argument checks."""
import math

import numpy as np
import pytest

from tests import normal_ref64 as NR

F = np.float32


def _ratio(got, want, tol):
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


SIZES = [(3, 3), (5, 5), (33, 31), (130, 67)]


# ---------------------------------------------------------------------------- 1. float32 against float64 autograd
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("bad", [False, True])
def test_pixel_restatement_matches_float64_autograd_within_the_running_bound(w, h, bad):
    c = NR.make_case(w, h, bad=bad)
    r32 = NR.normal_loss32(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], c["alpha_min"])
    want = NR.loss64(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], r32["counts"], r32["valid"])
    bound = NR.normal_loss_bound(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], c["alpha_min"], r32)
    if not bad:
        assert r32["valid"].sum() == (w - 2) * (h - 2)  # a random VALID case: every interior pixel
    assert r32["valid"].any()
    worst = {}
    for key, got in (("depth_normals", r32["depth_normals"]), ("v_depth", r32["v_depth"]),
                     ("v_normals_img", r32["v_normals_img"]), ("v_alpha", r32["v_pred_alpha"])):
        val, e = bound[key]
        assert np.isfinite(got).all(), key
        # the running evaluation in float64 IS the autograd value up to float64 rounding: the formulas are the gradient
        scale = np.abs(want[key]).max() + 1e-300
        assert np.abs(val - want[key]).max() <= 1e-9 * scale, key
        worst[key] = _ratio(got, want[key], e)
    lv, le = bound["loss"]
    assert abs(lv - want["loss"]) <= 1e-12 * max(abs(lv), 1e-30)
    worst["loss"] = abs(float(r32["stats"][0]) - want["loss"]) / le
    print(f"normal loss {w}x{h} bad={bad}: |f32 - f64| / bound", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert any(v > 0.0 for v in worst.values())  # (float32 is not float64: a bound of zero would be vacuous)
    # outside their support the gradients are exactly +0
    assert not r32["v_depth"][~r32["counts"]].view(np.uint32).any()
    assert not r32["v_normals_img"][~r32["valid"]].view(np.uint32).any()
    assert not r32["depth_normals"][~r32["valid"]].view(np.uint32).any()
    assert not r32["v_pred_alpha"][~r32["touched"]].view(np.uint32).any()


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_splat_restatement_matches_float64_autograd_within_the_running_bound(n):
    for seed in (0, -1):
        s = NR.make_splats(n, seed)
        normals, k, sign = NR.splat_normals32(s["viewmat"], s["means"], s["log_scales"], s["quats"])
        want_n, want_g = NR.splat_normals64(s["viewmat"], s["quats"], k, sign, s["v_normals"])
        zero = np.zeros((n, 4), F)
        got = NR.splat_normals_backward32(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"], zero)
        val, e, nval, ne = NR.splat_vjp_bound(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"])
        assert np.abs(val - want_g).max() <= 1e-12 * (np.abs(want_g).max() + 1.0)
        assert np.abs(nval - want_n).max() <= 1e-12
        assert 0.0 < _ratio(normals, want_n, ne) <= 1.0 and ne.max() < 64 * NR.U  # (a unit vector, a few roundings)
        r = _ratio(got, want_g, e)
        print(f"splat normal VJP n={n} seed={seed}: |f32 - f64| / bound {r:.4f}")
        assert 0.0 < r <= 1.0
        # the VJP accumulates: one float32 add per word
        acc = NR.splat_normals_backward32(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"],
                                          s["v_quats0"])
        assert np.array_equal(acc, (s["v_quats0"] + got).astype(F))
        # faces the camera: n . p <= 0 in float64 up to the rounding of a dot product near zero
        vm = s["viewmat"].astype(np.float64).reshape(4, 4)
        p = s["means"].astype(np.float64) @ vm[:3, :3] + vm[3, :3]
        assert ((want_n * p).sum(1) <= 64 * NR.U * np.abs(p).sum(1)).all()
        assert (sign == -1).any() or n == 1
        assert (sign == 1).any() or n == 1


def test_axis_ties_the_flip_and_a_zero_dot():
    s = NR.make_splats(65, -1)
    normals, k, sign = NR.splat_normals32(s["viewmat"], s["means"], s["log_scales"], s["quats"])
    assert list(k[1:6]) == [1, 0, 0, 2, 2]  # two-way ties, the three-way tie, a tie of the larger two, row 5
    assert sign[5] == 1 and np.array_equal(normals[5], np.array([0, 0, 1], F))  # dot == 0: not flipped
    nan = s["log_scales"].copy()
    nan[0] = [np.nan, -1.0, -2.0]
    nan[1] = [-1.0, np.nan, -2.0]
    nan[2] = [-1.0, -2.0, np.nan]
    assert list(NR.shortest_axis(nan)[:3]) == [0, 2, 1]  # every comparison with a NaN is false: nothing moves k
    # identity view: behind the camera (z < 0) a normal (0, 0, 1) has a negative dot and stays; in front it flips
    m = s["means"].copy()
    q = s["quats"].copy()
    ls = s["log_scales"].copy()
    q[6] = q[7] = [1, 0, 0, 0]
    ls[6] = ls[7] = [-1, -1, -2]
    m[6], m[7] = [0.1, 0.2, 3.0], [0.1, 0.2, -3.0]
    normals, _, sign = NR.splat_normals32(s["viewmat"], m, ls, q)
    assert sign[6] == -1 and sign[7] == 1 and normals[6][2] == -1 and normals[7][2] == 1


# ---------------------------------------------------------------------------- 2. a tilted plane
@pytest.mark.parametrize("normal,d", [((0.0, 0.0, -1.0), -4.0), ((0.3, -0.2, -0.933), -5.0), ((-0.5, 0.4, -0.768), -3.0)])
def test_a_tilted_planes_depth_gives_its_analytic_normal(normal, d):
    w, h = 21, 17
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    intr = NR.intrinsics(w, h)
    fx, fy, cx, cy = (float(x) for x in intr)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rx, ry = (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy
    z = d / (n[0] * rx + n[1] * ry + n[2])  # n . (z r) = d
    assert (z > 0).all()
    alpha = np.ones((h, w), F)
    depth = z.astype(F)  # alpha = 1: D = z, known to one rounding
    zeros = np.zeros((h, w, 3), F)
    r32 = NR.normal_loss32(intr, alpha, depth, None, 1.0, 0.5)
    assert r32["valid"].sum() == (w - 2) * (h - 2) and r32["stats"][0] == 0
    assert r32["stats"][1] == F((w - 2) * (h - 2) / (w * h))
    full = NR.normal_loss32(intr, alpha, depth, zeros, 1.0, 0.5)
    bound = NR.normal_loss_bound(intr, alpha, depth, zeros, 1.0, 0.5, full, depth_err=NR.U * np.abs(z))
    _, e = bound["depth_normals"]
    got = r32["depth_normals"][r32["valid"]]
    assert np.array_equal(got, full["depth_normals"][full["valid"]])
    r = _ratio(got, np.broadcast_to(n, got.shape), e[r32["valid"]])
    print(f"plane {normal}: |Nd - n| / bound {r:.4f}, worst error {np.abs(got - n).max():.3e}")
    assert r <= 1.0
    assert np.abs(got - n).max() < 1e-3  # (the bound itself is small here: the check above is not vacuous)
    assert got[:, 2].max() < 0  # faces the camera
    assert not r32["depth_normals"][~r32["valid"]].any()


# ---------------------------------------------------------------------------- 3. the validity rules
def _flat(w=7, h=7, z=4.0):
    return np.full((h, w), 0.9, F), np.full((h, w), 0.9 * z, F)


def _valid(alpha, depth, alpha_min=0.5):
    h, w = alpha.shape
    return NR.normal_loss32(NR.intrinsics(w, h), alpha, depth, None, 1.0, alpha_min)


def test_each_validity_rule_fires():
    a, d = _flat()
    base = _valid(a, d)
    interior = np.zeros((7, 7), bool)
    interior[1:-1, 1:-1] = True
    assert np.array_equal(base["valid"], interior)  # the border is never valid
    cross = np.zeros((7, 7), bool)
    cross[3, 2:5] = cross[2:5, 3] = True
    for name, (ai, di) in dict(low_alpha=(0.4999, None), zero_depth=(None, 0.0), neg_depth=(None, -1.0),
                               nan_alpha=(np.nan, None), nan_depth=(None, np.nan), inf_alpha=(np.inf, None),
                               inf_depth=(None, np.inf)).items():
        a, d = _flat()
        if ai is not None:
            a[3, 3] = ai
        if di is not None:
            d[3, 3] = di
        r = _valid(a, d)
        assert not r["counts"][3, 3] and r["counts"].sum() == 48, name
        assert np.array_equal(r["valid"], interior & ~cross), name  # the pixel and its four edge neighbours
        rule = {"low_alpha": "low_alpha", "zero_depth": "zero_depth", "neg_depth": "zero_depth"}.get(name, "nonfinite")
        assert r[rule][3, 3] and sum(int(r[k].sum()) for k in ("low_alpha", "zero_depth", "nonfinite")) == 1, name
    a, d = _flat()
    a[3, 3] = 0.5  # alpha == alpha_min counts
    assert _valid(a, d)["valid"][3, 3]
    # |c|^2 overflows while c is finite: two huge neighbours in different directions
    a, d = _flat()
    d[3, 4] = d[4, 3] = F(0.9e12)
    r = _valid(a, d)
    assert r["counts"].all() and r["overflow"][3, 3] and not r["valid"][3, 3]
    assert r["valid"][3, 5] and r["valid"][5, 3]  # one huge neighbour alone: still a (steep) normal
    # |c|^2 == 0: every product underflows
    a, d = _flat(z=1e-30)
    r = _valid(a, d)
    assert r["counts"].all() and r["degenerate"][1:-1, 1:-1].all() and not r["valid"].any()
    # frames without an interior
    for w, h in ((1, 1), (2, 5), (5, 2)):
        a, d = _flat(w, h)
        r = _valid(a, d)
        assert r["counts"].all() and not r["valid"].any() and r["stats"][1] == 0


@pytest.mark.parametrize("w,h", [(33, 31), (130, 67), (513, 512)])
def test_seeded_gpu_inputs_hold_every_rule_and_a_middling_valid_share(w, h):
    c = NR.make_case(w, h)
    r = NR.normal_loss32(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], c["alpha_min"], None)
    share = r["valid"].sum() / (w * h)
    print(f"{w}x{h}: valid share {share:.3f}", {k: int(r[k].sum()) for k in ("low_alpha", "zero_depth", "nonfinite",
                                                                              "overflow")})
    assert 0.25 <= share <= 0.75
    for rule in ("low_alpha", "zero_depth", "nonfinite", "overflow"):
        assert r[rule].any(), rule
    assert np.isnan(c["alpha"]).any() and np.isnan(c["depth"]).any() and np.isinf(c["depth"]).any()
    for key in ("depth_normals", "v_depth", "v_normals_img", "v_pred_alpha", "stats"):
        assert np.isfinite(r[key]).all(), key  # so that a comparison of bits is a comparison of numbers


def test_fixed_sum_is_a_sum_and_strides():
    rng = np.random.default_rng(3)
    for w, h in ((5, 5), (130, 67), (513, 512)):
        vals = rng.uniform(-1, 2, (h, w)).astype(F)
        valid = rng.uniform(size=(h, w)) < 0.6
        s, n = NR.fixed_sum(vals, valid)
        exact = math.fsum(float(x) for x in vals[valid])
        assert n == int(valid.sum())
        assert abs(s - exact) <= n * 2.0 ** -53 * float(np.abs(vals[valid]).sum())
    assert -(-513 // 16) * (512 // 16) > NR.MAX_ROWS  # 513x512 is the size at which the workgroups stride


# ---------------------------------------------------------------------------- 4. configuration and argument checks
def test_trainconfig_refusals_and_defaults():
    from brush_amd.train import TrainConfig, optimizer_path

    c = TrainConfig()
    assert c.normal_weight == 0.0 and c.normal_from_step == 7000 and c.normal_alpha_min == 0.5
    TrainConfig(normal_weight=0.05, normal_from_step=0).check()
    for kw in (dict(normal_weight=-0.1), dict(normal_weight=float("nan")), dict(normal_weight=float("inf")),
               dict(normal_from_step=-1), dict(normal_from_step=1.5), dict(normal_alpha_min=0.0),
               dict(normal_alpha_min=-0.5), dict(normal_weight=True)):
        with pytest.raises(ValueError, match="TrainConfig.normal_"):
            TrainConfig(**kw).check()
    # an active normal term is a depth gradient to the optimizer path
    assert optimizer_path(False, False, True, False, True, False) == "separate"
    assert optimizer_path(False, False, True, False, False, False) == "fused"


def test_trainlog_carries_the_weight():
    from brush_amd.train_loop import TrainLog

    log = TrainLog(0, np.zeros(0, F), normal_weight=0.05)
    assert log.to_json()["normal_weight"] == 0.05 and TrainLog(0, np.zeros(0, F)).normal_weight == 0.0


def test_command_line_flags(capsys):
    from brush_amd import eval as EV
    from brush_amd import train_loop as TLm
    from brush_amd.train import TrainConfig

    a = TLm.parser().parse_args(["scene"])
    assert a.normal_weight == 0.0 and a.normal_from_step == TrainConfig.normal_from_step == 7000
    a = TLm.parser().parse_args(["scene", "--normal-weight", "0.05", "--normal-from-step", "100"])
    assert a.normal_weight == 0.05 and a.normal_from_step == 100
    for bad in (["--normal-weight", "-1"], ["--normal-weight", "0.05", "--normal-from-step", "-3"]):
        with pytest.raises(SystemExit) as e:  # refused from TrainConfig.check, before the dataset is looked for
            TLm.main(["/nonexistent/scene"] + bad)
        assert e.value.code == 2 and "TrainConfig.normal_" in capsys.readouterr().err
    assert EV.parser().parse_args(["s.ply", "scene", "--normal-dir", "out"]).normal_dir == "out"
    assert EV.parser().parse_args(["s.ply", "scene"]).normal_dir is None


def test_argument_checks_that_need_no_device():
    import torch

    import brush_amd
    from brush_amd import _lib
    from brush_amd import normal_loss as NL

    for name in ("splat_normals", "depth_normals", "normal_loss_into", "normal_consistency_loss", "render_normals"):
        assert getattr(brush_amd, name) is getattr(NL, name)
    assert hasattr(brush_amd.Splats, "render_normals")
    u = _lib.BrushUniforms()
    u.img_size[:] = [8, 6]
    z = torch.zeros
    with pytest.raises(ValueError, match=r"means must be a float32 \[N,3\]"):
        NL.splat_normals(u, z(4, 2), z(4, 3), z(4, 4))
    with pytest.raises(ValueError, match=r"quats must be a float32 \[N,4\]"):
        NL.splat_normals(u, z(4, 3), z(4, 3), z(4, 3))
    with pytest.raises(ValueError, match="log_scales must be a float32"):
        NL.splat_normals(u, z(4, 3), z(4, 3, dtype=torch.float64), z(4, 4))
    with pytest.raises(ValueError, match="same number of rows"):
        NL.splat_normals(u, z(4, 3), z(5, 3), z(4, 4))
    with pytest.raises(ValueError, match="no CPU path"):
        NL.splat_normals(u, z(4, 3), z(4, 3), z(4, 4))
    cam = brush_amd.Camera([0.0, 0.0, -8.0], [0.0, 0.0, 0.0, 1.0], 0.6, 0.6, (0.5, 0.5))
    with pytest.raises(ValueError, match="img_size"):
        NL._uniforms(cam)
    assert tuple(NL._uniforms(cam, (8, 6)).img_size) == (8, 6) and NL._uniforms(u) is u
    with pytest.raises(ValueError, match=r"pred must be a float32 \[h,w,4\]"):
        NL.normal_loss_into(u, z(6, 8, 3), z(6, 8), z(6, 8, 3), None)
    with pytest.raises(ValueError, match="the uniforms describe a 8x6 frame"):
        NL.normal_loss_into(u, z(5, 8, 4), z(5, 8), z(5, 8, 3), None)
    with pytest.raises(ValueError, match="the uniforms describe a 8x6 frame"):
        NL.depth_normals(cam, (8, 6), z(6, 7, 4), z(6, 7))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha_min must be > 0"):
            NL._check_alpha_min(bad)
