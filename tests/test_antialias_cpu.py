"""CPU checks of the antialiased mode (include/brush_hip.h: BRUSH_AUX_ANTIALIASED): the float64 reference of the comp
VJP against central differences, the new Python arguments and CLI flags, and the refusal paths that need no GPU."""
import inspect

import numpy as np
import pytest

from tests import aa_ref64 as A
from tests import helpers as H


def _uniforms(w, h, n):
    import brush_amd
    from brush_amd.render import pack_uniforms

    c = H.reference_test_camera(w, h)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    return pack_uniforms(cam, (w, h), 0, n)


CASES_SIZE = (160, 120)


def cases_cloud():
    return H.synthetic_cloud(4000, 0, seed=11, mean_mult=1.0)


def _cases(u=None, cloud=None):
    """Splats of a synthetic cloud in front of the reference camera, clamp inactive, comp well inside (0, 1), scales
    spread so that comp covers sub-pixel and large splats.  `u`, `cloud`: another camera's packed uniforms of a
    CASES_SIZE frame and the cloud to take the splats from."""
    cloud = cases_cloud() if cloud is None else cloud
    u = _uniforms(*CASES_SIZE, cloud["means"].shape[0]) if u is None else u
    means = cloud["means"].astype(np.float64)
    ls = cloud["log_scales"].astype(np.float64)
    q = cloud["quats"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    W = np.array([[u.viewmat[c * 4 + r] for c in range(3)] for r in range(3)])
    z = means @ W.T + np.array(u.viewmat[12:15])
    comp = A.comp64(u, means, ls, q)
    ok = (z[:, 2] > 0.5) & ~A.clamp_active(u, means) & (comp > 0.02) & (comp < 0.98)
    idx = np.nonzero(ok)[0][:64]
    assert idx.size >= 32, idx.size
    return u, means[idx], ls[idx], q[idx]


def _cd(fn, x, h):
    g = np.zeros_like(x)
    for j in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        g[:, j] = (fn(xp) - fn(xm)) / (2 * h)
    return g


def test_comp_vjp_matches_central_differences():
    """float64 analytic VJP (the backward's own formula) against central differences of comp64.  Step 1e-6 of O(1)
    inputs: truncation O(h^2) ~ 1e-12, cancellation ~ 1e-16 / 1e-6 = 1e-10 relative; the backward's 1e-6 added to comp
    in 0.5 / (comp + 1e-6) biases by at most 1e-6 / 0.02 = 5e-5 relative.  Tolerance: 2e-4 relative to the largest
    component of the splat's gradient, plus 1e-8 absolute."""
    check_comp_vjp()


def check_comp_vjp(u=None, cloud=None):
    """The body of test_comp_vjp_matches_central_differences at the camera of the packed uniforms `u`."""
    u, m, ls, q = _cases(u, cloud)
    rng = np.random.default_rng(3)
    v = rng.uniform(0.5, 1.5, m.shape[0])
    gm, gs, gq = A.comp_vjp64(u, m, ls, q, v)
    f = lambda mm, ll, qq: v * A.comp64(u, mm, ll, qq)
    cm = _cd(lambda x: f(x, ls, q), m, 1e-6)
    cs = _cd(lambda x: f(m, x, q), ls, 1e-6)
    cq = _cd(lambda x: f(m, ls, x), q, 1e-6)
    for name, got, want in (("means", gm, cm), ("log_scales", gs, cs), ("quats", gq, cq)):
        scale = np.abs(want).max(axis=1, keepdims=True)
        err = np.abs(got - want)
        tol = 2e-4 * scale + 1e-8
        print(f"{name}: max err {err.max():.3e}, max rel {float((err / (scale + 1e-30)).max()):.3e}")
        assert (err <= tol).all(), (name, float(err.max()), int((err > tol).sum()))


def test_comp_is_one_for_large_and_zero_for_degenerate_splats():
    cov = np.array([[[1e6, 0.0], [0.0, 1e6]], [[1.0, 1.0], [1.0, 1.0]], [[-1.0, 0.0], [0.0, 2.0]]])
    c = A.comp_from(cov, cov + A.COV_BLUR * np.eye(2))
    assert abs(c[0] - 1.0) < 1e-6 and c[1] == 0.0 and c[2] == 0.0


def test_word8_bound_is_a_small_relative_bound_for_resolved_splats():
    """The bound is tight enough to mean something where det(S) is resolved: below 1e-4 relative for most splats."""
    u, m, ls, q = _cases()
    raw = np.zeros(m.shape[0])
    want, bound = A.word8_bound(u, m, ls, q, raw)
    assert (bound > 0).all() and np.median(bound / want) < 1e-4


def test_python_arguments_exist_and_default_off():
    import brush_amd
    from brush_amd import _lib, render as R
    from brush_amd.eval import eval_stats
    from brush_amd.gaussian_splats import Splats
    from brush_amd.train import TrainConfig

    assert _lib.AUX_ANTIALIASED == 4
    for fn in (R.render_splats, R.render_splats_depth, R.render_rgba8, Splats.render, Splats.render_depth, eval_stats,
               R._forward_impl):
        p = inspect.signature(fn).parameters
        assert "antialiased" in p and p["antialiased"].default is False, fn
    assert brush_amd.render_splats is R.render_splats
    assert TrainConfig().antialiased is False and TrainConfig(antialiased=True).antialiased is True
    aux = R.RenderAux(*([None] * 11), flags=_lib.AUX_ANTIALIASED | _lib.AUX_DETERMINISTIC)
    assert aux.antialiased and aux.deterministic and aux.workspace_flags == _lib.AUX_DETERMINISTIC
    assert not R.RenderAux(*([None] * 11), flags=_lib.AUX_DETERMINISTIC).antialiased
    assert R.RenderAux(*([None] * 11), flags=_lib.AUX_ANTIALIASED).workspace_flags == 0


def test_cli_flags_parse():
    from brush_amd import eval as E
    from brush_amd import train_loop as T

    assert E.parser().parse_args(["a.ply", "d", "--antialiased"]).antialiased is True
    assert E.parser().parse_args(["a.ply", "d"]).antialiased is False
    assert T.parser().parse_args(["d", "--antialiased"]).antialiased is True
    assert T.parser().parse_args(["d"]).antialiased is False


def test_eval_stats_passes_the_mode_to_the_render(monkeypatch):
    """eval_stats renders every view with the mode it is given (CPU stand-ins for the splats and the metrics)."""
    import torch

    from brush_amd import eval as E

    seen = []

    class FakeSplats:
        means = torch.zeros((1, 3))

        def render(self, camera, size, u32, antialiased=False):
            seen.append(antialiased)
            return torch.zeros((size[1], size[0], 4)), None

    class View:
        def __init__(self):
            self.image = np.zeros((4, 5, 3), np.uint8)
            self.camera = None
            self.name = "v"

    class Scene:
        views = [View(), View()]

    monkeypatch.setattr(E, "eval_metrics", lambda pred, gt, window, out: out.zero_())
    E.eval_stats(FakeSplats(), Scene(), antialiased=True)
    E.eval_stats(FakeSplats(), Scene())
    assert seen == [True, True, False, False]


def test_train_loop_main_passes_the_mode(monkeypatch, tmp_path):
    """python -m brush_amd.train_loop --antialiased: TrainConfig.antialiased is set and the JSON log records it."""
    import json

    import torch

    from brush_amd import train_loop as T

    got = {}

    class Log:
        steps, seconds, train_seconds, num_splats, image_bytes = 0, 1.0, 1.0, 0, 0
        losses = np.zeros(0)

        def to_json(self):
            return {}

    class Data:
        class train:
            views = [object()]
        eval = None

    def fake_train(data, config, **kw):
        got["config"] = config
        return None, Log()

    monkeypatch.setattr(T, "load_dataset", lambda *a, **k: (Data(), None))
    monkeypatch.setattr(T, "train_scene", fake_train)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    out = tmp_path / "log.json"
    assert T.main([str(tmp_path), "--steps", "0", "--antialiased", "--json", str(out)]) == 0
    assert got["config"].antialiased is True
    assert json.loads(out.read_text())["antialiased"] is True
    assert T.main([str(tmp_path), "--steps", "0", "--json", str(out)]) == 0
    assert got["config"].antialiased is False
    assert json.loads(out.read_text())["antialiased"] is False


def test_trainer_refuses_exchange_in_antialiased_mode():
    from brush_amd.train import SplatTrainer, TrainConfig

    t = SplatTrainer.__new__(SplatTrainer)  # no GPU state needed: the check comes first
    t.config = TrainConfig(antialiased=True)
    with pytest.raises(ValueError):
        t.step(None, None, None, exchange=object())
