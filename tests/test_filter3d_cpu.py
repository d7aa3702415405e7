"""The 3D smoothing filter without a GPU: the float64 reference of tests/filter3d_ref64.py against the covariance form
it abbreviates and against float64 autograd, the host-side view records, and the configuration / command-line checks."""
import math

import numpy as np
import pytest

from tests import filter3d_ref64 as F


def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    l = rng.uniform(-6.0, 1.0, (n, 3))
    o = rng.uniform(-6.0, 8.0, n)
    f = np.exp(rng.uniform(-7.0, 1.0, n))
    return rng, l, o, f


def test_reference_c_is_the_determinant_ratio_of_full_covariances():
    rng, l, o, f = _random_rows(200, 0)
    _, _, c, p = F.apply64(l, o, f)
    for i in range(200):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))  # a random rotation (or reflection: the determinant ratio is the same)
        sigma = q @ np.diag(np.exp(2.0 * l[i])) @ q.T
        want = math.sqrt(np.linalg.det(sigma) / np.linalg.det(sigma + f[i] ** 2 * np.eye(3)))
        assert abs(c[i] - want) <= 1e-9 * want
        # and the effective scales are those of Sigma + f^2 I: same eigenvectors, eigenvalues s^2 + f^2
        l2, _, _, _ = F.apply64(l[i:i + 1], o[i:i + 1], f[i:i + 1])
        assert np.allclose(np.sort(np.exp(2.0 * l2[0])), np.sort(np.linalg.eigvalsh(sigma + f[i] ** 2 * np.eye(3))),
                           rtol=1e-9)
    assert np.allclose(p, F.sigmoid(o) * c, rtol=1e-15)
    assert np.all(c > 0) and np.all(c < 1)


def test_reference_logit_form_is_the_logit_of_p():
    _, l, o, f = _random_rows(500, 1)
    _, o2, _, p = F.apply64(l, o, f)
    assert np.allclose(F.sigmoid(o2), p, rtol=1e-12, atol=0)


def test_reference_vjp_is_float64_autograd_of_its_forward():
    import torch

    rng, l, o, f = _random_rows(300, 2)
    v_l2, v_o2 = rng.normal(size=(300, 3)), rng.normal(size=300)
    tl = torch.tensor(l, dtype=torch.float64, requires_grad=True)
    to = torch.tensor(o, dtype=torch.float64, requires_grad=True)
    tf = torch.tensor(f, dtype=torch.float64)
    s = torch.exp(tl)
    tot = s * s + (tf * tf)[:, None]
    l2 = 0.5 * torch.log(tot)
    c = torch.prod(s / torch.sqrt(tot), dim=1)
    o2 = torch.logit(torch.sigmoid(to) * c)
    ref_l2, ref_o2, _, _ = F.apply64(l, o, f)
    assert np.allclose(l2.detach().numpy(), ref_l2, rtol=1e-13, atol=1e-13)
    assert np.allclose(o2.detach().numpy(), ref_o2, rtol=1e-10, atol=1e-10)
    ((l2 * torch.tensor(v_l2)).sum() + (o2 * torch.tensor(v_o2)).sum()).backward()
    v_l, v_o = F.vjp64(l, o, f, v_l2, v_o2)
    err_l = np.abs(tl.grad.numpy() - v_l).max()
    err_o = np.abs(to.grad.numpy() - v_o).max()
    print(f"vjp64 against float64 autograd: worst |diff| v_l {err_l:.2e}, v_o {err_o:.2e}")
    assert np.allclose(tl.grad.numpy(), v_l, rtol=1e-9, atol=1e-11)
    assert np.allclose(to.grad.numpy(), v_o, rtol=1e-9, atol=1e-11)


def test_reference_zero_filter_is_the_identity():
    rng, l, o, _ = _random_rows(100, 3)
    z = np.zeros(100)
    l2, o2, c, p = F.apply64(l, o, z)
    assert np.allclose(l2, l, rtol=0, atol=1e-14) and np.allclose(o2, o, rtol=0, atol=1e-9)
    assert np.allclose(c, 1.0, rtol=0, atol=1e-15) and np.allclose(p, F.sigmoid(o))
    v_l2, v_o2 = rng.normal(size=(100, 3)), rng.normal(size=100)
    v_l, v_o = F.vjp64(l, o, z, v_l2, v_o2)
    assert np.allclose(v_l, v_l2, rtol=1e-14) and np.allclose(v_o, v_o2, rtol=1e-10)


def test_reference_rates_on_hand_cases():
    """One camera at the origin of its own frame looking down +z of the world: the decisions and the length can be
    read off by hand."""
    from brush_amd.filter3d import VIEW_WORDS, view_records

    cam = F.look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 2.0 * math.atan(0.5), 100, 50)  # fx = 100
    rec = view_records([(cam, (100, 50))])
    assert rec.shape == (1, VIEW_WORDS) and rec.dtype == np.float32
    Wm, fx, fy, cx, cy, w, h = F.unpack_views(rec)
    assert abs(fx[0] - 100.0) < 1e-4 and (cx[0], cy[0], w[0], h[0]) == (50.0, 25.0, 100.0, 50.0)
    # the camera's local axes in world coordinates: x right, y down, z forward; p = W mean
    R = Wm[0, :, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.allclose(R[2], [0, 0, 1], atol=1e-6)
    local = np.array([[0.0, 0.0, 4.0],      # centre, depth 4: nu = 25
                      [0.0, 0.0, 0.1],      # nearer than 0.2
                      [2.5, 0.0, 4.0],      # u = 112.5 <= 115: inside the margin
                      [2.7, 0.0, 4.0],      # u = 117.5 > 115: outside
                      [0.0, -1.25, 4.0],    # t = -6.25 >= -7.5: inside
                      [0.0, -1.35, 4.0],    # t = -8.75: outside
                      [0.0, 0.0, -4.0]])    # behind
    means = (local @ R).astype(np.float32)  # world = R^T local (the camera sits at the origin)
    r = F.rates64(means, rec)
    assert r["valid"][:, 0].tolist() == [True, False, True, False, True, False, False]
    assert abs(r["filter"][0] - math.sqrt(0.2) / 25.0) < 1e-7
    assert np.allclose(r["filter"][~r["seen"]], r["filter"][r["seen"]].max())
    none = F.rates64(means[[1, 3, 5, 6]], rec)
    assert not none["seen"].any() and (none["filter"] == 0).all()
    empty = F.rates64(means, np.zeros((0, VIEW_WORDS), np.float32))
    assert (empty["filter"] == 0).all()
    _, edge = F.validity64(means, rec)
    assert edge.min() > 1e-2


def test_view_records_take_sizes_and_intrinsics_as_given():
    from brush_amd.dataset import SceneView
    from brush_amd.filter3d import view_records

    cam = F.look_at_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 0.8, 64, 48, center_uv=(0.4, 0.6))
    a = view_records([SceneView("v", cam, np.zeros((48, 64, 3), np.uint8))])
    b = view_records([(cam, (64, 48))])
    assert a.tobytes() == b.tobytes()
    assert a.view(np.uint32)[0, 20:24].tolist() == [64, 48, 0, 0]
    assert np.array_equal(a[0, :16].reshape(4, 4).T, cam.world_to_local())
    assert a[0, 16] == cam.focal((64, 48))[0] and a[0, 18] == np.float32(0.4) * np.float32(64)
    with pytest.raises(ValueError):
        view_records([(cam, (0, 48))])


def test_config_validation():
    from brush_amd import TrainConfig

    TrainConfig(filter3d=True).check_filter3d()
    assert TrainConfig().filter3d is False and TrainConfig().filter3d_every == 100
    assert TrainConfig().filter3d_variance == 0.2
    for bad in (dict(filter3d_every=0), dict(filter3d_every=2.5), dict(filter3d_every=True),
                dict(filter3d_variance=-0.1), dict(filter3d_variance=float("nan")), dict(filter3d_variance="0.2")):
        with pytest.raises(ValueError, match="filter3d"):
            TrainConfig(**bad).check_filter3d()
    with pytest.raises(ValueError, match="mcmc"):
        TrainConfig(filter3d=True, strategy="mcmc").check_filter3d()
    TrainConfig(filter3d=False, strategy="mcmc").check_filter3d()


def test_refusals_come_before_any_gpu_call():
    import torch

    from brush_amd import Splats
    from brush_amd.train import SplatTrainer, TrainConfig
    from brush_amd.train_loop import TrainLoop

    z = torch.zeros
    cpu_splats = Splats(z((4, 3)), z((4, 1, 3)), z((4, 4)), z((4,)), z((4, 3)))
    with pytest.raises(ValueError, match="mcmc"):
        SplatTrainer(cpu_splats, TrainConfig(filter3d=True, strategy="mcmc"))
    with pytest.raises(ValueError, match="filter3d_every"):
        SplatTrainer(cpu_splats, TrainConfig(filter3d_every=0))

    t = SplatTrainer.__new__(SplatTrainer)  # no GPU state needed: the checks come first
    t.config = TrainConfig(filter3d=True)
    with pytest.raises(ValueError, match="set_filter3d"):
        t.step(None, None, None)
    t.filter3d = torch.zeros(4)
    for kw in (dict(exchange=object()), dict(grad_sync=lambda block, aux: None)):
        with pytest.raises(ValueError, match="single-view"):
            t.step(None, None, None, **kw)
    m = SplatTrainer.__new__(SplatTrainer)
    m.config = TrainConfig(strategy="mcmc")
    with pytest.raises(ValueError, match="mcmc"):
        m.set_filter3d(torch.zeros(4))
    m.set_filter3d(None)
    with pytest.raises(ValueError, match="float32"):
        t.set_filter3d(torch.zeros(4))  # not on the GPU

    class Exchange:
        world = 2

    with pytest.raises(ValueError, match="multi-rank"):
        TrainConfig(filter3d=True).check(multi_rank=True)
    TrainConfig(filter3d=False).check(multi_rank=True)
    TrainConfig(filter3d=True).check(multi_rank=False)
    # TrainLoop derives multi_rank from its exchange's world size, before anything touches the dataset or a device
    with pytest.raises(ValueError, match="multi-rank"):
        TrainLoop(None, TrainConfig(filter3d=True), steps=20, exchange=Exchange())
    Exchange.world = 1
    with pytest.raises(AttributeError, match="train"):  # one rank is let through, as far as the dataset (None here)
        TrainLoop(None, TrainConfig(filter3d=True), steps=20, exchange=Exchange(), device="cpu")


def test_parser_flags_and_log():
    from brush_amd.train_loop import TrainLog, main, parser

    a = parser().parse_args(["scene"])
    assert a.filter3d is False and a.filter3d_every == 100
    a = parser().parse_args(["scene", "--filter3d", "--filter3d-every", "25"])
    assert a.filter3d is True and a.filter3d_every == 25
    for argv in (["scene", "--filter3d", "--strategy", "mcmc"], ["scene", "--filter3d", "--filter3d-every", "0"]):
        with pytest.raises(SystemExit):
            main(argv)
    log = TrainLog(3, np.zeros(3, np.float32), filter3d=True, filter3d_refreshes=[0, 2])
    j = log.to_json()
    assert j["filter3d"] is True and j["filter3d_refreshes"] == [0, 2]
    assert TrainLog(0, np.zeros(0, np.float32)).to_json()["filter3d"] is False


def test_eval_zoom_flags_and_camera():
    from brush_amd.eval import main, parser, zoomed_camera

    a = parser().parse_args(["s.ply", "scene", "--zoom", "4", "--image-dir", "out"])
    assert a.zoom == 4.0 and a.image_dir == "out"
    assert parser().parse_args(["s.ply", "scene"]).zoom is None
    for argv in (["s.ply", "scene", "--zoom", "4"], ["s.ply", "scene", "--image-dir", "out"],
                 ["s.ply", "scene", "--zoom", "0", "--image-dir", "out"]):
        with pytest.raises(SystemExit):
            main(argv)
    cam = F.look_at_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 0.8, 64, 48, center_uv=(0.4, 0.6))
    z = zoomed_camera(cam, (64, 48), 8.0)
    assert np.allclose(z.focal((64, 48)), 8.0 * np.asarray(cam.focal((64, 48))), rtol=1e-6)
    assert z.center_uv == cam.center_uv and np.array_equal(z.position, cam.position)
    assert np.array_equal(z.rotation, cam.rotation)


def test_filter3d_kernels_static_lds_and_no_spills():
    """The four kernels of filter3d.hip in the built library: the rates kernel's static LDS is one chunk of 64 view
    records of 96 bytes, the fill pass stages 16 wave maxima, the two per-step maps use none; nothing spills or uses
    scratch."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(root, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    import __graft_entry__ as G
    from brush_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        G.build()
    res = kd.resources(_lib.LIB_PATH, r"k_filter3d_")
    want = {"k_filter3d_rates": 64 * 96, "k_filter3d_fill_unseen": 16 * 4, "k_filter3d_apply": 0,
            "k_filter3d_backward": 0}
    seen = {}
    for name, r in res.items():
        kernel = next(k for k in sorted(want, key=len, reverse=True) if k in name)
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"]) == (0, 0, 0), name
        seen[kernel] = r["group_segment_fixed_size"]
    assert seen == want
    assert _lib.lib().brush_filter3d_view_chunk() == 64
