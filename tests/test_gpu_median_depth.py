"""GPU checks of the median depth (brush_render_median_depth, brush_amd/median_depth.py, brush_tsdf_integrate_ex):
the hand-made kernel inputs of tests/median_cases.py against the float64 reference of tests/median_ref64.py (decided
pixels exactly, undecided ones between the moved crossings, wrong references rejected, every pixel written), a rendered
scene with its exact properties, a silhouette where the expected depth blends and the median does not, the metric mode
of the TSDF fusion, and both command lines."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as E
from tests import helpers as H
from tests import median_cases as MC
from tests import median_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = MC.case_level_params()
CAP = 0.02
SENTINEL_DEPTH, SENTINEL_ID = -12345.0, -7


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _bits(t):
    import torch

    return t.detach().contiguous().view(-1).view(dtype=torch.int32).cpu().numpy()


# ---------------------------------------------------------------------------- 1. hand-made kernel inputs
def _run_case(case, level, dev, want_ids=True):
    """The kernel on a hand-made case through median_depth_from_aux, into outputs pre-filled with a sentinel; the aux
    arrays the entry does not read are one-word dummies.  Returns (ids, depth) as numpy arrays."""
    import torch

    from brush_amd import _lib
    from brush_amd.median_depth import median_depth_from_aux
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
    depth = torch.full((case["h"], case["w"]), SENTINEL_DEPTH, dtype=torch.float32, device=dev)
    ids = torch.full((case["h"], case["w"]), SENTINEL_ID, dtype=torch.int32, device=dev)
    got = median_depth_from_aux(u, aux, t(case["z"], torch.float32), level=level, want_ids=want_ids, out=(depth, ids))
    assert got[0] is depth and got[1] is (ids if want_ids else None)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), depth.cpu().numpy()


@pytest.mark.parametrize("param", PARAMS, ids=MC.param_id)
def test_hand_made_case(dev, param):
    case, level = param
    ref = R.walk(case, level)
    ids, depth = _run_case(case, level, dev)
    g = R.gate(case, ids, depth, ref)
    print(f"{MC.param_id(param)}: with a median {int((ref['id'] >= 0).sum())}, undecided {g['undecided']}, "
          f"bad decided {g['bad_decided']}, bad undecided {g['bad_undecided']}")
    assert (ids != SENTINEL_ID).all() and (depth != SENTINEL_DEPTH).all()   # every pixel is written
    assert g["undecided"] <= CAP * ids.size
    assert g["ok"], g
    assert np.array_equal(ids >= 0, depth != 0.0)
    # two runs give equal bits; without ids the depth is the same and the id buffer is left alone
    ids2, depth2 = _run_case(case, level, dev)
    assert ids2.tobytes() == ids.tobytes() and depth2.tobytes() == depth.tobytes()
    ids3, depth3 = _run_case(case, level, dev, want_ids=False)
    assert depth3.tobytes() == depth.tobytes() and (ids3 == SENTINEL_ID).all()
    # the wrong references fail the gate wherever they differ from the right one on a decided pixel
    for m in R.MUTATIONS:
        wrong = R.walk(case, level, mutate=m)
        if not R.gate(case, ref["id"], ref["depth"], wrong)["ok"]:
            assert not R.gate(case, ids, depth, wrong)["ok"], m


def test_each_wrong_reference_fails_on_the_device(dev):
    by_name = {c["name"]: c for c, _ in MC.all_cases()}
    for m, name, level in (("lt", "exact_half", 0.5), ("last", "random_200", 0.5), ("before", "cross_at_65", 0.5),
                           ("stop_counts", "stop_before_crossing", MC.STOP_LEVEL)):
        case = by_name[name]
        ids, depth = _run_case(case, level, dev)
        assert R.gate(case, ids, depth, R.walk(case, level))["ok"]
        assert not R.gate(case, ids, depth, R.walk(case, level, mutate=m))["ok"], (m, name)


def test_exact_ties_on_the_device(dev):
    """next_T == t_level exactly: `<=` makes that entry the median."""
    by_name = {c["name"]: c for c, _ in MC.all_cases()}
    for name, level, (y, x) in (("exact_half", 0.5, (8, 8)), ("quadrant_skip", 0.5, (3, 3)), ("exact_pair", 0.25, (8, 8))):
        case = by_name[name]
        ids, depth = _run_case(case, level, dev)
        assert int(ids[y, x]) == int(case["g_from_c"][0]), name
        assert depth[y, x].view(np.uint32) == case["z"][0].view(np.uint32), name
    # the crossing entry as the last of a staging batch and as the first of the next
    for position in (64, 65):
        case = by_name[f"cross_at_{position}"]
        ids, depth = _run_case(case, 0.5, dev)
        assert (ids == int(case["g_from_c"][position - 1])).all() and (depth == case["z"][position - 1]).all()


# ---------------------------------------------------------------------------- 2. a rendered scene
def _camera(w, h, position=None):
    import brush_amd

    c = H.reference_test_camera(w, h)
    return brush_amd.Camera(position or c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def _scene_splats(dev):
    import torch

    import brush_amd

    s = MC.rendered_scene()
    return brush_amd.Splats(*(torch.from_numpy(s[k]).to(dev) for k in ("means", "sh", "quats", "raw_opacity",
                                                                        "log_scales")))


def _bare(splats, cam, size, level, antialiased):
    """One depth forward and the replay, keeping compact_depth: (img, depth, median, ids, aux, compact_depth)."""
    import torch

    from brush_amd import render as Rn
    from brush_amd.median_depth import median_depth_from_aux

    with torch.no_grad():
        bufs = Rn._depth_buffers(splats.num_splats(), size, splats.means.device)
        img, aux, u = Rn._forward_impl(cam, size, splats.means.detach(), splats.log_scales.detach(),
                                       splats._synced_norm_rotation(), splats.sh_coeffs.detach(),
                                       splats.raw_opacity.detach(), False, None, expect_backward=False, depth=bufs,
                                       antialiased=antialiased)
        median, ids = median_depth_from_aux(u, aux, bufs[1], level=level)
    return img, bufs[0], median, ids, aux, bufs[1]


def _aux_equal(a, b):
    nv, ni = a.read_num_visible(), a.read_num_intersections()
    assert (nv, ni) == (b.read_num_visible(), b.read_num_intersections())
    assert a.flags == b.flags and a.max_intersects == b.max_intersects
    assert _bits(a.tile_bins).tobytes() == _bits(b.tile_bins).tobytes()
    assert _bits(a.final_index).tobytes() == _bits(b.final_index).tobytes()
    assert _bits(a.projected_splats[:nv]).tobytes() == _bits(b.projected_splats[:nv]).tobytes()
    assert _bits(a.global_from_compact_gid[:nv]).tobytes() == _bits(b.global_from_compact_gid[:nv]).tobytes()
    assert _bits(a.compact_gid_from_isect[:ni]).tobytes() == _bits(b.compact_gid_from_isect[:ni]).tobytes()


@pytest.mark.parametrize("antialiased", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("size", MC.SCENE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rendered_scene(dev, size, antialiased):
    import torch

    from brush_amd import render_splats_depth

    w, h = size
    splats = _scene_splats(dev)
    cam = _camera(w, h)
    with torch.no_grad():
        img0, depth0, aux0 = render_splats_depth(cam, size, splats.means, None, splats.log_scales,
                                                 splats._synced_norm_rotation(), splats.sh_coeffs, splats.raw_opacity,
                                                 antialiased=antialiased)
    med = {}
    for level in MC.LEVELS:
        img, depth, median, ids, aux = splats.render_median_depth(cam, size, level=level, antialiased=antialiased)
        assert not any(t.requires_grad for t in (img, depth, median, ids))
        assert _bits(img).tobytes() == _bits(img0).tobytes() and _bits(depth).tobytes() == _bits(depth0).tobytes()
        _aux_equal(aux, aux0)
        assert aux.antialiased == antialiased
        b_img, b_depth, b_median, b_ids, b_aux, cdepth = _bare(splats, cam, size, level, antialiased)
        assert _bits(b_median).tobytes() == _bits(median).tobytes() and _bits(b_ids).tobytes() == _bits(ids).tobytes()
        nv, ni = b_aux.read_num_visible(), b_aux.read_num_intersections()
        assert nv > 100
        case = MC.case_from_aux(f"scene_{w}x{h}", w, h, MC.SCENE_N, b_aux.projected_splats.cpu().numpy(),
                                b_aux.tile_bins.cpu().numpy(), b_aux.compact_gid_from_isect.cpu().numpy(),
                                b_aux.global_from_compact_gid.cpu().numpy(), nv, cdepth.cpu().numpy())
        ref = R.walk(case, level)
        ids_h, median_h = ids.cpu().numpy(), median.cpu().numpy()
        g = R.gate(case, ids_h, median_h, ref)
        print(f"{w}x{h} aa={antialiased} level {level}: with a median {int((ids_h >= 0).sum())} of {ids_h.size}, {g}")
        assert g["undecided"] <= CAP * ids_h.size
        assert g["ok"], g
        # median == z of ids through compact_from_global_gid, by bits
        c_from_g = b_aux.compact_from_global_gid.cpu().numpy().astype(np.int64)
        has = ids_h >= 0
        cz = cdepth.cpu().numpy()
        assert (c_from_g[ids_h[has]] >= 0).all() and (c_from_g[ids_h[has]] < nv).all()
        assert np.array_equal(median_h[has].view(np.uint32), cz[c_from_g[ids_h[has]]].view(np.uint32))
        assert (median_h[~has] == 0.0).all() and (ids_h[~has] == -1).all()
        med[level] = (ids_h, median_h)
        if level == 0.5:  # the walk's 1 - T is exact around one half
            alpha = img[..., 3].cpu().numpy()
            assert np.array_equal(has, alpha >= 0.5)
            if size == (64, 64):
                assert 0.2 < has.mean() < 1.0
    # the lists are depth sorted: a higher level is reached at a deeper splat
    all3 = (med[0.25][0] >= 0) & (med[0.5][0] >= 0) & (med[0.75][0] >= 0)
    assert all3.any()
    assert (med[0.25][1][all3] <= med[0.5][1][all3]).all() and (med[0.5][1][all3] <= med[0.75][1][all3]).all()
    # where a higher level is reached, so is every lower one
    assert not ((med[0.75][0] >= 0) & (med[0.5][0] < 0)).any() and not ((med[0.5][0] >= 0) & (med[0.25][0] < 0)).any()
    torch.cuda.synchronize()


def test_nothing_to_see(dev):
    import torch

    import brush_amd

    w, h = 33, 20
    cam = _camera(w, h)
    empty = brush_amd.Splats(torch.zeros((0, 3), device=dev), torch.zeros((0, 1, 3), device=dev),
                             torch.zeros((0, 4), device=dev), torch.zeros((0,), device=dev),
                             torch.zeros((0, 3), device=dev))
    behind = _scene_splats(dev)
    with torch.no_grad():
        behind.means[:, 2] -= 100.0  # everything behind the camera
    for splats in (empty, behind):
        img, depth, median, ids, aux = splats.render_median_depth(cam, (w, h))
        assert aux.read_num_visible() == 0
        assert median.shape == (h, w) and ids.shape == (h, w) and ids.dtype == torch.int32
        assert bool((median == 0).all()) and bool((ids == -1).all()) and not bool(img.any())


def test_bad_arguments(dev):
    import torch

    from brush_amd.median_depth import median_depth_from_aux

    splats = _scene_splats(dev)
    cam = _camera(32, 32)
    for level in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="level"):
            splats.render_median_depth(cam, (32, 32), level=level)
    img, depth, median, ids, aux, cdepth = _bare(splats, cam, (32, 32), 0.5, False)
    from brush_amd.render import pack_uniforms

    u = pack_uniforms(cam, (32, 32), 0, splats.num_splats())
    with pytest.raises(ValueError, match="compact_depth"):
        median_depth_from_aux(u, aux, cdepth[:10])
    with pytest.raises(ValueError, match="out: median"):
        median_depth_from_aux(u, aux, cdepth, out=(torch.zeros((32, 31), device=dev), ids))
    with pytest.raises(ValueError, match="out: ids"):
        median_depth_from_aux(u, aux, cdepth, out=(median, ids.float()))
    m2, i2 = median_depth_from_aux(u, aux, cdepth)   # pack_uniforms of the same camera and size beside the aux
    assert _bits(m2).tobytes() == _bits(median).tobytes() and _bits(i2).tobytes() == _bits(ids).tobytes()


# ---------------------------------------------------------------------------- 3. a silhouette
def _plane(dist, half, count, scale):
    import torch

    xs = torch.linspace(-half, half, count)
    gx, gy = torch.meshgrid(xs, xs, indexing="ij")
    n = gx.numel()
    means = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((n,), dist)], 1)
    log_scales = torch.log(torch.tensor([scale, scale, 1e-3])).repeat(n, 1)  # flat, facing the camera
    return means, log_scales


def test_silhouette_is_not_blended(dev):
    """A small opaque plate at z = 2 in front of a wall at z = 4, camera on the axis: the expected depth D / alpha takes
    values between the two along the plate's soft edge; the median depth is the depth of one of them everywhere."""
    import torch

    import brush_amd

    m1, s1 = _plane(2.0, 0.25, 5, 0.1)   # about 40 px across on the 64 x 64 image, soft edge included
    m2, s2 = _plane(4.0, 3.0, 13, 0.4)
    means, log_scales = torch.cat([m1, m2]).to(dev), torch.cat([s1, s2]).to(dev)
    n = means.shape[0]
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1).to(dev)
    splats = brush_amd.Splats(means, torch.full((n, 1, 3), 0.5, device=dev), quats, torch.full((n,), 6.0, device=dev),
                              log_scales)
    cam = brush_amd.Camera([0.0, 0.0, 0.0], [0, 0, 0, 1], 0.8, 0.8, (0.5, 0.5))
    img, depth, median, ids, _ = splats.render_median_depth(cam, (64, 64))
    median, alpha = median.cpu().numpy(), img[..., 3].cpu().numpy()
    assert (alpha > 0.9).all() and (median != 0).all()
    near2, near4 = np.abs(median - 2.0) <= 1e-4, np.abs(median - 4.0) <= 1e-4
    assert (near2 | near4).all() and near2.sum() > 100 and near4.sum() > 1000
    ids = ids.cpu().numpy()
    assert np.array_equal(near2, ids < m1.shape[0])   # the plate's splats come first
    expected = depth.cpu().numpy() / alpha
    blended = (expected > 2.2) & (expected < 3.8)
    print("plate pixels", int(near2.sum()), "blended pixels of the expected depth", int(blended.sum()))
    assert blended.sum() > 20


# ---------------------------------------------------------------------------- 4. the TSDF's metric mode
def _tsdf_inputs(dev, alpha_value):
    """Two hand-made views of a 32^3 grid: a smooth metric depth map M, a constant alpha, D = alpha M (exact for the
    alphas used: 1 and 0.5) and a premultiplied colour."""
    import torch

    import brush_amd
    from brush_amd.filter3d import view_records

    w, h = 48, 40
    views = [(brush_amd.Camera([x, 0.0, 0.0], [0, 0, 0, 1], 0.9, 0.8, (0.5, 0.5)), (w, h)) for x in (-0.2, 0.3)]
    rec = view_records(views)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    imgs, metric, accumulated = [], [], []
    for v in range(2):
        m = (2.0 + 0.4 * np.sin(0.21 * xx + v) * np.cos(0.17 * yy)).astype(np.float32)
        img = np.empty((h, w, 4), np.float32)
        img[..., :3] = alpha_value * np.stack([xx / w, yy / h, 0.5 + 0 * xx], -1)
        img[..., 3] = alpha_value
        imgs.append(torch.from_numpy(img).to(dev))
        metric.append(torch.from_numpy(m).to(dev))
        accumulated.append(torch.from_numpy((np.float32(alpha_value) * m).astype(np.float32)).to(dev))
    return rec, imgs, metric, accumulated


def _volume(dev):
    from brush_amd.tsdf import TsdfVolume

    return TsdfVolume((-0.8, -0.8, 1.2), 0.05, (32, 32, 32), device=dev)


@pytest.mark.parametrize("alpha_value", [1.0, 0.5])
def test_metric_mode_equals_accumulated_mode_where_they_must(dev, alpha_value):
    rec, imgs, metric, accumulated = _tsdf_inputs(dev, alpha_value)
    a, b = _volume(dev), _volume(dev)
    a.integrate(rec, imgs, accumulated, alpha_min=0.4)
    b.integrate(rec, imgs, metric, alpha_min=0.4, depth_kind="metric")
    assert bool((a.state[0] != 0).any()) and bool((a.state[1] < 0).any()) and bool((a.state[5] != 0).any())
    assert _bits(a.state).tobytes() == _bits(b.state).tobytes()
    if alpha_value == 0.5:  # the mode is not idle: the accumulated depth read as a distance gives another volume
        c = _volume(dev)
        c.integrate(rec, imgs, accumulated, alpha_min=0.4, depth_kind="metric")
        assert _bits(c.state).tobytes() != _bits(a.state).tobytes()
    with pytest.raises(ValueError, match="depth_kind"):
        a.integrate(rec, imgs, metric, depth_kind="median")


def test_ex_entry_with_no_flags_is_the_old_entry(dev):
    import torch

    from brush_amd import _lib

    rec, imgs, metric, accumulated = _tsdf_inputs(dev, 0.5)
    lib = _lib.lib()
    rec_dev = torch.from_numpy(np.ascontiguousarray(rec)).to(dev)
    data = (_lib.BrushTsdfViewData * 2)()
    for v in range(2):
        data[v].img, data[v].depth = imgs[v].data_ptr(), accumulated[v].data_ptr()
    old, new, bad = _volume(dev), _volume(dev), _volume(dev)
    g = old._grid()
    stream = _lib.current_stream(dev)
    assert lib.brush_tsdf_integrate(C.byref(g), old.state.data_ptr(), rec_dev.data_ptr(), data, 2, 0.4, 10.0, 0.2,
                                    stream) == 0
    assert lib.brush_tsdf_integrate_ex(C.byref(g), new.state.data_ptr(), rec_dev.data_ptr(), data, 2, 0.4, 10.0, 0.2, 0,
                                       stream) == 0
    assert lib.brush_tsdf_integrate_ex(C.byref(g), bad.state.data_ptr(), rec_dev.data_ptr(), data, 2, 0.4, 10.0, 0.2, 2,
                                       stream) == -1
    torch.cuda.synchronize()
    assert bool(old.state.any()) and _bits(old.state).tobytes() == _bits(new.state).tobytes()
    assert not bool(bad.state.any())


def test_integrate_splats_median(dev):
    import brush_amd

    splats = _scene_splats(dev)
    views = [(brush_amd.Camera([x, y, -8.0], [0, 0, 0, 1], 0.9, 0.9, (0.5, 0.5)), (64, 48))
             for x, y in ((0.0, 0.0), (0.5, -0.3), (-0.4, 0.2))]

    def volume():
        from brush_amd.tsdf import TsdfVolume

        return TsdfVolume((-4.0, -4.0, -4.0), 0.25, (32, 32, 32), device=dev)

    by_hand = volume()
    imgs, medians = [], []
    for cam, size in views:
        img, _, median, _, _ = splats.render_median_depth(cam, size, level=0.4)
        imgs.append(img)
        medians.append(median)
    by_hand.integrate(views, imgs, medians, depth_kind="metric")
    assert bool((by_hand.state[1] < 0).any())
    for k in (1, 2, 3):
        vol = volume()
        vol.integrate_splats(splats, views, depth="median", level=0.4, views_per_launch=k)
        assert vol.views == 3 and _bits(vol.state).tobytes() == _bits(by_hand.state).tobytes(), k
    expected = volume()
    expected.integrate_splats(splats, views)
    assert _bits(expected.state).tobytes() != _bits(by_hand.state).tobytes()
    with pytest.raises(ValueError, match="depth must be"):
        expected.integrate_splats(splats, views, depth="metric")


# ---------------------------------------------------------------------------- 5. command lines
def test_command_lines(dev, tmp_path):
    import torch

    import brush_amd
    from brush_amd.mesh import mesh_from_ply

    rng = np.random.default_rng(21)
    n = 3000
    means = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, (n, 4, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    raw = rng.uniform(1.0, 4.0, n).astype(np.float32)
    log_scales = np.log(rng.uniform(0.05, 0.12, (n, 3))).astype(np.float32)
    src = brush_amd.Splats(*(torch.from_numpy(a).to(dev) for a in (means, sh, quats, raw, log_scales)))
    ply = tmp_path / "cloud.ply"
    ply.write_bytes(src.to_ply())
    E.write_nerf(str(tmp_path / "nerf"), 120, 90, n_train=2, n_val=2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out, res = tmp_path / "mesh.ply", tmp_path / "mesh.json"
    r = subprocess.run([sys.executable, "-m", "brush_amd.mesh", str(ply), str(tmp_path / "nerf"), "--resolution", "32",
                        "--views", "all", "--depth", "median", "--median-level", "0.4", "--export", str(out), "--json",
                        str(res)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(res.read_text())
    mesh = mesh_from_ply(str(out))
    assert info["depth"] == "median" and info["median_level"] == 0.4 and info["num_views"] == 4
    assert info["vertices"] == len(mesh.vertices) > 0 and info["faces"] == len(mesh.faces) > 0

    r = subprocess.run([sys.executable, "-m", "brush_amd.eval", str(ply), str(tmp_path / "nerf"), "--depth-dir",
                        str(tmp_path / "depth"), "--depth-median", "--json", str(tmp_path / "eval.json")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    names = [v["name"] for v in json.loads((tmp_path / "eval.json").read_text())["views"]]
    assert len(names) == 2
    for name in names:
        stem = os.path.splitext(os.path.basename(name))[0]
        d = np.load(tmp_path / "depth" / f"{stem}_depth.npy")
        dn = np.load(tmp_path / "depth" / f"{stem}_depth_norm.npy")
        dm = np.load(tmp_path / "depth" / f"{stem}_depth_median.npy")
        assert dm.shape == (90, 120) and dm.dtype == np.float32 and d.shape == dm.shape
        assert (dm > 0).any() and ((dm[dm > 0] > 2.0) & (dm[dm > 0] < 6.5)).all()   # the cloud: 4 +- sqrt(3) away
        assert np.isfinite(dn).all() and ((dm > 0) <= (d > 0)).all()
