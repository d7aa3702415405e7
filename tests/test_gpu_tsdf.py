"""GPU checks of the mesh export (brush_tsdf_integrate / brush_tsdf_mesh_count / brush_tsdf_mesh_emit, TsdfVolume,
`python -m brush_amd.mesh`) against the float64 restatement in tests/tsdf_ref64.py: the fusion on synthetic sphere depth
maps (no rendering), its invariances (view order, views per launch, launch shape, run to run), the extraction from
given volumes, exactly in the faces, and the whole path on a wall of splats at a known depth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as E
from tests import tsdf_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    return torch.device("cuda:0")


# ---------------------------------------------------------------------------- 1. fusion against the reference
@pytest.fixture(scope="module")
def case():
    c = R.fusion_case()
    c["ref"] = R.integrate(c["origin"], c["voxel"], c["dims"], c["trunc"], c["records"], c["imgs"], c["depths"],
                           c["masks"], alpha_min=c["alpha_min"], max_depth=c["max_depth"], near=c["near"])
    return c


def _fuse(dev, c, order=None, per_launch=None, dims=None, origin=None):
    """The volume's planes [6, nvox] on the host after fusing the case's views in `order`, `per_launch` at a time."""
    import torch

    from brush_amd.tsdf import TsdfVolume

    order = list(range(len(c["imgs"]))) if order is None else list(order)
    per_launch = len(order) if per_launch is None else per_launch
    vol = TsdfVolume(c["origin"] if origin is None else origin, c["voxel"], c["dims"] if dims is None else dims,
                     trunc=c["trunc"], device=dev)
    imgs = [torch.from_numpy(c["imgs"][v]).to(dev) for v in order]
    depths = [torch.from_numpy(c["depths"][v]).to(dev) for v in order]
    masks = [None if c["masks"][v] is None else torch.from_numpy(c["masks"][v]).to(dev) for v in order]
    for base in range(0, len(order), per_launch):
        sl = slice(base, base + per_launch)
        vol.integrate(np.ascontiguousarray(c["records"][order[sl]]), imgs[sl], depths[sl], masks=masks[sl],
                      alpha_min=c["alpha_min"], max_depth=c["max_depth"], near=c["near"])
    torch.cuda.synchronize()
    return vol, vol.state.cpu().numpy()


@pytest.fixture(scope="module")
def fused(dev, case):
    return _fuse(dev, case)


def test_fusion_matches_reference(case, fused):
    ref = case["ref"]
    _, planes = fused
    left_out = ref["uncertain"]
    assert left_out.mean() <= 0.02, left_out.mean()
    keep = ~left_out.any(0)  # voxels none of whose pairs is left out: their sums are comparable as a whole
    assert keep.mean() >= 0.95
    count, sdf_sum = planes[0].view(np.uint32).astype(np.int64), planes[1].astype(np.int64)
    rgb_sum, rgb_count = planes[2:5].view(np.uint32).astype(np.int64).T, planes[5].view(np.uint32).astype(np.int64)
    d_sdf = np.abs(sdf_sum - ref["sdf_sum"])[keep]
    d_rgb = np.abs(rgb_sum - ref["rgb_sum"])[keep]
    print("pairs left out", left_out.mean(), "voxels compared", keep.mean(), "max |d sdf_sum|", d_sdf.max(),
          "max |d rgb_sum|", d_rgb.max(), "count != ref", int((count != ref["count"])[keep].sum()))
    assert np.array_equal(count[keep], ref["count"][keep])
    assert np.array_equal(rgb_count[keep], ref["rgb_count"][keep])
    # one rounding unit per contributing view: each term is rint of a value whose f32 error is far below one unit
    assert (d_sdf <= ref["count"][keep]).all(), d_sdf.max()
    assert (d_rgb <= ref["rgb_count"][keep][:, None]).all(), d_rgb.max()
    # the bound is not idle: most sums agree exactly
    assert (d_sdf == 0).mean() > 0.9 and (d_rgb == 0).mean() > 0.9


def test_read_returns_the_state(case, fused):
    vol, planes = fused
    nx, ny, nz = case["dims"]
    a = vol.read()
    assert a.count.shape == (nz, ny, nx) and a.count.dtype == np.uint32 and a.sdf_sum.dtype == np.int32
    assert np.array_equal(a.count.reshape(-1), planes[0].view(np.uint32))
    assert np.array_equal(a.sdf_sum.reshape(-1), planes[1])
    seen = a.count > 0
    assert np.isnan(a.sdf[~seen]).all() and (np.abs(a.sdf[seen]) <= 1.0).all() and a.sdf.dtype == np.float32
    assert a.rgb.shape == (nz, ny, nx, 3) and a.rgb.dtype == np.uint8
    has = a.rgb_count > 0
    assert has.any() and (a.rgb[~has] == 0).all()
    assert np.array_equal(a.rgb[has], np.rint(a.rgb_sum[has] / a.rgb_count[has][:, None]).astype(np.uint8))


# ---------------------------------------------------------------------------- 2. invariance
def test_view_order_does_not_change_a_bit(dev, case, fused):
    for order in ([4, 2, 0, 3, 1], [1, 0, 4, 3, 2]):
        assert _fuse(dev, case, order=order)[1].tobytes() == fused[1].tobytes()


@pytest.mark.parametrize("per_launch", [1, 2])
def test_views_per_launch_do_not_change_a_bit(dev, case, fused, per_launch):
    assert _fuse(dev, case, per_launch=per_launch)[1].tobytes() == fused[1].tobytes()


def test_two_runs_are_bitwise_equal(dev, case, fused):
    assert _fuse(dev, case)[1].tobytes() == fused[1].tobytes()


def test_launch_shape_does_not_change_a_bit(dev, case):
    """The same voxel centres inside grids of other x sides (none a multiple of 64, one wider than a workgroup's 256
    lanes, one with workgroups that straddle rows): a voxel's words do not depend on where in the launch it sits."""
    nx, ny, nz = 24, 5, 3
    origin = (case["origin"][0], -0.27, -0.13)  # a slab through the sphere
    _, base = _fuse(dev, case, dims=(nx, ny, nz), origin=origin)
    base = base.reshape(6, nz, ny, nx)
    for wide in (37, 300):
        _, planes = _fuse(dev, case, dims=(wide, ny, nz), origin=origin)
        planes = planes.reshape(6, nz, ny, wide)
        assert np.array_equal(planes[..., :nx], base)
    assert base[0].any() and (base[1] < 0).any()


# ---------------------------------------------------------------------------- 3. extraction
def _colour_field(count, seed):
    rng = np.random.default_rng(seed)
    rgb_count = rng.integers(0, 4, count.shape) * (count > 0)
    rgb_sum = rng.integers(0, 256, count.shape + (3,)) * rgb_count[..., None]
    return rgb_sum, rgb_count


def _ulp32(x):
    x = np.abs(x.astype(np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("kind", ["sphere", "cut"])
def test_extraction_matches_reference(dev, kind):
    from brush_amd.tsdf import TsdfVolume

    dims, origin, voxel = (20, 18, 16), (0.3, 0.2, 0.1), 0.1
    count, sdf_sum = R.sphere_field(dims, 6.0, centre=(9.3, 8.6, 7.4))
    if kind == "cut":  # unobserved voxels cutting through the sphere, and a band seen by one view only
        count[:, :, 11:] = 0
        count[5:7, :, :] = 1
        sdf_sum[5:7, :, :] //= 3
        count[9, 9, 3:6] = 0
    rgb_sum, rgb_count = _colour_field(count, 3)
    vol = TsdfVolume.from_arrays(origin, voxel, count, sdf_sum, rgb_sum, rgb_count, device=dev)
    mesh = vol.extract_mesh(min_views=2)
    v, c, f = R.extract(origin, voxel, count, sdf_sum, rgb_sum, rgb_count, min_views=2)
    assert len(f) > 300 and mesh.faces.dtype == np.int32 and mesh.vertices.dtype == np.float32
    assert mesh.colors.dtype == np.uint8
    assert mesh.faces.shape == f.shape and np.array_equal(mesh.faces, f)
    assert mesh.vertices.shape == v.shape
    want = v.astype(np.float32)
    err = np.abs(mesh.vertices.astype(np.float64) - want.astype(np.float64)) / _ulp32(want)
    print(kind, "V", len(v), "F", len(f), "max vertex error in ulp", err.max(), "max colour error",
          np.abs(mesh.colors - c).max())
    assert err.max() <= 2.0, err.max()
    assert np.abs(mesh.colors.astype(np.float64) - c).max() <= 1.0
    again = vol.extract_mesh(min_views=2)
    assert again.vertices.tobytes() == mesh.vertices.tobytes() and again.faces.tobytes() == mesh.faces.tobytes()
    assert again.colors.tobytes() == mesh.colors.tobytes()


def test_extraction_without_colours_is_grey(dev):
    from brush_amd.tsdf import TsdfVolume

    count, sdf_sum = R.sphere_field((9, 8, 7), 2.5)
    mesh = TsdfVolume.from_arrays((0, 0, 0), 0.5, count, sdf_sum, device=dev).extract_mesh()
    assert len(mesh.faces) > 20 and (mesh.colors == 128).all()


def test_degenerate_volumes(dev):
    from brush_amd.tsdf import TsdfVolume

    def shapes(m):
        return m.vertices.shape, m.colors.shape, m.faces.shape

    # 2 x 2 x 2: one cell, corner 0 alone inside: 7 active edges, and the 6 tetrahedra give one triangle each
    count = np.full((2, 2, 2), 2)
    sdf_sum = np.full((2, 2, 2), 2 * 9000)
    sdf_sum[0, 0, 0] = -2 * 9000
    mesh = TsdfVolume.from_arrays((0, 0, 0), 1.0, count, sdf_sum, device=dev).extract_mesh()
    v, _, f = R.extract((0, 0, 0), 1.0, count, sdf_sum)
    assert shapes(mesh) == ((7, 3), (7, 3), (6, 3)) and np.array_equal(mesh.faces, f)
    assert np.abs(mesh.vertices - v).max() <= 1e-6
    # one voxel: no edge at all
    one = TsdfVolume.from_arrays((0, 0, 0), 1.0, np.full((1, 1, 1), 5), np.full((1, 1, 1), -7), device=dev)
    assert shapes(one.extract_mesh()) == ((0, 3), (0, 3), (0, 3))
    # everything outside, everything inside, a fresh volume
    count, sdf_sum = np.full((5, 6, 7), 3), np.full((5, 6, 7), 3 * R.SDF_ONE)
    for s in (sdf_sum, -sdf_sum, 0 * sdf_sum):
        assert shapes(TsdfVolume.from_arrays((0, 0, 0), 1.0, count, s, device=dev).extract_mesh()) == \
            ((0, 3), (0, 3), (0, 3))
    assert shapes(TsdfVolume((0, 0, 0), 1.0, (7, 6, 5), device=dev).extract_mesh()) == ((0, 3), (0, 3), (0, 3))
    # min_views above every count
    count, sdf_sum = R.sphere_field((9, 8, 7), 2.5)
    vol = TsdfVolume.from_arrays((0, 0, 0), 1.0, count, sdf_sum, device=dev)
    assert len(vol.extract_mesh(min_views=3).faces) > 0
    assert shapes(vol.extract_mesh(min_views=4)) == ((0, 3), (0, 3), (0, 3))
    with pytest.raises(ValueError):
        vol.extract_mesh(min_views=0)


def test_invalid_arguments(dev, case):
    import ctypes as C

    import torch

    from brush_amd import _lib
    from brush_amd.tsdf import TsdfVolume

    vol = TsdfVolume((0, 0, 0), 0.1, (8, 8, 8), device=dev)
    img, depth = torch.zeros((45, 67, 4), device=dev), torch.zeros((45, 67), device=dev)
    rec = case["records"][:1]
    for kw in ({"alpha_min": 0.0}, {"alpha_min": float("nan")}, {"max_depth": 0.0}, {"near": -1.0}):
        with pytest.raises(ValueError):
            vol.integrate(rec, [img], [depth], **kw)
    with pytest.raises(ValueError):
        vol.integrate(rec, [img[:, :60]], [depth])            # not the record's size
    with pytest.raises(ValueError):
        vol.integrate(rec, [img], [depth.double()])
    with pytest.raises(ValueError):
        vol.integrate(rec, [img], [depth], masks=[depth])     # a float mask
    with pytest.raises(ValueError):
        vol.integrate(rec, [img, img], [depth])
    with pytest.raises(ValueError):
        vol.integrate_splats(None, [], views_per_launch=17)
    # the C entry points, with real device pointers: nothing may be launched, the volume stays zero
    lib, g = _lib.lib(), vol._grid()
    data = (_lib.BrushTsdfViewData * 1)()
    data[0].img, data[0].depth = img.data_ptr(), depth.data_ptr()
    rec_dev = torch.from_numpy(rec.copy()).to(dev)
    args = (vol.state.data_ptr(), rec_dev.data_ptr(), data)
    assert lib.brush_tsdf_integrate(C.byref(g), *args, 0, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), *args, 17, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), *args, 1, -0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), vol.state.data_ptr(), None, data, 1, 0.5, 10.0, 0.2, None) == -1
    g.voxel = float("nan")
    assert lib.brush_tsdf_integrate(C.byref(g), *args, 1, 0.5, 10.0, 0.2, None) == -1
    g = vol._grid()
    g.nx = 4096
    assert lib.brush_tsdf_integrate(C.byref(g), *args, 1, 0.5, 10.0, 0.2, None) == -1
    torch.cuda.synchronize()
    assert not bool(vol.state.any())


# ---------------------------------------------------------------------------- 4. end to end
def _wall(dev, dist):
    import torch

    import brush_amd

    xs = torch.linspace(-3.0, 3.0, 25)
    gx, gy = torch.meshgrid(xs, xs, indexing="ij")
    n = gx.numel()
    means = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((n,), dist)], 1).to(dev)
    log_scales = torch.log(torch.tensor([0.4, 0.4, 1e-3])).repeat(n, 1).to(dev)  # flat, facing the cameras
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1).to(dev)
    sh = torch.full((n, 1, 3), 0.5, device=dev)
    raw = torch.full((n,), 6.0, device=dev)
    return brush_amd.Splats(means, sh, quats, raw, log_scales)


def test_wall_of_splats_becomes_a_plane(dev):
    import brush_amd
    from brush_amd.tsdf import TsdfVolume

    dist, voxel = 4.0, 0.05
    splats = _wall(dev, dist)
    views = [(brush_amd.Camera([x, y, 0.0], [0, 0, 0, 1], 0.8, 0.8, (0.5, 0.5)), (96, 96))
             for x, y in ((0.0, 0.0), (0.35, -0.2), (-0.3, 0.25))]
    vol = TsdfVolume((-1.0, -1.0, dist - 0.5), voxel, (40, 40, 20), device=dev)
    vol.integrate_splats(splats, views, views_per_launch=2)
    assert vol.views == 3
    other = TsdfVolume((-1.0, -1.0, dist - 0.5), voxel, (40, 40, 20), device=dev)
    other.integrate_splats(splats, views[::-1], views_per_launch=3)
    assert bool((other.state == vol.state).all())
    a = vol.read()
    assert (a.count[:12] == 3).all()                 # free space in front of the wall: carved by every view
    assert (a.sdf[:5] == 1.0).all()
    assert (a.count[16:] == 0).all()                 # more than trunc = 4 voxels behind it: never observed
    mesh = vol.extract_mesh(min_views=2)
    assert len(mesh.faces) >= 2 * 39 * 39
    assert np.abs(mesh.vertices[:, 2] - dist).max() <= 0.5 * voxel, np.abs(mesh.vertices[:, 2] - dist).max()
    p = mesh.vertices[mesh.faces].astype(np.float64)
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (normals[:, 2] < 0).all()                 # at the cameras, which sit at z = 0
    # the wall's colour: SH degree 0, C0 * 0.5 + 0.5
    want = 255.0 * (0.2820947917738781 * 0.5 + 0.5)
    assert np.abs(mesh.colors.astype(np.float64) - want).max() <= 2.0


def test_mesh_cli(dev, tmp_path):
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
    E.write_nerf(str(tmp_path / "nerf"), 120, 90, n_train=4, n_val=2)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out, res = tmp_path / "mesh.ply", tmp_path / "mesh.json"
    r = subprocess.run([sys.executable, "-m", "brush_amd.mesh", str(ply), str(tmp_path / "nerf"), "--resolution", "40",
                        "--views", "all", "--min-views", "2", "--export", str(out), "--json", str(res)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(res.read_text())
    mesh = mesh_from_ply(str(out))
    assert info["num_views"] == 6 and max(info["grid"]["dims"]) == 40
    assert info["grid"]["bytes"] == 24 * int(np.prod(info["grid"]["dims"]))
    assert info["vertices"] == len(mesh.vertices) > 0 and info["faces"] == len(mesh.faces) > 0
    assert 0.0 < info["observed_fraction"] <= 1.0
    assert mesh.faces.min() >= 0 and mesh.faces.max() < len(mesh.vertices)
    lo, hi = np.array(info["grid"]["origin"]), np.array(info["grid"]["origin"]) + info["grid"]["voxel_size"] * \
        np.array(info["grid"]["dims"])
    assert (mesh.vertices >= lo - 1e-5).all() and (mesh.vertices <= hi + 1e-5).all()
    for word in ("grid\t", "views\t6 all", "observed\t", f"mesh\tV {len(mesh.vertices)}\tF {len(mesh.faces)}"):
        assert word in r.stdout, r.stdout
