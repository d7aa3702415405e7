"""CPU checks of the mesh export (brush_amd/tsdf.py, brush_amd/mesh.py): the float64 reference of the extraction on an
analytic sphere (closed, oriented, genus 0, on the sphere), the reference of the fusion on the GPU test's scene (the
share of voxel / view pairs too close to a decision edge to compare), the PLY round trip, the grid helpers, the command
line's refusals and the ValueErrors."""
import math
from collections import Counter

import numpy as np
import pytest

from tests import tsdf_ref64 as R


# ---------------------------------------------------------------------------- the reference extraction
@pytest.fixture(scope="module")
def sphere():
    dims, radius, voxel, origin = (20, 18, 16), 6.0, 0.25, (-1.0, 0.5, 2.0)
    count, sdf_sum = R.sphere_field(dims, radius)
    v, c, f = R.extract(origin, voxel, count, sdf_sum)
    centre = np.array(origin) + (np.array([d - 1 for d in dims]) / 2.0 + 0.5) * voxel
    return {"v": v, "c": c, "f": f, "centre": centre, "radius": radius * voxel, "voxel": voxel}


def test_reference_sphere_is_closed_and_oriented(sphere):
    f = sphere["f"]
    assert len(f) > 500
    directed = Counter()
    for a, b, c in f:
        assert a != b and b != c and a != c
        for e in ((a, b), (b, c), (c, a)):
            directed[e] += 1
    # every edge is shared by exactly two faces, which run through it in opposite directions
    assert set(directed.values()) == {1}
    assert all((b, a) in directed for a, b in directed)
    nv, ne, nf = len(sphere["v"]), len(directed) // 2, len(f)
    assert len(np.unique(f)) == nv  # no vertex without a face
    assert nv - ne + nf == 2


def test_reference_sphere_volume_and_distance(sphere):
    v, f = sphere["v"] - sphere["centre"], sphere["f"]
    vol = np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0
    assert vol > 0  # normals point outwards, towards positive distance
    r = sphere["radius"]
    assert abs(vol - 4.0 / 3.0 * math.pi * r ** 3) < 0.05 * vol
    # linear interpolation of the distance to a sphere of radius 6 voxels along an edge of up to sqrt(3) voxels is off by
    # about L^2 / (8 R) = 3 / 48 voxel, the 1 / 32767 quantisation adds nothing visible: half a voxel holds with room
    err = np.abs(np.linalg.norm(v, axis=1) - r)
    assert err.max() <= 0.5 * sphere["voxel"], err.max()
    assert err.max() <= 0.1 * sphere["voxel"], err.max()  # what the estimate above predicts


def test_reference_table_is_consistent():
    table = R.tet_table()
    for t in range(6):
        assert table[t][0] == [] and table[t][15] == []
        for m in range(1, 15):
            assert len(table[t][m]) == (2 if bin(m).count("1") == 2 else 1)
            # the complement cuts the same edges with the opposite winding
            a = [frozenset(tri) for tri in table[t][m]]
            b = [frozenset(tri) for tri in table[t][15 - m]]
            assert set().union(*a) == set().union(*b)
    # the six tetrahedra tile the cube: every one of the 19 edges of the decomposition occurs
    edges = {e for t in range(6) for m in range(16) for tri in table[t][m] for e in tri}
    assert len(edges) == 19


def test_reference_unobserved_voxels_open_the_mesh():
    count, sdf_sum = R.sphere_field((14, 13, 12), 4.0)
    count[:, :, 7:] = 0  # nothing observed beyond x = 7: the surface ends there with a boundary
    v, _, f = R.extract((0, 0, 0), 1.0, count, sdf_sum)
    assert len(f) > 50 and v[:, 0].max() <= 6.5 + 1e-9
    directed = Counter(e for a, b, c in f for e in ((a, b), (b, c), (c, a)))
    assert any((b, a) not in directed for a, b in directed)  # boundary edges exist
    assert set(directed.values()) == {1}
    assert len(R.extract((0, 0, 0), 1.0, count, sdf_sum, min_views=4)[2]) == 0


# ---------------------------------------------------------------------------- the reference fusion
def test_fusion_case_leaves_few_pairs_out():
    """The scene of tests/test_gpu_tsdf.py, on the reference alone: at most 2 % of the voxel / view pairs lie within a
    relative 1e-5 of a decision edge, and what remains exercises every branch."""
    case = R.fusion_case()
    ref = R.integrate(case["origin"], case["voxel"], case["dims"], case["trunc"], case["records"], case["imgs"],
                      case["depths"], case["masks"], alpha_min=case["alpha_min"], max_depth=case["max_depth"],
                      near=case["near"])
    assert ref["uncertain"].mean() <= 0.02, ref["uncertain"].mean()
    per_view = ref["contrib"].sum(1)
    nvox = ref["count"].size
    assert per_view[4] == 0                      # the view that looks away
    assert 0 < per_view[3] < 0.7 * per_view[0]   # the one that sees the volume partly
    assert (per_view[:3] > 0.3 * nvox).all()
    assert ref["count"].max() == 4 and (ref["count"] == 0).any()
    assert (ref["rgb_count"] > 0).any() and (ref["rgb_count"] < ref["count"]).any()
    assert (ref["sdf_sum"] < 0).any() and (ref["sdf_sum"] == ref["count"] * R.SDF_ONE).any()
    assert (ref["rgb_sum"] <= 255 * ref["rgb_count"][:, None]).all()
    # the fused sphere is there: the reference extraction gives a surface near it
    nx, ny, nz = case["dims"]
    v, _, f = R.extract(case["origin"], case["voxel"], ref["count"].reshape(nz, ny, nx),
                        ref["sdf_sum"].reshape(nz, ny, nx), min_views=2)
    assert len(f) > 100


# ---------------------------------------------------------------------------- PLY
def test_ply_round_trip():
    from brush_amd.mesh import Mesh, mesh_from_ply, mesh_to_ply

    rng = np.random.default_rng(0)
    m = Mesh(rng.normal(size=(11, 3)).astype(np.float32), rng.integers(0, 256, (11, 3)).astype(np.uint8),
             rng.integers(0, 11, (7, 3)).astype(np.int32))
    data = mesh_to_ply(m)
    assert data.startswith(b"ply\nformat binary_little_endian 1.0\n")
    header = data[:data.index(b"end_header\n")].decode()
    assert "element vertex 11" in header and "element face 7" in header
    assert "property list uchar int vertex_indices" in header
    assert len(data) == len(header) + len("end_header\n") + 11 * 15 + 7 * 13
    back = mesh_from_ply(data)
    for a, b in ((m.vertices, back.vertices), (m.colors, back.colors), (m.faces, back.faces)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    empty = mesh_from_ply(mesh_to_ply(Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8),
                                           np.zeros((0, 3), np.int32))))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh_to_ply(Mesh(m.vertices, m.colors, np.array([[0, 1, 11]], np.int32)))
    with pytest.raises(ValueError):
        mesh_from_ply(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        mesh_from_ply(data[:-1])


def test_ply_file_round_trip(tmp_path):
    from brush_amd.mesh import mesh_from_ply, mesh_to_ply

    count, sdf_sum = R.sphere_field((9, 8, 7), 2.5)
    v, c, f = R.extract((0, 0, 0), 0.5, count, sdf_sum)
    from brush_amd.mesh import Mesh

    path = tmp_path / "m.ply"
    path.write_bytes(mesh_to_ply(Mesh(v.astype(np.float32), np.rint(c).astype(np.uint8), f.astype(np.int32))))
    back = mesh_from_ply(str(path))
    assert np.array_equal(back.faces, f) and np.array_equal(back.vertices, v.astype(np.float32))
    assert (back.colors == 128).all()  # no voxel had a colour


# ---------------------------------------------------------------------------- grid helpers
class _Cloud:
    def __init__(self, means, raw):
        import torch

        self.means, self.raw_opacity = torch.as_tensor(means), torch.as_tensor(raw)


def test_default_bounds_and_grid_for():
    from brush_amd.mesh import default_bounds, grid_for

    rng = np.random.default_rng(1)
    means = rng.uniform(-1.0, 1.0, (4000, 3)).astype(np.float32) * np.float32([2.0, 1.0, 0.5])
    raw = np.full(4000, 2.0, np.float32)
    means[:50] = 100.0   # transparent outliers are not counted
    raw[:50] = -6.0
    means[50:60] = -80.0  # opaque outliers fall outside the quantiles
    lo, hi = default_bounds(_Cloud(means, raw), pad=0.0)
    assert (np.abs(lo - [-1.96, -0.98, -0.49]) < 0.05).all() and (np.abs(hi - [1.96, 0.98, 0.49]) < 0.05).all()
    lo2, hi2 = default_bounds(_Cloud(means, raw))
    assert np.allclose(lo - lo2, 0.05 * (hi - lo).max()) and np.allclose(hi2 - hi, 0.05 * (hi - lo).max())
    with pytest.raises(ValueError):
        default_bounds(_Cloud(means, np.full(4000, -9.0, np.float32)))
    with pytest.raises(ValueError):
        default_bounds(_Cloud(means, raw), quantiles=(0.9, 0.1))

    origin, voxel, dims = grid_for(((0, 0, 0), (4, 2, 1)), resolution=64)
    assert origin == (0.0, 0.0, 0.0) and voxel == 4 / 64 and dims == (64, 32, 16)
    origin, voxel, dims = grid_for(((-1, 0, 0), (1, 0.95, 0.1)), voxel_size=0.1)
    assert origin == (-1.0, 0.0, 0.0) and voxel == 0.1 and dims == (20, 10, 1)
    for kw in ({}, {"voxel_size": 0.1, "resolution": 8}, {"voxel_size": 0.0}, {"voxel_size": float("nan")},
               {"resolution": 0}, {"resolution": 2.5}):
        with pytest.raises(ValueError):
            grid_for(((0, 0, 0), (1, 1, 1)), **kw)
    with pytest.raises(ValueError):
        grid_for(((0, 0, 0), (1, 0, 1)), resolution=8)
    with pytest.raises(ValueError, match="2048"):
        grid_for(((0, 0, 0), (1, 1, 1)), resolution=4096)
    with pytest.raises(ValueError, match=r"2\^28"):
        grid_for(((0, 0, 0), (1, 1, 1)), resolution=1024)


# ---------------------------------------------------------------------------- command line and ValueErrors
@pytest.mark.parametrize("extra, message", [
    (["--resolution", "64", "--voxel-size", "0.1"], "give one of them"),
    (["--trunc-voxels", "1.5"], "sqrt"),
    (["--alpha-min", "0"], "alpha-min"),
    (["--max-depth", "-1"], "max-depth"),
    (["--min-views", "0"], "min-views"),
    (["--bounds", "0,0,0,1,1"], "--bounds takes"),
    (["--bounds", "0,0,0,1,-1,1"], "--bounds takes"),
    (["--bounds", "0,0,0,1,1,1", "--resolution", "1024"], r"2\^28"),
    (["--bounds", "0,0,0,1,1,1", "--voxel-size", "1e-4"], "2048"),
    (["--views", "some"], "invalid choice"),
])
def test_cli_refuses_before_reading_anything(capsys, extra, message):
    import re

    from brush_amd import mesh

    with pytest.raises(SystemExit) as e:
        mesh.main(["no_such_splats.ply", "no_such_dataset"] + extra)
    assert e.value.code == 2
    assert re.search(message, capsys.readouterr().err)


def test_volume_value_errors():
    """The checks in front of the allocation (none of them needs a device)."""
    from brush_amd.tsdf import TsdfVolume, check_grid

    assert check_grid(0.5, (3, 4, 5)) == (0.5, (3, 4, 5))
    for voxel, dims in ((0.0, (4, 4, 4)), (float("inf"), (4, 4, 4)), (0.1, (4, 4)), (0.1, (0, 4, 4)),
                        (0.1, (2049, 1, 1)), (0.1, (1024, 1024, 512))):
        with pytest.raises(ValueError):
            TsdfVolume((0, 0, 0), voxel, dims)
    with pytest.raises(ValueError, match=r"2\^28"):
        TsdfVolume((0, 0, 0), 0.1, (1024, 1024, 512))
    with pytest.raises(ValueError, match="sqrt"):
        TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), trunc=0.17)
    with pytest.raises(ValueError):
        TsdfVolume((0, 0, float("nan")), 0.1, (4, 4, 4))
    with pytest.raises(ValueError):
        TsdfVolume.from_arrays((0, 0, 0), 0.1, np.zeros((4, 4)), np.zeros((4, 4)))
    with pytest.raises(ValueError):
        TsdfVolume.from_arrays((0, 0, 0), 0.1, np.zeros((4, 4, 4)), np.zeros((4, 4, 5)))
    with pytest.raises(ValueError):
        TsdfVolume.from_arrays((0, 0, 0), 0.1, np.zeros((4, 4, 4)), np.zeros((4, 4, 4)), rgb_sum=np.zeros((4, 4, 4, 3)))


def test_python_constants_are_the_headers():
    import os
    import re

    from brush_amd import tsdf

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "brush_hip.h")).read()

    def define(name):
        return eval(re.search(rf"#define {name} \(?([0-9u<> ]+?)\)?(?: /\*.*)?$", hdr, flags=re.M).group(1).replace("u", ""))

    assert define("BRUSH_TSDF_MAX_SIDE") == tsdf.MAX_SIDE and define("BRUSH_TSDF_MAX_VOXELS") == tsdf.MAX_VOXELS
    assert define("BRUSH_TSDF_PLANES") == tsdf.PLANES and define("BRUSH_TSDF_MAX_VIEWS") == tsdf.MAX_VIEWS


def test_entry_points_refuse_invalid_arguments_without_a_device():
    """Every invalid argument of the header's list returns BRUSH_ERR_INVALID_ARG before any device work."""
    import ctypes as C

    from brush_amd import _lib

    lib = _lib.lib()
    for name in ("brush_tsdf_integrate", "brush_tsdf_mesh_workspace_size", "brush_tsdf_mesh_count",
                 "brush_tsdf_mesh_emit"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)

    def grid(voxel=0.1, trunc=0.4, dims=(8, 8, 8)):
        g = _lib.BrushTsdfGrid()
        g.origin[:] = (0.0, 0.0, 0.0)
        g.voxel, g.trunc = voxel, trunc
        g.nx, g.ny, g.nz = dims
        return g

    data = (_lib.BrushTsdfViewData * 1)()
    data[0].img, data[0].depth = 4096, 8192
    fake, n = 1 << 20, C.c_size_t()
    bad_grids = [grid(voxel=0.0), grid(voxel=-1.0), grid(voxel=float("nan")), grid(voxel=float("inf")),
                 grid(trunc=0.0), grid(trunc=float("nan")), grid(dims=(0, 8, 8)), grid(dims=(2049, 1, 1)),
                 grid(dims=(1024, 1024, 257))]
    for g in bad_grids:
        assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, data, 1, 0.5, 10.0, 0.2, None) == -1
        assert lib.brush_tsdf_mesh_count(C.byref(g), fake, 2, fake, fake, 1 << 30, None) == -1
        assert lib.brush_tsdf_mesh_emit(C.byref(g), fake, 2, 1, 1, fake, fake, fake, fake, 1 << 30, None) == -1
    g = grid()
    assert lib.brush_tsdf_integrate(None, fake, fake, data, 1, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), None, fake, data, 1, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), fake, None, data, 1, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, None, 1, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, data, 0, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, data, 17, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_integrate(C.byref(g), fake + 4, fake, data, 1, 0.5, 10.0, 0.2, None) == -1
    for alpha_min, max_depth, near in ((0.0, 10.0, 0.2), (float("nan"), 10.0, 0.2), (0.5, 0.0, 0.2),
                                       (0.5, float("nan"), 0.2), (0.5, 10.0, -1.0), (0.5, 10.0, float("inf"))):
        assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, data, 1, alpha_min, max_depth, near, None) == -1
    null_img = (_lib.BrushTsdfViewData * 1)()
    null_img[0].depth = 8192
    assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, null_img, 1, 0.5, 10.0, 0.2, None) == -1
    assert lib.brush_tsdf_mesh_workspace_size(8, 8, 8, C.byref(n)) == 0 and n.value >= 8 * 8 * 8 * 13
    assert lib.brush_tsdf_mesh_workspace_size(8, 8, 8, None) == -1
    assert lib.brush_tsdf_mesh_workspace_size(4096, 1, 1, C.byref(n)) == -1
    assert lib.brush_tsdf_mesh_count(C.byref(g), None, 2, fake, fake, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_count(C.byref(g), fake, 0, fake, fake, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_count(C.byref(g), fake, 2, None, fake, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_count(C.byref(g), fake, 2, fake, None, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_count(C.byref(g), fake, 2, fake, fake, 16, None) == -2  # workspace too small
    assert lib.brush_tsdf_mesh_emit(C.byref(g), fake, 2, 1, 0, None, fake, None, fake, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_emit(C.byref(g), fake, 2, 0, 1, None, None, None, fake, 1 << 30, None) == -1
    assert lib.brush_tsdf_mesh_emit(C.byref(g), fake, 2, 1, 1, fake, fake, fake, fake, 16, None) == -2
