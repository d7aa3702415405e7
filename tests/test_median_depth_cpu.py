"""CPU-side checks of the median depth: the float64 reference checks itself (the exact ties, the batch-boundary cases,
the cap on undecided pixels, a float32 restatement inside the gate, wrong references rejected), the new cases are
threshold-free, the pure-Python layer (levels, depth kinds, both command lines), and the library: argument validation of
brush_render_median_depth and brush_tsdf_integrate_ex without a device, and the resources of k_median_depth_quad."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import contrib_ref64 as CR
from tests import helpers as H
from tests import median_cases as MC
from tests import median_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = MC.case_level_params()
CAP = 0.02  # undecided pixels per (case, level)


@pytest.fixture(scope="module")
def refs():
    """One reference walk per (case, level), shared and left unchanged."""
    return {MC.param_id(p): R.walk(p[0], p[1]) for p in PARAMS}


@pytest.fixture(scope="module")
def emus():
    return {MC.param_id(p): R.emulate32(p[0], p[1]) for p in PARAMS}


# ---------------------------------------------------------------------------- the cases and the reference
def test_case_list():
    names = [c["name"] for c, _ in MC.all_cases()]
    assert len(set(names)) == len(names)
    for name in ("exact_half", "exact_half_below", "cross_at_64", "cross_at_65", "stop_before_crossing", "batch_129",
                 "ragged_17x9", "random_200", "quadrant_skip", "exact_pair", "empty"):
        assert name in names
    assert len(PARAMS) == 3 * (len(names) - 1) + 1
    for c, _ in MC.all_cases():
        m = c["num_visible"]
        assert c["z"].dtype == np.float32 and len(np.unique(c["z"][:m])) == m


def test_new_cases_are_threshold_free():
    """No alpha test, sigma test or stop test of a new case lies within 8 allowances of its threshold (the cases of
    contrib_cases are held to that by tests/test_contribution_cpu.py): only the level test can be undecided."""
    for c in MC.new_cases() + [MC.stop_before_crossing()]:
        d = CR.decisions(c)
        print(f"{c['name']}: {d.size} decisions, nearest {float(d.min()):.3g} allowances")
        assert float(d.min()) > 8.0, c["name"]


def test_undecided_pixels_are_capped(refs):
    for p in PARAMS:
        r = refs[MC.param_id(p)]
        frac = float(r["undecided"].mean())
        print(f"{MC.param_id(p)}: undecided {int(r['undecided'].sum())} of {r['undecided'].size}, "
              f"with a median {int((r['id'] >= 0).sum())}")
        assert frac <= CAP, (MC.param_id(p), frac)
        assert (r["pos_lo"] <= r["pos"]).all() and (r["pos"] <= r["pos_hi"]).all()


def test_exact_ties_pin_the_comparison(refs):
    """next_T == t_level exactly, on exactly computed values: `<=` makes that entry the median, and the pixel is decided."""
    for key, (y, x), want in (("exact_half-0.5", (8, 8), 0), ("quadrant_skip-0.5", (3, 3), 0),
                              ("exact_pair-0.25", (8, 8), 0)):
        r = refs[key]
        assert int(r["pos"][y, x]) == want and not r["undecided"][y, x], key
    c = MC.exact_half()
    r = refs["exact_half-0.5"]
    assert int(r["id"][8, 8]) == 0 and r["depth"][8, 8] == c["z"][0]
    assert int(R.walk(c, 0.5, mutate="lt")["pos"][8, 8]) == 1
    # One ulp less opacity: in float64 next_T = 0.5 + 2^-25 > 0.5 and record 1 is the median.  (float32 rounds
    # 1 - alpha to 0.5, ties to even, and picks record 0: the pixel is undecided, as it must be.)
    r = refs["exact_half_below-0.5"]
    assert int(r["pos"][8, 8]) == 1 and r["undecided"][8, 8]
    assert int(r["pos_lo"][8, 8]) == 0 and int(r["pos_hi"][8, 8]) == 1


def test_crossing_on_either_side_of_a_batch(refs):
    for position in (64, 65):
        c = MC.cross_at(position)
        assert c["num_isect"] == position + 20
        r = refs[f"cross_at_{position}-0.5"]   # T = 0.995^(position - 1) ~ 0.73, then 0.29: the 0.6 record crosses 0.5
        assert (r["pos"] == position - 1).all() and not r["undecided"].any()
        assert (r["depth"] == c["z"][position - 1]).all()
        # level 0.25 is crossed by the flat records alone (0.995^58 < 0.75), level 0.75 only behind the 0.6 record
        assert (refs[f"cross_at_{position}-0.25"]["pos"] == 57).all()
        assert (refs[f"cross_at_{position}-0.75"]["pos"] > position - 1).all()


def test_a_stopping_entry_is_never_the_median(refs):
    r = refs[f"stop_before_crossing-{MC.STOP_LEVEL:g}"]
    none = r["id"] < 0
    assert 40 < int(none.sum()) < 120 and none[8, 8] and not none[0, 0]   # within ~5 px of (8, 8)
    assert (r["id"][~none] == 1).all()   # further out the second record (global id 1) is added and crosses
    wrong = R.walk(MC.stop_before_crossing(), MC.STOP_LEVEL, mutate="stop_counts")
    assert (wrong["id"] == 1).all()


def test_float32_restatement_passes_the_gate(refs, emus):
    for p in PARAMS:
        key = MC.param_id(p)
        g = R.gate(p[0], *emus[key], refs[key])
        assert g["ok"], (key, g)


def test_each_wrong_reference_is_rejected_somewhere(emus):
    for m in R.MUTATIONS:
        rejected = [MC.param_id(p) for p in PARAMS
                    if not R.gate(p[0], *emus[MC.param_id(p)], R.walk(p[0], p[1], mutate=m))["ok"]]
        print(m, "rejected on", rejected)
        assert rejected, m
    assert not R.gate(MC.exact_half(), *emus["exact_half-0.5"], R.walk(MC.exact_half(), 0.5, mutate="lt"))["ok"]
    key = f"stop_before_crossing-{MC.STOP_LEVEL:g}"
    assert not R.gate(MC.stop_before_crossing(), *emus[key],
                      R.walk(MC.stop_before_crossing(), MC.STOP_LEVEL, mutate="stop_counts"))["ok"]


def test_gate_checks_every_pixel(refs, emus):
    """A single wrong pixel fails the gate, whether it is decided or not; so does an id that is not in the tile's list."""
    c = MC.with_z(CC.random_case())
    ref = refs["random_200-0.5"]
    ids, depth = (a.copy() for a in emus["random_200-0.5"])
    y, x = np.argwhere(ref["id"] >= 0)[0]
    for bad_id, bad_depth in ((-1, 0.0), (int(ids[y, x]), 0.0), (c["n"] - 1, float(depth[y, x]))):
        i2, d2 = ids.copy(), depth.copy()
        i2[y, x], d2[y, x] = bad_id, bad_depth
        assert not R.gate(c, i2, d2, ref)["ok"]
    und = R.walk(MC.exact_half_below(), 0.5)
    ids, depth = R.emulate32(MC.exact_half_below(), 0.5)
    assert und["undecided"][8, 8] and R.gate(MC.exact_half_below(), ids, depth, und)["ok"]
    ids[8, 8] = -1
    depth[8, 8] = 0.0
    assert not R.gate(MC.exact_half_below(), ids, depth, und)["ok"]


# ---------------------------------------------------------------------------- the rendered scene, lists from the CPU oracle
def oracle_case(w, h):
    from oracle import oracle as O

    s = MC.rendered_scene()
    u = H.reference_test_uniforms(w, h, 0)
    _, aux = O.render_forward(u, s["means"], s["log_scales"], s["quats"], s["sh"], s["raw_opacity"])
    m = u["viewmat"].astype(np.float32)
    z_global = (m[2] * s["means"][:, 0] + m[6] * s["means"][:, 1] + m[10] * s["means"][:, 2] + m[14]).astype(np.float32)
    nv = int(aux["num_visible"][0])
    z = np.full(MC.SCENE_N, np.nan, np.float32)
    z[:nv] = z_global[aux["global_from_compact_gid"][:nv]]
    return MC.case_from_aux(f"scene_{w}x{h}", w, h, MC.SCENE_N, aux["projected_splats"], aux["tile_bins"],
                            aux["compact_gid_from_isect"], aux["global_from_compact_gid"], nv, z)


@pytest.mark.parametrize("size", MC.SCENE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rendered_scene_is_inside_the_cap(size):
    c = oracle_case(*size)
    assert c["num_visible"] > 100
    for level in MC.LEVELS:
        r = R.walk(c, level)
        with_median = float((r["id"] >= 0).mean())
        print(f"{c['name']} level {level}: undecided {int(r['undecided'].sum())} of {r['undecided'].size}, "
              f"with a median {with_median:.3f}")
        assert float(r["undecided"].mean()) <= CAP
        if size == (64, 64) and level == 0.5:
            assert 0.2 < with_median < 1.0   # the scene has both kinds of pixels
        assert R.gate(c, *R.emulate32(c, level), r)["ok"]


# ---------------------------------------------------------------------------- the pure-Python layer
def test_level_and_kind_value_errors():
    from brush_amd.median_depth import check_level
    from brush_amd.tsdf import TsdfVolume, _depth_kind_flags

    assert check_level(0.5) == 0.5 and check_level(np.float32(0.25)) == 0.25
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), None, "half"):
        with pytest.raises(ValueError, match="level must be finite with 0 < level < 1"):
            check_level(bad)
    assert _depth_kind_flags("accumulated") == 0 and _depth_kind_flags("metric") == 1
    with pytest.raises(ValueError, match="depth_kind must be 'accumulated' or 'metric'"):
        _depth_kind_flags("median")
    # refused before the volume or a device is touched
    with pytest.raises(ValueError, match="depth_kind"):
        TsdfVolume.integrate(None, np.zeros((0, 24), np.float32), [], [], depth_kind="expected")
    with pytest.raises(ValueError, match="depth must be 'expected' or 'median'"):
        TsdfVolume.integrate_splats(None, None, [], depth="metric")
    with pytest.raises(ValueError, match="level must be"):
        TsdfVolume.integrate_splats(None, None, [], depth="median", level=1.0)


def test_exports():
    import brush_amd
    from brush_amd import median_depth

    assert brush_amd.render_median_depth is median_depth.render_median_depth
    assert brush_amd.median_depth_from_aux is median_depth.median_depth_from_aux
    assert hasattr(brush_amd.Splats, "render_median_depth")
    assert "not differentiable" in median_depth.__doc__.lower()


def test_both_parsers(capsys, tmp_path):
    from brush_amd import eval as E
    from brush_amd import mesh

    a = mesh.parser().parse_args(["in.ply", "scene"])
    assert a.depth == "expected" and a.median_level == 0.5
    mesh.plan_from_args(a)
    a = mesh.parser().parse_args(["in.ply", "scene", "--depth", "median", "--median-level", "0.4"])
    assert a.depth == "median" and a.median_level == 0.4
    mesh.plan_from_args(a)
    for bad in ("0", "1", "-0.5", "nan", "inf"):
        with pytest.raises(ValueError, match="--median-level"):
            mesh.plan_from_args(mesh.parser().parse_args(["a", "b", "--median-level", bad]))
    missing = str(tmp_path / "missing")  # nothing is read: the parser refuses first
    for argv in ([missing, missing, "--depth", "mean"], [missing, missing, "--median-level", "1.0"],
                 [missing, missing, "--depth", "median", "--median-level", "x"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(argv)
        assert e.value.code == 2
    a = E.parser().parse_args(["in.ply", "scene", "--depth-dir", "d", "--depth-median"])
    assert a.depth_median and a.depth_dir == "d"
    assert not E.parser().parse_args(["in.ply", "scene", "--depth-dir", "d"]).depth_median
    with pytest.raises(SystemExit) as e:
        E.main([missing, missing, "--depth-median"])   # needs --depth-dir
    assert e.value.code == 2
    assert "--depth-median needs --depth-dir" in capsys.readouterr().err


# ---------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_median_entry_validates_before_any_device_work(lib):
    from brush_amd import _lib

    u = _lib.BrushUniforms()
    u.img_size[:] = [17, 9]
    u.tile_bounds[:] = [2, 1]
    aux = _lib.BrushAux()
    fake = 0x1000  # never dereferenced on the host: every call below is refused before a launch
    needed = ("projected_splats", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid", "num_visible")
    for name in needed:
        setattr(aux, name, fake)
    aux.max_intersects = 8
    call = lib.brush_render_median_depth
    ok_args = [C.byref(u), C.byref(aux), fake, 0.5, fake, fake, 4, None]
    for i in (0, 1, 2, 4):  # uniforms, aux, compact_depth, out_depth
        args = list(ok_args)
        args[i] = None
        assert call(*args) == -1, i
    for level in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf"), float("-inf")):
        args = list(ok_args)
        args[3] = level
        assert call(*args) == -1, level
    for i in (2, 4, 5):  # 4-byte alignment of compact_depth, out_depth, out_id
        args = list(ok_args)
        args[i] = fake + 2
        assert call(*args) == -1, i
    for name in needed:
        setattr(aux, name, None)
        assert call(*ok_args) == -1, name
        setattr(aux, name, fake)
    aux.max_intersects = 0
    assert call(*ok_args) == -1
    aux.max_intersects = 8
    u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
    assert call(*ok_args) == -1
    u.tile_bounds[:] = [2, 1]
    u.img_size[:] = [0, 9]
    assert call(*ok_args) == -1


def test_tsdf_ex_entry_validates_before_any_device_work(lib):
    from brush_amd import _lib

    g = _lib.BrushTsdfGrid()
    g.origin[:] = [0.0, 0.0, 0.0]
    g.voxel, g.trunc = 0.1, 0.4
    g.nx, g.ny, g.nz = 8, 8, 8
    fake = 0x1000
    data = (_lib.BrushTsdfViewData * 1)()
    data[0].img, data[0].depth = fake, fake
    call = lib.brush_tsdf_integrate_ex
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):  # unknown bits, with or without the known one
        assert call(C.byref(g), fake, fake, data, 1, 0.5, 10.0, 0.2, flags, None) == -1, flags
    for flags in (0, _lib.TSDF_DEPTH_METRIC):  # the other refusals hold in both modes
        assert call(C.byref(g), fake, fake, data, 0, 0.5, 10.0, 0.2, flags, None) == -1
        assert call(C.byref(g), fake, fake, data, 17, 0.5, 10.0, 0.2, flags, None) == -1
        assert call(C.byref(g), fake, fake, data, 1, -0.5, 10.0, 0.2, flags, None) == -1
        assert call(C.byref(g), None, fake, data, 1, 0.5, 10.0, 0.2, flags, None) == -1
        assert call(C.byref(g), fake + 4, fake, data, 1, 0.5, 10.0, 0.2, flags, None) == -1
        data[0].depth = None
        assert call(C.byref(g), fake, fake, data, 1, 0.5, 10.0, 0.2, flags, None) == -1
        data[0].depth = fake
    assert lib.brush_tsdf_integrate(C.byref(g), fake, fake, data, 0, 0.5, 10.0, 0.2, None) == -1


def test_median_kernel_static_lds_and_no_spills(lib):
    """One kernel, no spills, no scratch, and the static LDS the .hip pins with a static_assert: 4 waves x 64 records x
    32 bytes.  The TSDF fusion has its two instantiations."""
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_median_depth_quad")
    assert len(res) == 1, sorted(res)
    (name, r), = res.items()
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name
    assert r["group_segment_fixed_size"] == 8192, name
    src = open(os.path.join(ROOT, "brush_amd", "csrc", "median_depth.hip")).read()
    walk = open(os.path.join(ROOT, "brush_amd", "csrc", "replay_walk.hpp")).read()  # the staged record is the shared walk's
    assert "static_assert(sizeof(ReplayRec) * kTilesPerBlock * kBatch == 8192" in walk
    assert "s_barrier" not in src.split("#include")[1] and "atomic" not in src.split("#include")[1]
    # the loop the kernel runs is the shared walk's: its code (comments cut) has neither as well
    code = re.sub(r"/\*.*?\*/", "", "\n".join(l.split("//")[0] for l in walk.split("#pragma once")[1].splitlines()))
    assert "s_barrier" not in code and "atomic" not in code
    assert len(kd.resources(_lib.LIB_PATH, r"k_tsdf_integrate")) == 2
