"""CPU-side checks of error-driven densification: densify_candidates, the revised-opacity formula, the configuration's
refusals and the command line, the float64 reference of the error replay checking itself (a float32 restatement inside
the allowance, wrong references rejected), and the library: argument validation of the two entries and the resources of
their kernels."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import contrib_ref64
from tests import error_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- densify_candidates
def _cand(scores, n, thresh, growth, max_splats=None):
    import torch

    from brush_amd.train import densify_candidates

    return densify_candidates(torch.tensor(scores, dtype=torch.float32), n, thresh, growth, max_splats).tolist()


def test_threshold_edge():
    assert _cand([0.99999994, 1.0, 1.0000001, 0.0], 4, 1.0, 1.0) == [False, True, True, False]
    assert _cand([0.0, 0.0], 2, 0.0, 1.0) == [True, True]  # == passes at a zero threshold too


def test_growth_cap_keeps_the_largest_ties_to_the_lower_index():
    s = [2.0, 5.0, 2.0, 0.5, 3.0, 2.0, 2.0, 9.0, 0.1, 2.0]
    assert _cand(s, 10, 1.0, 1.0) == [True, True, True, False, True, True, True, True, False, True]
    assert _cand(s, 10, 1.0, 0.3) == [False, True, False, False, True, False, False, True, False, False]  # ceil(3.0) = 3
    # ceil(0.31 * 10) = 4: the first of the five tied 2.0s joins
    assert _cand(s, 10, 1.0, 0.31) == [True, True, False, False, True, False, False, True, False, False]
    assert _cand(s, 10, 1.0, 0.5) == [True, True, True, False, True, False, False, True, False, False]
    assert _cand(s, 10, 1.0, 0.05) == [False] * 7 + [True, False, False]  # ceil(0.5) = 1
    # fewer pass than the cap allows: the cap adds nobody
    assert _cand(s, 10, 4.0, 0.5) == [False, True, False, False, False, False, False, True, False, False]


def test_max_splats_cap():
    s = [3.0, 1.0, 2.0, 4.0]
    assert _cand(s, 4, 1.0, 1.0, max_splats=100) == [True] * 4
    assert _cand(s, 4, 1.0, 1.0, max_splats=6) == [True, False, False, True]   # room for two
    assert _cand(s, 4, 1.0, 0.25, max_splats=6) == [False, False, False, True]  # the growth cap is the smaller one
    assert _cand(s, 4, 1.0, 1.0, max_splats=4) == [False] * 4                   # max_splats == n
    assert _cand(s, 4, 1.0, 1.0, max_splats=2) == [False] * 4                   # max_splats < n: clamped at 0
    assert _cand(s, 4, 1.0, 1.0, max_splats=0) == [False] * 4


def test_nan_scores_never_pass_and_empty():
    nan = float("nan")
    assert _cand([nan, 2.0, nan, 1.0], 4, 1.0, 1.0) == [False, True, False, True]
    assert _cand([nan, 2.0, nan, 1.0], 4, 1.0, 0.25) == [False, True, False, False]
    assert _cand([nan, nan], 2, 0.0, 1.0) == [False, False]
    assert _cand([float("inf"), 1.0], 2, 1.0, 0.5) == [True, False]
    assert _cand([], 0, 1.0, 0.05) == []
    assert _cand([], 0, 1.0, 0.05, max_splats=10) == []
    import torch

    from brush_amd.train import densify_candidates

    with pytest.raises(ValueError, match="scores must be"):
        densify_candidates(torch.zeros(3), 4, 1.0, 0.05)


# ---------------------------------------------------------------------------- revised opacity
def test_revised_opacity_against_float64():
    import torch

    from brush_amd.train import revised_opacity

    raw = torch.tensor([-12.0, -5.293, -2.0, -0.1, 0.0, 0.7, 2.0, 5.0, 9.0, 15.0], dtype=torch.float32)
    got = revised_opacity(raw).double().numpy()
    x = raw.double().numpy()
    o = 1.0 / (1.0 + np.exp(-x))
    root = np.sqrt(1.0 / (1.0 + np.exp(x)))          # sqrt(1 - o) without the cancellation
    new = o / (1.0 + root)                            # 1 - sqrt(1 - o)
    want = np.log(new / root)                         # logit(new): 1 - new = root
    # float32 sigmoid, sqrt, two divisions and a log: a handful of roundings, amplified by at most 1 / |logit'| <= 1
    # on the logit's scale of |want| <= 16: 16 eps32 relative to max(|want|, 1)
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -24 * np.maximum(np.abs(want), 1.0)), (got, want)
    # the definition: two splats of the new opacity cover what the source covered
    o_new = 1.0 / (1.0 + np.exp(-got))
    assert np.allclose(1.0 - (1.0 - o_new) ** 2, o, rtol=1e-5, atol=1e-9)
    assert np.all(got < x)


# ---------------------------------------------------------------------------- configuration and command line
def test_defaults_and_good_values():
    from brush_amd import TrainConfig

    c = TrainConfig()
    assert (c.densify_by, c.densify_error_thresh, c.densify_error_views, c.densify_growth, c.densify_max_splats,
            c.revised_opacity) == ("grad", 1.0, 32, 0.05, None, False)
    c.check()
    TrainConfig(densify_by="error", densify_error_thresh=0.0, densify_error_views=0, densify_growth=1.0,
                densify_max_splats=0, revised_opacity=True).check()
    # what the option combines with
    TrainConfig(densify_by="error", antialiased=True, background="random", filter3d=True, depth_weight=0.1,
                downscale_schedule=((0, 2), (10, 1)), contribution_prune_at=(5,)).check()
    # nothing asked, nothing refused
    TrainConfig(strategy="mcmc", revised_opacity=True).check(multi_rank=True)
    TrainConfig(pose_opt=True, exposure_opt=True).check()


def test_refused_combinations():
    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop

    class Exchange:
        world = 2

    with pytest.raises(ValueError, match=r"densify_by='error' cannot be combined with strategy='mcmc'"):
        TrainConfig(densify_by="error", strategy="mcmc").check()
    with pytest.raises(ValueError, match=r"densify_by='error' cannot be combined with a multi-rank exchange"):
        TrainConfig(densify_by="error").check(multi_rank=True)
    with pytest.raises(ValueError, match=r"densify_by='error' cannot be combined with pose_opt"):
        TrainConfig(densify_by="error", pose_opt=True).check()
    with pytest.raises(ValueError, match=r"densify_by='error' cannot be combined with exposure_opt"):
        TrainConfig(densify_by="error", exposure_opt=True).check()
    # at construction of the loop, before anything touches the dataset or a device
    with pytest.raises(ValueError, match="multi-rank exchange"):
        TrainLoop(None, TrainConfig(densify_by="error"), steps=20, exchange=Exchange())
    with pytest.raises(ValueError, match="pose_opt"):
        TrainLoop(None, TrainConfig(densify_by="error", pose_opt=True), steps=20)


@pytest.mark.parametrize("kw,match", [
    ({"densify_by": "ssim"}, "densify_by must be 'grad' or 'error'"),
    ({"densify_error_thresh": -0.5}, "densify_error_thresh must be finite and >= 0"),
    ({"densify_error_thresh": float("nan")}, "densify_error_thresh"),
    ({"densify_error_views": -1}, "densify_error_views must be an integer >= 0"),
    ({"densify_error_views": 2.5}, "densify_error_views"),
    ({"densify_growth": 0.0}, r"densify_growth must be in \(0, 1\]"),
    ({"densify_growth": 1.5}, r"densify_growth must be in \(0, 1\]"),
    ({"densify_growth": float("nan")}, "densify_growth"),
    ({"densify_max_splats": -3}, "densify_max_splats"),
    ({"densify_max_splats": 10.5}, "densify_max_splats")])
def test_bad_values(kw, match):
    from brush_amd import TrainConfig

    with pytest.raises(ValueError, match=match):
        TrainConfig(**kw).check()  # whatever densify_by says: a bad value is refused before it could be used


def test_parser(capsys):
    from brush_amd import train_loop

    d = train_loop.parser().parse_args(["scene"])
    assert (d.densify_by, d.densify_error_thresh, d.densify_error_views, d.densify_growth, d.max_splats,
            d.revised_opacity) == ("grad", 1.0, 32, 0.05, None, False)
    a = train_loop.parser().parse_args(["scene", "--densify-by", "error", "--densify-error-thresh", "0.25",
                                        "--densify-error-views", "0", "--densify-growth", "0.1", "--max-splats",
                                        "200000", "--revised-opacity"])
    assert (a.densify_by, a.densify_error_thresh, a.densify_error_views, a.densify_growth, a.max_splats,
            a.revised_opacity) == ("error", 0.25, 0, 0.1, 200000, True)
    for argv in (["scene", "--densify-by", "error", "--strategy", "mcmc"],
                 ["scene", "--densify-by", "error", "--pose-opt"],
                 ["scene", "--densify-by", "error", "--exposure-opt"],
                 ["scene", "--densify-growth", "0"], ["scene", "--densify-by", "loss"]):
        with pytest.raises(SystemExit):
            train_loop.main(argv)
    capsys.readouterr()


def test_train_log_carries_the_new_fields():
    from brush_amd.train_loop import TrainLog

    log = TrainLog(3, np.zeros(3, np.float32))
    assert log.densify_by == "grad" and log.error_passes == []
    log.densify_by = "error"
    log.error_passes.append((5, 4))
    j = log.to_json()
    assert j["densify_by"] == "error" and j["error_passes"] == [[5, 4]]


def test_lazy_exports():
    import brush_amd
    from brush_amd import error_score

    for name in ("ErrorScores", "ErrorScoreBuffers", "l1_error_map", "error_scores_from_aux", "splat_error_scores"):
        assert getattr(brush_amd, name) is getattr(error_score, name)


# ---------------------------------------------------------------------------- the reference checks itself
def _map(case, lo=0.0, hi=1.0, seed=0):
    return np.random.default_rng(seed + case["w"]).uniform(lo, hi, (case["h"], case["w"])).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in CC.all_cases()}


def test_float32_restatement_is_inside_the_allowance(cases):
    for name, c in cases.items():
        m = _map(c)
        ref = R.walk(c, m)
        ratio = R.gate(R.emulate32(c, m) / R.Q24, ref)
        assert ratio <= 1.0, (name, ratio)
        assert not ref["err"][~ref["touched"]].any()


def test_all_ones_restatement_is_the_contribution_sum(cases):
    for name in ("batch_65", "ragged_17x9", "saturating", "clamped"):
        c = cases[name]
        q = R.emulate32(c, np.ones((c["h"], c["w"]), np.float32))
        assert np.array_equal(q.astype(np.float64) / R.Q24, contrib_ref64.emulate32(c)["sum"]), name
        ref = R.walk(c, np.ones((c["h"], c["w"]), np.float32))
        assert np.allclose(ref["err"], contrib_ref64.walk(c)["sum"], rtol=0, atol=1e-12)


def test_clamp_map():
    m = np.array([[-1.0, 2.0, np.nan], [np.inf, -np.inf, 0.25]], np.float32)
    assert R.clamp_map(m).tolist() == [[0.0, 1.0, 0.0], [1.0, 0.0, 0.25]]


def test_each_wrong_reference_is_rejected(cases):
    """On the cases the GPU test names, the restatement passes the right reference and fails each wrong one."""
    for mutation, name, lo, hi in (("ignore_map", "random_200", 0, 1), ("transposed_map", "ragged_17x9", 0, 1),
                                   ("transposed_map", "random_200", 0, 1), ("unclamped", "random_200", -1, 2),
                                   ("ignore_T", "random_200", 0, 1)):
        c = cases[name]
        m = _map(c, lo, hi)
        emu = R.emulate32(c, m) / R.Q24
        assert R.passes(R.gate(emu, R.walk(c, m))), (mutation, name)
        assert not R.passes(R.gate(emu, R.walk(c, m, mutate=mutation))), (mutation, name)
    # `unclamped` is the right reference on a map inside [0, 1]: it needs the out-of-range values
    c = cases["random_200"]
    m = _map(c)
    assert np.array_equal(R.walk(c, m)["err"], R.walk(c, m, mutate="unclamped")["err"])


# ---------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_error_scores_entry_validates_before_any_device_work(lib):
    from brush_amd import _lib

    u = _lib.BrushUniforms()
    u.img_size[:] = [17, 9]
    u.tile_bounds[:] = [2, 1]
    aux = _lib.BrushAux()
    fake = 0x1000  # never dereferenced on the host: every call below is refused before a launch
    names = ("projected_splats", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid", "num_visible")
    for name in names:
        setattr(aux, name, fake)
    aux.max_intersects = 8
    call = lib.brush_render_error_scores
    ok_args = [C.byref(u), C.byref(aux), fake, fake, 4, None]
    for i in range(4):  # uniforms, aux, error_map, view_err
        args = list(ok_args)
        args[i] = None
        assert call(*args) == -1, i
    assert call(C.byref(u), C.byref(aux), fake + 2, fake, 4, None) == -1  # error_map: 4-byte aligned
    assert call(C.byref(u), C.byref(aux), fake, fake + 4, 4, None) == -1  # view_err: 8-byte aligned
    for name in names:
        setattr(aux, name, None)
        assert call(*ok_args) == -1, name
        setattr(aux, name, fake)
    assert aux.final_index is None  # not needed
    assert call(C.byref(u), C.byref(aux), fake, fake, 0, None) == 0  # n = 0: nothing to do, no launch
    aux.max_intersects = 0
    assert call(*ok_args) == -1
    aux.max_intersects = 8
    u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
    assert call(*ok_args) == -1
    u.tile_bounds[:] = [2, 1]
    u.img_size[:] = [0, 9]
    assert call(*ok_args) == -1


def test_l1_error_map_entry_validates_before_any_device_work(lib):
    from brush_amd import _lib

    fake = 0x1000
    call = lib.brush_l1_error_map
    ok_args = [fake, fake, _lib.EVAL_GT_U8, 3, None, fake, 17, 9, None]
    for i in (0, 1, 5):  # pred, gt, out
        args = list(ok_args)
        args[i] = None
        assert call(*args) == -1, i
    for i, bad in ((2, 2), (3, 2), (3, 5), (6, 0), (7, 0), (6, 1 << 20)):  # dtype, channels, sizes (2^20 x 9... x 2^20)
        args = list(ok_args)
        args[i] = bad
        if i == 6 and bad == 1 << 20:
            args[7] = 1 << 20  # 2^40 pixels
        assert call(*args) == -1, (i, bad)
    assert call(fake + 4, fake, _lib.EVAL_GT_U8, 3, None, fake, 17, 9, None) == -1   # pred: 16-byte aligned
    assert call(fake, fake, _lib.EVAL_GT_U8, 3, None, fake + 2, 17, 9, None) == -1   # out: 4-byte aligned
    assert call(fake, fake + 2, _lib.EVAL_GT_F32, 3, None, fake, 17, 9, None) == -1  # an f32 target: 4-byte aligned


def test_error_kernels_static_lds_and_no_spills(lib):
    """k_error_quad: one kernel, the static LDS the .hip pins with a static_assert (4 waves x 64 records x 32 bytes);
    k_l1_error_map: eight instantiations (u8 / f32, 3 / 4 channels, with and without a mask) and no LDS; no spills and
    no scratch anywhere; the forward's and the contribution replay's kernels are their own."""
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_error_quad|k_l1_error_map")
    quad = [n for n in res if "k_error_quad" in n]
    maps = [n for n in res if "k_l1_error_map" in n]
    assert len(quad) == 1 and len(maps) == 8 and len(res) == 9, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name
        assert r["group_segment_fixed_size"] == (8192 if name in quad else 0), name
    walk = open(os.path.join(ROOT, "brush_amd", "csrc", "replay_walk.hpp")).read()  # the staged record is the shared walk's
    assert "static_assert(sizeof(ReplayRec) * kTilesPerBlock * kBatch == 8192" in walk
    assert "k_rasterize" not in quad[0] and "k_contribution" not in quad[0]
    assert len(kd.resources(_lib.LIB_PATH, r"k_contribution_quad")) == 1
