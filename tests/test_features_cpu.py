"""CPU-side checks of the feature replays: the float64 reference checks itself (a float32 restatement inside every
gate, every wrong reference rejected on a named case), the host logic on arrays (FeatureSums.mean, the argmax of
lift_labels: ties, min_weight, -1), the pure-Python layer (exports, the lift command line's parser and label-file
lookup), and the library: the three symbols, argument validation without a device, and the kernels' resources."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import features_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
Q24 = 2.0 ** 24


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("c", [1, 5, 17])
def test_float32_restatement_passes_every_gate(c):
    worst = {}
    for case in CASES:
        f, v, m = R.seeded(case, c)
        ref = R.walk(case, f, v, m)
        emu = R.emulate32(case, f, v, m)
        g = R.gate(ref, out=emu["out"], grad=emu["grad"], q=emu["q"] / Q24)
        assert R.passes(g), (case["name"], g)
        assert not emu["out"][~ref["added"]].any() and not emu["grad"][~ref["touched"]].any()
        assert not emu["q"][~ref["touched"]].any()
        assert (ref["partials"][ref["touched"]] >= 1).all() and not ref["partials"][~ref["touched"]].any()
        for k, x in g.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"C={c}: worst err/tol of the float32 restatement {worst}")
    assert all(0.0 < x <= 1.0 for x in worst.values())  # the allowances are neither vacuous nor violated


WRONG = [("chw", "ragged_17x9"), ("chw", "random_200"), ("channel_off_by_one", "batch_65"), ("ignore_T", "random_200"),
         ("stop_added", "saturating"), ("stop_added", "clamped"), ("compact_row", "four_tiles"),
         ("compact_row", "random_200")]


def test_every_mutation_is_named():
    assert {m for m, _ in WRONG} == set(R.MUTATIONS)


@pytest.mark.parametrize("mutation,name", WRONG)
def test_each_wrong_reference_is_rejected(mutation, name):
    case = BY_NAME[name]
    f, v, m = R.seeded(case, 5)
    emu = R.emulate32(case, f, v, m)
    got = dict(out=emu["out"], grad=emu["grad"], q=emu["q"] / Q24)
    assert R.passes(R.gate(R.walk(case, f, v, m), **got))
    bad = R.gate(R.walk(case, f, v, m, mutate=mutation), **got)
    assert all(x > 1.0 for x in bad.values()), (mutation, name, bad)


def test_one_channel_sums_restate_the_error_reference():
    from tests import error_ref64 as E

    case = BY_NAME["random_200"]
    f, v, m = R.seeded(case, 1)
    assert np.array_equal(R.emulate32(case, f, v, m)["q"][:, 0], E.emulate32(case, m[..., 0]))
    ref, eref = R.walk(case, f, v, m), E.walk(case, m[..., 0])
    assert np.allclose(ref["q"][:, 0], eref["err"], rtol=1e-13, atol=0) and np.array_equal(ref["touched"], eref["touched"])
    assert np.allclose(ref["tol_q"][:, 0], eref["tol_err"], rtol=1e-12, atol=0)  # the same allowance, term by term


def test_one_hot_and_gate_edges():
    lab = np.array([[0, 1, 2], [3, 255, 1]], np.uint8)
    hot = R.one_hot(lab, 2)
    assert hot.shape == (2, 3, 2) and hot.dtype == np.float32
    assert np.array_equal(hot[..., 0], [[1, 0, 0], [0, 0, 0]]) and np.array_equal(hot[..., 1], [[0, 1, 0], [0, 0, 1]])
    assert R.ratio(np.array([1.0]), np.array([1.0]), np.array([0.0])) == 0.0
    assert R.ratio(np.array([1.0]), np.array([0.0]), np.array([0.0])) == np.inf
    assert R.ratio(np.array([np.nan]), np.array([0.0]), np.array([1.0])) == np.inf


# ---------------------------------------------------------------------------- the host logic
def test_feature_sums_mean_on_arrays():
    import torch

    from brush_amd.features import FeatureSums

    s = torch.tensor([[3, 1], [0, 0], [5, 0], [1 << 40, 7]], dtype=torch.int64)
    w = torch.tensor([4, 0, 5, 1 << 41], dtype=torch.int64)
    fs = FeatureSums(s, w, 2)
    mean = fs.mean()
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (4, 2)
    want = np.array([[0.75, 0.25], [0.0, 0.0], [1.0, 0.0], [0.5, 7.0 / 2.0 ** 41]], np.float64).astype(np.float32)
    assert np.array_equal(mean.numpy(), want)
    r = fs.read()
    assert torch.equal(r.sum, s) and torch.equal(r.weight, w) and r.views == 2


def test_labels_from_sums_argmax_ties_min_weight():
    import torch

    from brush_amd.features import labels_from_sums

    one = 1 << 24
    s = torch.tensor([[0, 0, 0],            # nothing: -1
                      [5, 9, 2],            # class 1
                      [7, 7, 3],            # tie: the lowest class
                      [0, 4, 4],            # tie between 1 and 2
                      [2 * one, one, 0],    # 2 px
                      [one, 0, one + 1]], dtype=torch.int64)
    got = labels_from_sums(s)
    assert got.dtype == torch.int32 and got.tolist() == [-1, 1, 0, 1, 0, 2]
    # min_weight in pixels of full weight: strictly above it
    assert labels_from_sums(s, 1.0).tolist() == [-1, -1, -1, -1, 0, 2]
    assert labels_from_sums(s, 2.0).tolist() == [-1, -1, -1, -1, -1, -1]
    assert labels_from_sums(torch.zeros((0, 3), dtype=torch.int64)).tolist() == []
    with pytest.raises(ValueError, match="min_weight"):
        labels_from_sums(s, -1.0)
    with pytest.raises(ValueError, match="min_weight"):
        labels_from_sums(s, float("nan"))
    with pytest.raises(ValueError, match="int64"):
        labels_from_sums(s.to(torch.int32))


def test_python_refusals_before_any_launch():
    import torch

    from brush_amd import _lib
    from brush_amd import features as F

    u = _lib.BrushUniforms()
    u.img_size[:] = [17, 9]
    with pytest.raises(ValueError, match="features must be"):
        F.features_from_aux(u, None, torch.zeros((4, 3)))  # on the CPU
    with pytest.raises(ValueError, match="v_features must be"):
        F.feature_grads_from_aux(u, None, torch.zeros((9, 17, 3)), torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="sums must be"):
        F.feature_sums_from_aux(u, None, torch.zeros((9, 17, 3)), torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="remap"):
        F.lift_labels(None, [], [], 65)
    with pytest.raises(ValueError, match="one map per view"):
        F.splat_feature_sums(None, [1, 2], [1])
    with pytest.raises(ValueError, match="channel count"):
        F._check_channels(0)
    with pytest.raises(ValueError, match="channel count"):
        F._check_channels(65)
    assert F._check_channels(1) == 1 and F._check_channels(64) == 64 == F.MAX_CHANNELS


def test_exports():
    import brush_amd
    from brush_amd import features

    for name in ("render_features", "splat_feature_sums", "lift_labels", "FeatureSums", "features_from_aux",
                 "feature_grads_from_aux", "feature_sums_from_aux"):
        assert getattr(brush_amd, name) is getattr(features, name), name
    assert hasattr(brush_amd.Splats, "render_features")
    assert "frozen" in features.render_features.__doc__ and "frozen" in features.__doc__.lower()


# ---------------------------------------------------------------------------- the command line
def test_lift_parser_and_refusals(capsys, tmp_path):
    from brush_amd import lift

    a = lift.parser().parse_args(["in.ply", "scene", "--labels", "seg"])
    assert a.labels == "seg" and a.num_classes is None and a.views == "train" and a.min_weight == 0.0
    assert not a.antialiased and not a.no_undistort and a.select is None and a.export is None
    lift.check_args(a)
    a = lift.parser().parse_args(["in.ply", "scene", "--labels", "seg", "--num-classes", "5", "--views", "all",
                                  "--antialiased", "--no-undistort", "--min-weight", "2.5", "--export-labels", "l.npy",
                                  "--select", "3", "--export", "o.ply", "--render-dir", "r", "--json", "o.json"])
    assert (a.num_classes, a.views, a.min_weight, a.select, a.export) == (5, "all", 2.5, 3, "o.ply")
    assert a.antialiased and a.no_undistort and a.export_labels == "l.npy" and a.render_dir == "r" and a.json == "o.json"
    lift.check_args(a)
    missing = str(tmp_path / "missing")  # nothing is read: the parser refuses first
    for argv, msg in (([missing, missing], "--labels"),
                      ([missing, missing, "--labels", "d", "--select", "1"], "go together"),
                      ([missing, missing, "--labels", "d", "--export", "o.ply"], "go together"),
                      ([missing, missing, "--labels", "d", "--num-classes", "65"], "remap"),
                      ([missing, missing, "--labels", "d", "--num-classes", "0"], "--num-classes"),
                      ([missing, missing, "--labels", "d", "--min-weight", "-1"], "--min-weight"),
                      ([missing, missing, "--labels", "d", "--views", "some"], "--views")):
        with pytest.raises(SystemExit) as e:
            lift.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, argv


def test_label_file_lookup_and_the_mask_field_round_trip(tmp_path):
    from PIL import Image

    from brush_amd import lift
    from brush_amd.dataset import SceneView

    d = tmp_path / "seg"
    d.mkdir()
    lab = np.array([[0, 1, 255], [2, 254, 1]], np.uint8)
    Image.fromarray(lab, mode="L").save(d / "0001.jpg.png")   # <image name>.png wins
    Image.fromarray(lab.T.copy(), mode="L").save(d / "0001.png")
    Image.fromarray(lab, mode="L").save(d / "0002.png")       # <stem>.png
    pal = Image.fromarray(lab, mode="P")
    pal.putpalette([i % 256 for i in range(768)])
    pal.save(d / "0003.png")
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(d / "0004.png")  # RGB: refused
    assert lift.find_label_file(str(d), "scene/images/0001.jpg") == str(d / "0001.jpg.png")
    assert lift.find_label_file(str(d), "scene/images/0002.jpg") == str(d / "0002.png")
    assert lift.find_label_file(str(d), "images\\0002.jpg") == str(d / "0002.png")
    assert lift.find_label_file(str(d), "scene/images/0009.jpg") is None
    assert np.array_equal(lift.decode_labels(str(d / "0002.png")), lab)
    assert np.array_equal(lift.decode_labels(str(d / "0003.png")), lab)  # palette indices are the class ids
    with pytest.raises(ValueError, match="single channel"):
        lift.decode_labels(str(d / "0004.png"))
    img = np.zeros((2, 3, 3), np.uint8)
    mask = np.array([[255, 255, 255], [0, 255, 255]], np.uint8)
    views = [SceneView("scene/images/0001.jpg", None, img), SceneView("scene/images/0002.jpg", None, img, mask=mask),
             SceneView("scene/images/0003.jpg", None, np.zeros((4, 6, 3), np.uint8))]
    out = lift.with_labels_as_masks(views, str(d))
    assert views[0].mask is None  # copies
    assert np.array_equal(out[0].mask, [[1, 2, 0], [3, 255, 2]])  # shifted by one: unlabelled is 0, as "no source"
    assert np.array_equal(lift.labels_of(out[0]), lab)
    masked = lab.copy()
    masked[1, 0] = 255  # the view's own loss mask rules the pixel out
    assert np.array_equal(lift.labels_of(out[1]), masked)
    big = lift.labels_of(out[2])  # another size: nearest resize to the view's
    assert big.shape == (4, 6) and np.array_equal(big[::2, ::2], lab) and np.array_equal(big[1::2, 1::2], lab)
    with pytest.raises(ValueError, match="no label image"):
        lift.with_labels_as_masks([SceneView("scene/images/0009.jpg", None, img)], str(d))


# ---------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_the_three_symbols_are_exported_and_bound(lib):
    from brush_amd import _lib

    for name in ("brush_render_features", "brush_render_features_backward", "brush_render_feature_sums"):
        assert name in _lib.SYMBOL_NAMES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == (8 if name.endswith("sums") else 7)
    header = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    assert "#define BRUSH_FEATURE_MAX_CHANNELS 64u" in header
    assert "#define BRUSH_FEATURE_MAP_F32 0u" in header and "#define BRUSH_FEATURE_MAP_LABEL_U8 1u" in header


def test_entries_validate_before_any_device_work(lib):
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
    U, A = C.byref(u), C.byref(aux)
    entries = {
        "fwd": (lib.brush_render_features, [U, A, fake, 5, fake, 4, None], (2, 4), 3, 5),
        "bwd": (lib.brush_render_features_backward, [U, A, fake, 5, fake, 4, None], (2, 4), 3, 5),
        "sums": (lib.brush_render_feature_sums, [U, A, fake, 0, 5, fake, 4, None], (2, 5), 4, 6),
    }
    for key, (call, ok, ptrs, ci, ni) in entries.items():
        for i in (0, 1) + ptrs:  # uniforms, aux and the two device pointers
            args = list(ok)
            args[i] = None
            assert call(*args) == -1, (key, i)
        for c in (0, 65, 1 << 31):
            args = list(ok)
            args[ci] = c
            assert call(*args) == -1, (key, c)
        for c in (1, 64):
            args = list(ok)
            args[ci], args[ni] = c, 0
            if key != "fwd":  # n = 0: nothing to do, no launch (the forward replay would still write zeros)
                assert call(*args) == 0, (key, c)
        for i in ptrs:  # f32: 4-byte aligned
            args = list(ok)
            args[i] = fake + 2
            assert call(*args) == -1, (key, i)
        for name in names:
            setattr(aux, name, None)
            assert call(*ok) == -1, (key, name)
            setattr(aux, name, fake)
        aux.max_intersects = 0
        assert call(*ok) == -1, key
        aux.max_intersects = 8
        u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
        assert call(*ok) == -1, key
        u.tile_bounds[:] = [2, 1]
        u.img_size[:] = [0, 9]
        assert call(*ok) == -1, key
        u.img_size[:] = [17, 9]
    sums = lib.brush_render_feature_sums
    assert sums(U, A, fake, 2, 5, fake, 4, None) == -1         # no such map kind
    assert sums(U, A, fake, 0, 5, fake + 4, 4, None) == -1     # sums: 8-byte aligned
    assert sums(U, A, fake + 1, 1, 5, fake, 0, None) == 0      # a label image needs no alignment
    assert lib.brush_render_features(U, A, None, 5, None, 0, None) == -1  # n = 0 still writes: out is required
    assert aux.final_index is None  # not needed


def test_feature_kernels_static_lds_and_no_spills(lib):
    """k_feature_quad: passes of 4, 8 and 16 channels, each with and without 16-byte slices, the static LDS of
    4 waves x 64 records x (32 + 4 CP) bytes; k_feature_grad_quad: three widths x three modes, ReplayRec's 8192 bytes;
    no spills and no scratch anywhere; registers far from the 128 of the 256-thread bound."""
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_feature_quad|k_feature_grad_quad")
    fwd = [n for n in res if "k_feature_quad" in n]
    grad = [n for n in res if "k_feature_grad_quad" in n]
    assert len(fwd) == 6 and len(grad) == 9 and len(res) == 15, sorted(res)
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name
    assert sorted(res[n]["group_segment_fixed_size"] for n in fwd) == [12288, 12288, 16384, 16384, 24576, 24576]
    assert all(res[n]["group_segment_fixed_size"] == 8192 for n in grad)
    src = open(os.path.join(ROOT, "brush_amd", "csrc", "features.hip")).read()
    assert "static_assert(sizeof(FeatRec<16>) * kTilesPerBlock * kBatch == 24576" in src
    walk = open(os.path.join(ROOT, "brush_amd", "csrc", "replay_walk.hpp")).read()  # the staged record is the shared walk's
    assert "static_assert(sizeof(ReplayRec) * kTilesPerBlock * kBatch == 8192" in walk
    assert len(kd.resources(_lib.LIB_PATH, r"k_error_quad")) == 1  # the replays it generalises are their own kernels


def test_the_compositing_walk_is_written_in_one_place():
    """The forward's walk (the `quad_may_pass(` ballot, the FCMP_UNO liveness check) stands in the compositing kernels'
    own files and in the replay walk's header, nowhere else.  Exempt, by name: the kernel whose walk stays written out
    (its staged record and its veto are its own)."""
    csrc = os.path.join(ROOT, "brush_amd", "csrc")
    allowed = {"rasterize.hip", "rasterize_bwd.hip", "raster_common.hpp", "replay_walk.hpp"}
    written_out = {"features.hip": ("k_feature_quad",)}
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if name in allowed or not os.path.isfile(path):
            continue
        src = open(path, errors="replace").read()
        for kernel in written_out.get(name, ()):  # cut it out: from its name to the brace that closes it in column 0
            start = src.index("void %s(" % kernel)
            src = src[:start] + src[src.index("\n}\n", start):]
        for needle in ("quad_may_pass(", "FCMP_UNO"):
            assert needle not in src, (name, needle)
