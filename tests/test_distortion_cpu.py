"""CPU-side checks of the depth-distortion term: the float64 reference checks itself (the running form against the
brute-force pair sum, closed forms, the shift invariance, sum w g = 2 L, the analytic compact-row sums against torch
float64 autograd of an independent dense restatement, every wrong reference rejected), the pure-Python layer (the
ctypes struct and prototypes against the header, TrainConfig validation, the step's refusals, the command lines) and
the library's argument validation without a device."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import distortion_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c["name"] for c in CASES]
MODES = {"depth": dict(mode="depth"), "ndc": R.NDC}


@functools.lru_cache(maxsize=None)
def ref(name, mode, mutate=None):
    """(depth, v, reference walk) of a case: computed once, shared and left unchanged."""
    case = BY_NAME[name]
    z, v = R.seeded_depth(case), R.seeded_v(case)
    return z, v, R.walk(case, z, v, mutate=mutate, **MODES[mode])


# ---------------------------------------------------------------------------- the reference
def test_seeded_depths_are_non_decreasing_with_equal_neighbours():
    for case in CASES:
        z = R.seeded_depth(case)
        assert z.dtype == np.float32 and z.shape == (case["n"],) and (np.diff(z) >= 0).all() and (z >= 1.0).all()
    z = R.seeded_depth(BY_NAME["random_200"])
    assert (np.diff(z) == 0).any() and (np.diff(z) > 0).any()


def test_every_case_is_threshold_free():
    """contrib_cases asserts it for its own; the case added here must be too: no alpha test and no stop test within 8
    allowances of its threshold, and no alpha_u within 8 allowances of the clamp but the ones that are exactly 1."""
    from tests import contrib_ref64 as CR

    assert CR.decisions(R.clamped_pair()).min() > 8.0


@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_running_form_equals_the_brute_force_pair_sum(case, mode):
    z, _, want = ref(case["name"], mode)
    brute = R.brute_force(case, z, **MODES[mode])
    L = want["stats"][..., 0]
    scale = np.maximum(np.abs(brute), 1e-300)
    assert (np.abs(L - brute) <= 1e-11 * scale + 1e-30).all(), float(np.max(np.abs(L - brute) / scale))
    assert not L[~want["added"]].any() and (L >= 0).all()
    if case["num_isect"] == 0:
        assert not want["stats"].any() and not want["rows"].any()


@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sum_of_w_g_is_twice_L(case, mode):
    _, _, want = ref(case["name"], mode)
    L = want["stats"][..., 0]
    assert (np.abs(want["sum_wg"] - 2.0 * L) <= 1e-11 * np.maximum(L, 1e-300)).all()


def test_closed_forms():
    one = BY_NAME["one_record"]
    assert not R.walk(one, R.seeded_depth(one), R.seeded_v(one))["stats"][..., 0].any()  # one hit: no pair
    # equal depths: every pair vanishes, and so does every gradient
    case = BY_NAME["random_200"]
    flat = R.walk(case, np.full(case["n"], 2.5, np.float32), R.seeded_v(case))
    assert not flat["stats"][..., 0].any() and not flat["stats"][..., 2:].any() and not flat["rows"].any()
    assert flat["stats"][..., 1].max() > 0.5
    # two concentric hits: w1 = a, w2 = a (1 - a), L = w1 w2 (m1 - m2)^2
    pair = BY_NAME["exact_pair"]
    z = np.array([1.5, 4.0], np.float32)
    for mode, kw in MODES.items():
        got = R.walk(pair, z, **kw)["stats"][..., 0]
        p = pair["projected"].astype(np.float64)
        ys, xs = np.meshgrid(np.arange(16) + 0.5, np.arange(16) + 0.5, indexing="ij")
        dx, dy = p[0, 0] - xs, p[0, 1] - ys
        a = p[0, 8] * np.exp(-(0.5 * (p[0, 2] * dx * dx + p[0, 4] * dy * dy) + p[0, 3] * dx * dy))
        m = R.mu(z.astype(np.float64), **kw)[0]
        both = a >= R.INV255  # (0.25 (1 - 0.25) never stops)
        want = np.where(both, a * (a * (1 - a)) * (m[0] - m[1]) ** 2, 0.0)
        assert np.allclose(got, want, rtol=1e-12, atol=0) and both.any(), mode


def test_shift_invariance():
    case = BY_NAME["random_200"]
    z = np.round(R.seeded_depth(case) * 1024.0) / 1024.0  # a shift by 8 is then exact in float32
    v = R.seeded_v(case)
    a, b = R.walk(case, z.astype(np.float32), v), R.walk(case, (z + 8.0).astype(np.float32), v)
    assert ((z + 8.0).astype(np.float32).astype(np.float64) - 8.0 == z).all()
    for key in ("stats", "rows"):
        assert np.allclose(a[key], b[key], rtol=1e-10, atol=1e-18), key


# ---------------------------------------------------------------------------- autograd of a dense restatement
def dense_rows(case, z, v, mode, near=0.2, far=None):
    """d (sum_p v(p) L(p)) / d (mean2d, conic, opacity, z) per record by torch float64 autograd of the PAIR form over
    (mean2d, conic, opacity, z): [n,7] in the columns of R.ROW_WORDS.  Uses none of the reference's formulas: the
    weights come from the product of (1 - alpha), L from all ordered pairs halved."""
    import torch

    f64 = torch.float64
    p = torch.tensor(case["projected"].astype(np.float64))
    mean = p[:, 0:2].clone().requires_grad_(True)
    conic = p[:, 2:5].clone().requires_grad_(True)
    opac = p[:, 8].clone().requires_grad_(True)
    zz = torch.tensor(np.asarray(z, np.float32).astype(np.float64))[: p.shape[0]].clone().requires_grad_(True)
    if mode == "ndc":
        A, nz = R.scale_a(near, far), float(np.float32(near))
        m_all = A * (1.0 - nz / zz)
    else:
        m_all = zz
    V = torch.tensor(np.asarray(v, np.float32).astype(np.float64))
    bins, isect = case["tile_bins"], case["isect"]
    total = torch.zeros((), dtype=f64)
    for ty in range(bins.shape[0]):
        for tx in range(bins.shape[1]):
            ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, case["h"])),
                                 np.arange(tx * 16, min(tx * 16 + 16, case["w"])), indexing="ij")
            px = torch.tensor(xs.reshape(-1) + 0.5)
            py = torch.tensor(ys.reshape(-1) + 0.5)
            T = torch.ones_like(px)
            alive = torch.ones_like(px, dtype=torch.bool)
            ws, ms = [], []
            for i in range(int(bins[ty, tx, 0]), int(bins[ty, tx, 1])):
                c = int(isect[i])
                dx, dy = mean[c, 0] - px, mean[c, 1] - py
                sigma = 0.5 * (conic[c, 0] * dx * dx + conic[c, 2] * dy * dy) + conic[c, 1] * dx * dy
                au = opac[c] * torch.exp(-sigma)
                al = torch.clamp(au, max=R.CLAMP)  # (no gradient through the clamped branch)
                with torch.no_grad():
                    passed = alive & (sigma >= 0) & (au >= R.INV255)
                    stop = passed & (T * (1 - al) <= R.T_STOP)
                    hit = passed & ~stop
                    alive = alive & ~stop
                ws.append(torch.where(hit, al * T, torch.zeros_like(T)))
                ms.append(m_all[c])
                T = torch.where(hit, T * (1 - al), T)
            if not ws:
                continue
            Wm, m = torch.stack(ws), torch.stack(ms)
            D2 = (m[:, None] - m[None, :]) ** 2
            Lp = 0.5 * torch.einsum("ip,jp,ij->p", Wm, Wm, D2)
            total = total + (Lp * V[ys.reshape(-1), xs.reshape(-1)]).sum()
    out = np.zeros((case["n"], 7))
    if total.requires_grad:
        gm, gc, go, gz = torch.autograd.grad(total, (mean, conic, opac, zz), allow_unused=True)
        k = p.shape[0]
        for j, g in ((0, gm[:, 0]), (1, gm[:, 1]), (2, gc[:, 0]), (3, gc[:, 1]), (4, gc[:, 2]), (5, go), (6, gz)):
            out[:k, j] = g.numpy()
    return out


@pytest.mark.parametrize("mode", ["depth", "ndc"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_analytic_rows_equal_autograd_of_the_dense_restatement(case, mode):
    z, v, want = ref(case["name"], mode)
    if case["num_visible"] == 0:
        assert not want["rows"].any()
        return
    auto = dense_rows(case, z, v, **MODES[mode])
    err = np.abs(auto - want["rows"])
    assert (err <= 1e-9 * want["abs_rows"] + 1e-300).all(), float(np.max(err / np.maximum(want["abs_rows"], 1e-300)))
    assert not want["rows"][~want["touched"]].any()
    if case["num_isect"] > 1:
        assert want["touched"].any()


# ---------------------------------------------------------------------------- wrong references
WRONG = [("pairs_twice", "random_200", "depth"), ("ignore_T", "random_200", "depth"), ("stop_added", "saturating", "depth"),
         ("global_row", "four_tiles", "depth"), ("global_row", "random_200", "ndc"), ("no_dmu", "random_200", "ndc"),
         ("clamp_grad", "clamped_pair", "depth"), ("suffix_incl", "random_200", "depth"), ("suffix_incl", "batch_65", "ndc")]


def test_every_mutation_is_named():
    assert {m for m, _, _ in WRONG} == set(R.MUTATIONS)


@pytest.mark.parametrize("mutation,name,mode", WRONG)
def test_each_wrong_reference_is_rejected(mutation, name, mode):
    """The true reference's values stand in for the device: they pass the true gate with ratio 0 and must fail the
    mutated one."""
    _, _, true = ref(name, mode)
    _, _, bad = ref(name, mode, mutation)
    r = R.gate(bad, stats=true["stats"], rows=true["rows"])
    print(mutation, name, mode, r)
    assert not R.passes(r), (mutation, name, r)
    assert R.passes(R.gate(true, stats=true["stats"], rows=true["rows"]))


def test_allowances_are_finite_and_tight():
    """No allowance is vacuous: summed over a case's rows, a word's allowances stay below 1 % of the sum of its
    |terms| (single rows can be looser: a far splat's terms are small beside the error its pixel's totals carry, and
    1 / (1 - alpha) is up to 1000 next to the clamp); a pixel's stays below 1e-3 of L's own scale
    W^2 (m_max - m_min)^2."""
    for name in IDS:
        for mode in MODES:
            z, _, want = ref(name, mode)
            assert np.isfinite(want["tol_rows"]).all() and np.isfinite(want["tol_stats"]).all()
            t = want["touched"]
            if t.any():
                tot, mag = want["tol_rows"][t].sum(axis=0), want["abs_rows"][t].sum(axis=0)
                assert (tot <= 1e-2 * mag)[mag > 0].all(), (name, mode, tot / np.maximum(mag, 1e-300))
            m = R.mu(z.astype(np.float64), **MODES[mode])[0]
            span = (m.max() - m.min()) ** 2 if len(m) else 0.0
            assert (want["tol_stats"][..., 0] <= 1e-3 * max(span, 1e-30)).all(), (name, mode)


# ---------------------------------------------------------------------------- the end-to-end scene
def test_scene_stays_within_its_exclusion_cap_under_the_oracle():
    """The GPU test compares gradients splat by splat and leaves out the splats with a record within 8 allowances of a
    threshold: at most 5 % of the visible ones, here with the CPU oracle's projection, lists and order; and the scene is
    the one asked for (about 200 splats, opacities at most 0.9, a 48 x 40 frame, most of them seen)."""
    from tests import distortion_scene as S

    cloud = S.scene()
    assert cloud["means"].shape == (S.N, 3) and (1 / (1 + np.exp(-cloud["raw_opac"])) <= 0.9).all()
    assert (S.W, S.H) == (48, 40) and S.H % 16 == 8  # the last tile row is half outside: two quadrants per tile do not run
    case, z = S.oracle_case(cloud)
    v = case["num_visible"]
    assert v >= 150 and case["num_isect"] >= 2 * v and (z[:v] > 0.5).all()
    assert (np.diff(z[:v]) >= 0).all()  # the compact order is the depth order
    for mode in MODES.values():
        want = R.walk(case, z, R.seeded_v(case), **mode)
        bad, share = S.excluded(want, v)
        print(f"visible {v}, intersections {case['num_isect']}, excluded {int(bad.sum())} ({share:.3f})")
        assert share <= S.MAX_EXCLUDED
        assert want["touched"][:v].mean() > 0.8 and (want["stats"][..., 0] > 0).mean() > 0.5


# ---------------------------------------------------------------------------- the Python layer
def test_struct_and_prototypes_match_the_header():
    from brush_amd import _lib

    S = _lib.BrushDistortion
    assert C.sizeof(S) == 12
    assert (S.mode.offset, S.near_z.offset, S.far_z.offset) == (0, 4, 8)
    assert (_lib.DISTORTION_DEPTH, _lib.DISTORTION_NDC) == (0, 1)
    header = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    assert "#define BRUSH_DISTORTION_DEPTH 0u" in header and "#define BRUSH_DISTORTION_NDC 1u" in header
    assert re.search(r"typedef struct BrushDistortion \{\s*uint32_t mode;\s*float near_z, far_z;", header)
    protos = {name: args for name, _, args in _lib._SYMBOLS}
    for name in ("brush_render_distortion", "brush_distortion_compact_grads", "brush_render_backward_distortion"):
        decl = re.search(r"int " + name + r"\((.*?)\);", header, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == len(protos[name]), name
        for p, t in zip(params, protos[name]):
            if "BrushDistortion" in p:
                assert t is C.POINTER(S) or t == C.POINTER(S), (name, p)
            elif "uint32_t" in p and "*" not in p:
                assert t is C.c_uint32, (name, p)
            elif "size_t" in p:
                assert t is C.c_size_t, (name, p)


def test_distortion_config_validation():
    from brush_amd import _lib
    from brush_amd.distortion import distortion_config

    c = distortion_config()
    assert (c.mode, c.near_z, c.far_z) == (_lib.DISTORTION_DEPTH, 0.0, 0.0)
    c = distortion_config("ndc", 0.25, 40.0)
    assert (c.mode, c.near_z, c.far_z) == (_lib.DISTORTION_NDC, 0.25, 40.0)
    for bad in (dict(mode="disparity"), dict(mode="ndc"), dict(mode="ndc", far=0.1), dict(mode="ndc", near=0.0, far=5.0),
                dict(mode="ndc", far=float("inf")), dict(mode="ndc", near=float("nan"), far=5.0)):
        with pytest.raises(ValueError):
            distortion_config(**bad)


def test_exports():
    import brush_amd

    for name in ("render_distortion", "distortion_from_aux", "distortion_compact_grads_from_aux", "distortion_loss_into",
                 "distortion_config"):
        assert callable(getattr(brush_amd, name)), name
    assert callable(brush_amd.Splats.render_distortion)


def test_train_config_validation():
    from brush_amd import TrainConfig

    c = TrainConfig()
    assert (c.distortion_weight, c.distortion_from_step, c.distortion_mode, c.distortion_near, c.distortion_far) == \
        (0.0, 3000, "depth", 0.2, None)
    c.check()
    TrainConfig(distortion_weight=100.0, distortion_from_step=0).check()
    TrainConfig(distortion_weight=1.0, distortion_mode="ndc", distortion_far=30.0).check()
    for bad in (dict(distortion_weight=-1.0), dict(distortion_weight=float("nan")), dict(distortion_weight=True),
                dict(distortion_from_step=-1), dict(distortion_from_step=2.5), dict(distortion_mode="disparity"),
                dict(distortion_mode="ndc"), dict(distortion_mode="ndc", distortion_far=0.1),
                dict(distortion_weight=1.0, pose_opt=True)):
        with pytest.raises(ValueError, match="distortion"):
            TrainConfig(**bad).check()


class _Trainer:
    """SplatTrainer's _check_step on a bare object: the refusals look at the configuration and the arguments only."""

    def __init__(self, config, it=0):
        from brush_amd.train import SplatTrainer

        self.config, self.iter, self.filter3d = config, it, None
        self._normal_active = lambda: SplatTrainer._normal_active(self)
        self._distortion_active = lambda: SplatTrainer._distortion_active(self)
        self.check = lambda **kw: SplatTrainer._check_step(self, **{**dict(
            grad_sync=None, exchange=None, view_index=None, poses=None, exposures=None, gt_depth=None), **kw})


def test_check_step_refusals(monkeypatch):
    from brush_amd import TrainConfig
    from brush_amd import render as Rn

    monkeypatch.setattr(Rn, "DETERMINISTIC", False)
    monkeypatch.delenv("BRUSH_DETERMINISTIC", raising=False)
    on = TrainConfig(distortion_weight=10.0, distortion_from_step=5)
    _Trainer(on, 5).check()
    for kw in (dict(exchange=object()), dict(grad_sync=object())):
        with pytest.raises(ValueError, match="distortion_weight.*single-view"):
            _Trainer(on, 5).check(**kw)
    with pytest.raises(ValueError, match="distortion_weight.*pose refinement"):
        _Trainer(on, 5).check(poses=object(), view_index=0)
    monkeypatch.setattr(Rn, "DETERMINISTIC", True)
    with pytest.raises(ValueError, match="distortion_weight.*deterministic mode"):
        _Trainer(on, 5).check()
    # off, or before distortion_from_step: nothing is refused
    for t in (_Trainer(on, 4), _Trainer(TrainConfig(), 9000)):
        t.check()
        t.check(poses=object(), view_index=0)
        t.check(grad_sync=object())


def test_command_lines_parse():
    from brush_amd import eval as E
    from brush_amd import train_loop as TL

    a = TL.parser().parse_args(["scene", "--distortion-weight", "100", "--distortion-from-step", "7",
                                "--distortion-mode", "ndc", "--distortion-far", "25"])
    assert (a.distortion_weight, a.distortion_from_step, a.distortion_mode, a.distortion_far) == (100.0, 7, "ndc", 25.0)
    a = TL.parser().parse_args(["scene"])
    assert (a.distortion_weight, a.distortion_from_step, a.distortion_mode) == (0.0, 3000, "depth")
    with pytest.raises(SystemExit):
        TL.parser().parse_args(["scene", "--distortion-mode", "disparity"])
    assert E.parser().parse_args(["s.ply", "scene", "--distortion-dir", "out"]).distortion_dir == "out"
    assert E.parser().parse_args(["s.ply", "scene"]).distortion_dir is None
    assert "distortion_weight" in TL.TrainLog(0, np.zeros(0, np.float32), distortion_weight=2.0).to_json()


# ---------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_entries_validate_before_any_device_work(lib):
    from brush_amd import _lib

    u = _lib.BrushUniforms()
    u.img_size[:] = [17, 9]
    u.tile_bounds[:] = [2, 1]
    aux = _lib.BrushAux()
    fake = 0x1000  # never dereferenced on the host: every call below is refused before a launch
    for name in ("projected_splats", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid", "num_visible"):
        setattr(aux, name, fake)
    aux.max_intersects = 8
    cfg = _lib.BrushDistortion(_lib.DISTORTION_NDC, 0.2, 50.0)
    U, A, K = C.byref(u), C.byref(aux), C.byref(cfg)
    fwd, grad = lib.brush_render_distortion, lib.brush_distortion_compact_grads
    ok_f = [U, A, fake, K, 4, fake, None]
    ok_g = [U, A, fake, K, fake, fake, 0, fake, None]  # n = 0: BRUSH_OK without a launch
    assert grad(*ok_g) == 0
    for call, ok, ptrs, aligned16 in ((fwd, ok_f, (0, 1, 2, 3, 5), (5,)), (grad, ok_g, (0, 1, 2, 3, 4, 5, 7), (4,))):
        for i in ptrs:
            args = list(ok)
            args[i] = None
            assert call(*args) == -1, i
        for i in aligned16:  # stats: 16-byte aligned
            args = list(ok)
            args[i] = fake + 4
            assert call(*args) == -1, i
        args = list(ok)
        args[2] = fake + 2  # f32: 4-byte aligned
        assert call(*args) == -1
        for bad in ((2, 0.2, 50.0), (1, 0.0, 50.0), (1, 0.2, 0.2), (1, 0.2, float("inf")), (1, float("nan"), 50.0)):
            b = _lib.BrushDistortion(*bad)
            args = list(ok)
            args[3] = C.byref(b)
            assert call(*args) == -1, bad
        u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
        assert call(*ok) == -1
        u.tile_bounds[:] = [2, 1]
    # deterministic mode: both gradient entries refuse, the forward replay does not look at the flag
    aux.flags = _lib.AUX_DETERMINISTIC
    assert grad(*ok_g) == -1
    bwd = lib.brush_render_backward_distortion
    for flags, want in ((_lib.AUX_DETERMINISTIC, -1),):
        aux.flags = flags
        for name in ("uniforms_buffer", "num_intersections", "final_index", "cum_tiles_hit", "compact_from_global_gid",
                     "overflow", "isect_unsorted_pos"):
            setattr(aux, name, fake)
        args = [U, A, fake, fake, fake, fake, 0, fake, fake, fake, fake, K, fake, fake, fake, fake, fake, fake, fake,
                fake, fake, 1 << 20, None]
        assert bwd(*args) == want
    aux.flags = 0
    for i in (9, 10, 11, 12, 13):  # compact_depth, v_depth, cfg, stats, v_distortion are required
        a2 = list(args)
        a2[i] = None
        assert bwd(*a2) == -1, i
