"""GPU checks of the depth backward (brush_render_backward_depth) in every launch form of its compositing kernel and
beyond the grid caps of its two depth-only kernels (tests/depth_form_scenes.py; the scenes' conditions and the
launchers' thresholds are asserted on the CPU by tests/test_depth_forms_cpu.py).

k_rasterize_backward_quad<NQ, DET, TPB, DepthGrad> takes NQ = 1 below 1100 tiles, NQ = 2 from 1100, NQ = 4 from 2304 and
<4, DET> in deterministic mode; every other depth-gradient test stays at 625 tiles or fewer.  Here:
  1. test_gpu_depth's linearity identity and forward twin on both sides of both switches and on `caps`, both modes;
  2. the depth gradient against the float64 arbiter element by element (test_gpu_depth.check_backward_arbiter), on the
     form scenes and on `ragged` / `c1`, so that the forms the older tests reach are held to the same gate;
  3. `caps`: the rows of k_depth_means_grad's second grid-stride trip (compact ids >= 524 288) and the sums of
     k_sum_isect_depth's second trip (more than 1 048 576 intersection rows, deterministic mode), directly;
  4. negative controls: the GPU's result FAILS the same gates against references with a dropped tail term, mixed-up
     quadrants, a depth channel that does not reach v_alpha, or column 2 of W for row 2."""
import numpy as np
import pytest

from tests import camera_cases as CC
from tests import depth_form_scenes as S
from tests import margins
from tests import test_gpu_depth as TD

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
ARBITER_SCENES = S.FORM_SCENES + ("ragged", "c1")


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    _states.clear()
    _caps.clear()


def _scene(kind):
    """(cloud, w, h, max_intersects): a scene of depth_form_scenes, or one of test_gpu_depth's."""
    if kind in S.FORM_SCENES or kind == S.CAPS:
        return S.scene(kind)
    return TD._scene(kind) + (None,)


def _record(section, ratios):
    for k, v in ratios.items():
        margins.record(section, k, v)
        margins.check_growth(section, k, v["worst"] if isinstance(v, dict) else v)


# ---------------------------------------------------------------------------- 1. the linearity identity at every form
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", S.FORM_SCENES + (S.CAPS,))
def test_backward_is_sum_of_colour_and_twin_parts(dev, kind, det):
    """The depth op, the colour op and the twin share one frame and therefore one form."""
    cloud, w, h, cap = _scene(kind)
    _record("depth_grad_linear", TD.check_backward_linearity(dev, kind, det, cloud, w, h, max_intersects=cap))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", S.FORM_SCENES + (S.CAPS,))
def test_forward_matches_depth_as_colour_twin(dev, kind, det):
    cloud, w, h, cap = _scene(kind)
    V, r_twin, r_oracle = TD.check_forward_twin(dev, kind, cloud, w, h, max_intersects=cap, det=det)
    assert V == S.facts(kind)["visible"]
    _record("depth_forward", {"twin": r_twin, "oracle": r_oracle})


# ---------------------------------------------------------------------------- 2. against the f64 arbiter
_states = {}  # (kind, det) -> arbiter_state, kept for the controls of section 4


def _state(dev, kind, det, keep=False):
    if (kind, det) in _states:
        return _states[kind, det]
    cloud, w, h, cap = _scene(kind)
    st = TD.arbiter_state(dev, kind, det, cloud, w, h, max_intersects=cap)
    if keep:
        _states[kind, det] = st
    return st


CONTROL_SCENES = ("at2_sparse", "at2_deep", "at4_sparse", "at4_deep")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ARBITER_SCENES)
def test_backward_against_f64_arbiter(dev, kind, det):
    st = _state(dev, kind, det, keep=kind in CONTROL_SCENES and not det)
    if kind in S.FORM_SCENES:
        assert st["V"] == S.facts(kind)["visible"]
    _record("depth_grad_arbiter", TD.arbiter_gate(st))


# ---------------------------------------------------------------------------- 3. beyond the grid caps
_caps = {}


def _caps_run(dev, det):
    """The depth op and the colour op on the twin under v_out = 0 and the usual v_D, on `caps`: (depth op's gradients,
    twin's v_means, v_z, compact order as global ids, row 2 of W), float64 except the first."""
    if det in _caps:
        return _caps[det]
    import torch

    cloud, w, h, cap = _scene(S.CAPS)
    _, v_d = TD._upstream(dev, w, h, seed=5)
    v_out = torch.zeros((h, w, 4), device=dev)
    got, _, aux = TD._grads(dev, cloud, w, h, det, v_out, v_d, max_intersects=cap)
    V, I = aux.read_num_visible(), aux.read_num_intersections()
    assert V > S.MEANS_GRAD_ONE_TRIP + 10_000 and I > S.ISECT_DEPTH_ONE_TRIP and int(aux.overflow.item()) == 0
    assert (V, I) == (S.facts(S.CAPS)["visible"], S.facts(S.CAPS)["intersections"])
    u = TD._u(aux, w, h, cloud)
    tw, _ = TD._twin(cloud, u)
    vt = torch.zeros_like(v_out)
    vt[..., 0] = v_d
    twin, _, _ = TD._grads(dev, tw, w, h, det, vt, max_intersects=cap)
    gids = TD._np_u32(aux.global_from_compact_gid)[:V].astype(np.int64)
    _caps[det] = (got, twin["v_means"].astype(np.float64),
                  twin["v_sh"][:, 0, 0].astype(np.float64) / float(TD.C0), gids, TD._z_row(u))
    return _caps[det]


def _norm(a):
    return np.sqrt((a * a).sum(axis=-1))


def check_caps_rows(dev, det, drop_tail_z=False):
    """Rows of v_means in compact order, ahead of and behind the first trip of k_depth_means_grad: the depth op's row is
    the twin's plus v_z times row 2 of W, within 1e-3 |want| + 64 eps32 (|twin v_means| + |v_z row|), | | the Euclidean
    norm of a ROW: the gate is on the row as a vector, as the rows test_depth_forms_cpu.py counts as strong are.
    (Component by component the same bound is missed by 192 of the 1 650 120 components, in both modes, by up to 830 x:
    x and y components that cancel to 1e-5 .. 1e-8 of the magnitudes they are summed from, where the depth op and the
    twin, which sees z through its f32 colour, are both within 1.5 eps32 of those magnitudes of the float64 arbiter, 46
    in deterministic mode.  Measured on an MI355X; as vectors the worst row is at 0.13 of the bound.)  `drop_tail_z`:
    the wrong reference of a kernel that never makes its second trip."""
    grads, t_means, v_z, gids, row = _caps_run(dev, det)
    got, worst, over = grads["v_means"], {}, {}
    for name, ids in (("ahead", gids[:S.MEANS_GRAD_ONE_TRIP]), ("behind", gids[S.MEANS_GRAD_ONE_TRIP:])):
        zterm = v_z[ids, None] * row[None, :]
        want = t_means[ids] + (0.0 if drop_tail_z and name == "behind" else zterm)
        tol = 1e-3 * _norm(want) + 64 * EPS32 * (_norm(t_means[ids]) + _norm(zterm))
        err = _norm(got[ids].astype(np.float64) - want)
        over[name] = int((err > tol).sum())
        worst[name] = float((err / (tol + 1e-300)).max())
        print(f"[caps det={det} {name}] {ids.size} rows, {int((v_z[ids] != 0).sum())} with v_z != 0, worst err/tol "
              f"{worst[name]:.3f}, {over[name]} rows over")
    for name in worst:
        assert over[name] == 0, f"caps det={det} rows {name} the cap: {over[name]} rows over, worst {worst[name]:.3f}"
    return worst


@pytest.mark.parametrize("det", [False, True])
def test_caps_rows_behind_the_grid_cap(dev, det):
    grads, _, v_z, gids, _ = _caps_run(dev, det)
    got = grads["v_means"]
    tail = gids[S.MEANS_GRAD_ONE_TRIP:]
    assert int((v_z[tail] != 0).sum()) >= 10_000  # the second trip has something to add
    _record("depth_caps_rows", check_caps_rows(dev, det))
    # off the visible set the rows stay exact zeros
    mask = np.ones(got.shape[0], bool)
    mask[gids] = False
    assert not got[mask].any()


@pytest.mark.parametrize("det", [False, True])
def test_caps_depth_gradient_against_f64_arbiter(dev, det):
    """The depth gradient alone (v_out = 0) on `caps`, every element against the float64 arbiter under the allowance of
    test_gpu_depth.arbiter_gate: the components the row gate above only sees through their row's norm."""
    cloud, w, h, cap = _scene(S.CAPS)
    st = TD.arbiter_state(dev, S.CAPS, det, cloud, w, h, max_intersects=cap, zero_v_out=True)
    assert st["V"] > S.MEANS_GRAD_ONE_TRIP + 10_000
    _record("depth_grad_arbiter", TD.arbiter_gate(st))


def test_caps_deterministic_backward_repeats_bitwise(dev):
    import torch

    cloud, w, h, cap = _scene(S.CAPS)
    _, v_d = TD._upstream(dev, w, h, seed=5)
    v_out = torch.zeros((h, w, 4), device=dev)
    a = _caps_run(dev, True)[0]
    b, _, _ = TD._grads(dev, cloud, w, h, True, v_out, v_d, max_intersects=cap)
    for k in TD.GRADS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.abs(a["v_means"]).max() > 0


# ---------------------------------------------------------------------------- 4. negative controls
@pytest.mark.parametrize("det", [False, True])
def test_control_dropped_tail_term_fails_the_caps_gate(dev, det):
    check_caps_rows(dev, det)
    with pytest.raises(AssertionError, match="rows behind the cap"):
        check_caps_rows(dev, det, drop_tail_z=True)


@pytest.mark.parametrize("control", ["rotate_quadrants", "no_depth_in_alpha"])
@pytest.mark.parametrize("kind", CONTROL_SCENES)
def test_control_wrong_reference_fails_the_arbiter_gate(dev, kind, control):
    st = _state(dev, kind, False)
    TD.arbiter_gate(st)
    with pytest.raises(AssertionError, match="against the f64 arbiter"):
        TD.arbiter_gate(st, control=control)
    cloud, w, h, cap = _scene(kind)
    for det in (False, True):  # and outside the linearity gate's fraction of the tensor's maximum, in both modes
        with pytest.raises(AssertionError, match=f"{kind} det={det} v_"):
            TD.check_backward_linearity(dev, kind, det, cloud, w, h, max_intersects=cap, control=control)


def test_control_quadrant_rotation_moves_every_quadrant():
    v = np.arange(20 * 36, dtype=np.float32).reshape(20, 36)
    r = TD._quadrants_rotated(v)
    assert np.array_equal(r[0:8, 8:16], v[0:8, 0:8]) and np.array_equal(r[8:16, 0:8], v[0:8, 8:16])
    assert np.array_equal(r[8:16, 8:16], v[8:16, 0:8]) and np.array_equal(r[0:8, 0:8], v[8:16, 8:16])
    assert np.array_equal(r[0:8, 24:32], v[0:8, 16:24])  # the second tile of the row likewise
    assert not r[16:20, 0:8].any() and np.array_equal(r[16:20, 8:16], v[16:20, 0:8])  # ragged rows: zero padding comes in


@pytest.mark.parametrize("kind", ["at2_sparse", "at2_deep"])
def test_control_column_2_fails_under_a_general_camera(dev, kind):
    """The scene co-moved in front of camera_cases' `general`: the gates pass with row 2 of W and fail with column 2."""
    cloud, w, h, cap = _scene(kind)
    moved, cam = CC.co_moved(cloud, w, h, "general"), CC.camera("general", w, h)
    tag = f"{kind}@general"
    TD.check_backward_linearity(dev, tag, False, moved, w, h, camera=cam, max_intersects=cap)
    if kind == "at2_sparse":
        # (on the deep scene the linearity gate's 1e-4 of the tensor's maximum is wider than the whole depth term: the
        # column mistake passes it there, measured, which is what the element-wise gate below is for)
        with pytest.raises(AssertionError, match="v_means"):
            TD.check_backward_linearity(dev, tag, False, moved, w, h, camera=cam, column=True, max_intersects=cap)
    st = TD.arbiter_state(dev, tag, False, moved, w, h, camera=cam, max_intersects=cap)
    TD.arbiter_gate(st)
    with pytest.raises(AssertionError, match="v_means"):
        TD.arbiter_gate(st, control="column")
