"""GPU checks of the accumulated depth, the antialiased mode and the camera-pose gradient away from the identity
camera (tests/camera_cases.py).

Every other test of these three features looks through the reference test camera, whose world-to-camera rotation W is
the identity: there row 2 of W is column 2, T = J W is J W^T, and a gradient sent through W^T is the one sent through W.
Here the same check bodies (test_gpu_depth.py, test_gpu_antialias.py, test_gpu_pose.py) run with their gates unchanged
on scenes moved rigidly in front of five general cameras, and on `ragged` under a camera that is not co-moved.  The
float64 references they compare with are pinned at these cameras by tests/test_general_camera_cpu.py.  The negative
controls at the end show that the GPU's output FAILS the same gates against references that carry such a W / W^T
mistake.  Scene conditions (visible count kept, flip-risk share <= 0.1 %) are asserted from the CPU oracle by
camera_cases.scene_at."""
import numpy as np
import pytest

from tests import camera_cases as CC
from tests import margins
from tests import pose_ref64 as P
from tests import test_general_camera_cpu as GC
from tests import test_gpu_antialias as TA
from tests import test_gpu_depth as TD
from tests import test_gpu_pose as TP

pytestmark = pytest.mark.gpu

SCENES = CC.GPU_SCENES
GOLDEN = tuple(s for s in SCENES if s[0] != "ragged")
CONTROLS = tuple((kind, name) for kind in ("tiny_case", "basic_case") for name in ("general", "tilt_x"))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    TP.write_margins()


def _at(kind, name, normalised=False):
    """(tag, cloud, w, h, camera)."""
    cloud, w, h, _ = CC.scene_at(kind, name, normalised)
    return f"{kind}@{name}", cloud, w, h, CC.camera(name, w, h)


def _record(section, ratios):
    for k, v in ratios.items():
        margins.record(section, k, v)
        margins.check_growth(section, k, v)


# ---------------------------------------------------------------------------- 1. depth
@pytest.mark.parametrize("kind,name", SCENES)
def test_depth_forward_matches_twin_and_oracle(dev, kind, name):
    tag, cloud, w, h, cam = _at(kind, name)
    V, r_twin, r_oracle = TD.check_forward_twin(dev, tag, cloud, w, h, camera=cam, max_risk=CC.MAX_FLIP_FRACTION)
    assert V == CC.scene_at(kind, name)[3]["visible"]
    _record("depth_forward", {"twin": r_twin, "oracle": r_oracle})


@pytest.mark.parametrize("kind,name", GOLDEN)
def test_depth_backward_against_oracle(dev, kind, name):
    tag, cloud, w, h, cam = _at(kind, name)
    _record("depth_grad_oracle", TD.check_backward_oracle(dev, tag, cloud, w, h, camera=cam))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind,name", SCENES)
def test_depth_backward_is_sum_of_colour_and_twin_parts(dev, kind, name, det):
    tag, cloud, w, h, cam = _at(kind, name)
    _record("depth_grad_linear", TD.check_backward_linearity(dev, tag, det, cloud, w, h, camera=cam))


@pytest.mark.parametrize("name", CC.CO_MOVED)
def test_depth_central_difference_wrt_means(dev, name):
    """test_gpu_depth's smooth scene co-moved in front of the camera (its own lens as the base)."""
    import torch

    _, means, log_scales, quats, sh, raw = TD._smooth_scene(dev)
    moved = CC.co_moved(dict(means=TD._np(means), quats=TD._np(quats)), 32, 32, name,
                        m_ref=CC.matrix64(CC.REFERENCE, 32, 32, base=TD.SMOOTH_CAMERA))
    cam = CC.camera(name, 32, 32, base=TD.SMOOTH_CAMERA)
    analytic, fd = TD.check_central_difference(dev, cam, torch.as_tensor(moved["means"], device=dev), log_scales,
                                               torch.as_tensor(moved["quats"], device=dev), sh, raw)
    print(f"[{name}] analytic {analytic:+.6e} fd {fd:+.6e}")
    assert abs(fd) > 1.0  # the derivative is resolved against the margin's absolute part


# ---------------------------------------------------------------------------- 2. antialias
@pytest.mark.parametrize("kind,name", SCENES)
def test_antialias_word8_against_aa_ref64(dev, kind, name):
    tag, cloud, w, h, cam = _at(kind, name)
    _record("aa_word8", {"err_over_bound": TA.check_word8(dev, tag, cloud, w, h, camera=cam)})


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind,name", SCENES)
def test_antialias_image_matches_oracle_twin(dev, kind, name, det):
    tag, cloud, w, h, cam = _at(kind, name)
    _record("aa_image", {"pixels": TA.check_image_oracle_twin(dev, tag, det, cloud, w, h, camera=cam)})


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind,name", SCENES)
def test_antialias_backward_against_oracle_twin(dev, kind, name, det):
    tag, cloud, w, h, cam = _at(kind, name)
    _record("aa_grad_oracle", TA.check_backward_oracle_twin(dev, tag, det, cloud, w, h, camera=cam))


# ---------------------------------------------------------------------------- 3. pose
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind,name", SCENES)
def test_pose_against_pose_ref64_on_the_oracle(dev, kind, name, det):
    """The three legs (plain, depth, antialiased); the ratios go to profiles/pose_margins.json under oracle/<scene>@
    <camera> ..."""
    tag, cloud, w, h, cam = _at(kind, name, normalised=True)
    TP.check_against_pose_ref64(dev, tag, det, cloud, w, h, camera=cam)


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind,name", SCENES)
def test_pose_rigid_identities(dev, kind, name, det, aa):
    """identity_sides with a real W: K_ROT / K_TR as counted in pose_ref64 (the W products are part of the count)."""
    tag, cloud, w, h, cam = _at(kind, name, normalised=True)
    TP.check_rigid_identities(dev, tag, det, aa, cloud, w, h, camera=cam)


def test_pose_autograd_viewmat_gradient_is_the_abi_rows(dev):
    """render_splats_pose under `general`: the [4,4] viewmat gradient holds the ABI's [3,4] rows and a last row of
    zeros; the dense gradients and the image are those of the ABI call."""
    import torch

    import brush_amd

    tag, cloud, w, h, cam = _at("ragged", "general", normalised=True)
    v_out, v_d = TD._upstream(dev, w, h, seed=4)
    M0 = torch.from_numpy(cam.world_to_local())
    assert np.array_equal(M0.numpy().astype(np.float64), CC.matrix64("general", w, h))
    for depth in (False, True):
        t = TD._tensors(cloud, dev, grad=True)
        vm = M0.clone().requires_grad_(True)
        res = brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), vm, deterministic=True, depth=depth)
        outs, gos = ([res[0], res[1]], [v_out, v_d]) if depth else ([res[0]], [v_out])
        ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"], vm]
        gr = torch.autograd.grad(outs, ps, gos)
        img0, _, _, g0, vv = TP._call(dev, cloud, w, h, True, False, v_out, v_d if depth else None, camera=cam)
        assert TD._np(res[0]).tobytes() == TD._np(img0).tobytes()
        for k, x in zip(TP.GRADS, gr[:6]):
            assert TD._np(x).tobytes() == g0[k].tobytes(), k
        gv = gr[6]
        assert gv.device.type == "cpu" and gv.shape == (4, 4) and gv.dtype == torch.float32
        assert np.abs(vv).max() > 0 and gv[:3].numpy().tobytes() == vv.tobytes() and not gv[3].any()


@pytest.mark.parametrize("aa", [False, True])
def test_pose_deterministic_calls_repeat_bitwise(dev, aa):
    tag, cloud, w, h, cam = _at("ragged", "general", normalised=True)
    v_out, v_d = TD._upstream(dev, w, h, seed=7)
    a = TP._call(dev, cloud, w, h, True, aa, v_out, v_d, camera=cam)
    b = TP._call(dev, cloud, w, h, True, aa, v_out, v_d, camera=cam)
    assert a[4].tobytes() == b[4].tobytes() and np.abs(a[4]).max() > 0
    for k in TP.GRADS:
        assert a[3][k].tobytes() == b[3][k].tobytes(), k


# ---------------------------------------------------------------------------- 4. negative controls
@pytest.mark.parametrize("kind,name", CONTROLS)
def test_control_gpu_v_means_fails_the_gate_against_column_2(dev, kind, name):
    """The GPU's v_means with a depth gradient against references whose depth term is v_z times COLUMN 2 of W: outside
    the oracle gate and the linearity gate, in v_means."""
    tag, cloud, w, h, cam = _at(kind, name)
    with pytest.raises(AssertionError, match="v_means"):
        TD.check_backward_oracle(dev, tag, cloud, w, h, camera=cam, column=True)
    for det in (False, True):
        with pytest.raises(AssertionError, match="v_means"):
            TD.check_backward_linearity(dev, tag, det, cloud, w, h, camera=cam, column=True)


@pytest.mark.parametrize("mutate", P.MUTATIONS)
@pytest.mark.parametrize("kind,name", CONTROLS)
def test_control_gpu_v_viewmat_fails_the_gate_against_w_transposed(dev, kind, name, mutate):
    """The GPU's v_viewmat against pose_ref64 with one W / W^T swap: outside the gate on every leg."""
    tag, cloud, w, h, cam = _at(kind, name, normalised=True)
    for leg in ("plain", "depth", "antialiased"):
        with pytest.raises(AssertionError, match=leg):
            TP.check_against_pose_ref64(dev, tag, False, cloud, w, h, camera=cam, mutate=mutate, legs=(leg,))


# ---------------------------------------------------------------------------- 5. pose fit
def test_pose_fit_recovers_a_perturbed_general_camera(dev):
    """test_gpu_pose's fit on the problem co-moved with `general` (rehearsed on the oracle by
    test_general_camera_cpu.py): below one tenth of the initial rotation and translation error."""
    cloud, _, w, h = GC.fit_problem_at("general")
    TP.check_pose_fit(dev, cloud, CC.camera("general", w, h), "pose_fit@general")
